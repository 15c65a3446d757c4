"""BatchedMiniWorld: N MiniWorld environments stepped and rendered on one MI355X.

Thin host object over the C ABI (include/miniworld_batch.h).  PyTorch is used only as plumbing:
device tensors for actions / zero-copy views of the library's output buffers, and the current HIP
stream.  All simulation and rendering runs in the HIP kernels of csrc/.
"""
import ctypes
import functools
import os

import numpy as np

from . import _lib
from .params import DEFAULT_PARAMS, sim_to_real_params
from .tasks import task_facts

TEX_FILES = ["floor_tiles_bw_1", "concrete_1", "concrete_2", "concrete_3", "concrete_4", "concrete_tiles_1",
             "brick_wall_1",
             # the sim-to-real rinks' choices (envs/simtorealgoto.py:52-66); uploaded only for those tasks
             "cardboard_1", "cardboard_2", "cardboard_3", "cardboard_4", "wood_1", "wood_2", "wood_planks_1",
             "drywall_1", "stucco_1", "ceiling_tiles_1",
             # the tasks with mesh entities / frames: room textures, the ImageFrame's picture, the images of the textured meshes, and
             # for Sign nine variants of each character of its words (Texture.get probes <name>_1 .. _9, opengl.py:50-58)
             "asphalt_1", "slime_1", "cinder_blocks_1", "logo_mila_1",
             "../meshes/medkit", "../meshes/duckie", "../meshes/building", "../meshes/cone"] + \
            ["chars/ch_0x%d_%d" % (ord(c), v) for c in "BLUERDGN" for v in range(1, 10)]
TEX_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "textures")


def _sign_params():   # Sign.__init__, sign.py:62-64
    p = DEFAULT_PARAMS.no_random()
    p.set("forward_step", 0.7)
    p.set("turn_step", 45)
    return p

# registered ids of the reference (envs/__init__.py:43-49) that this package covers:
# id -> (task, task_args, max_episode_steps or 0 for the class default, params override)
def _fast_params(forward_step=0.7, turn_step=45):   # envs/oneroom.py:52-66, envs/maze.py:123-141
    p = DEFAULT_PARAMS.no_random()
    p.set("forward_step", forward_step)
    p.set("turn_step", turn_step)
    return p


ENV_SPECS = {
    "MiniWorld-Hallway-v0": ("Hallway", [12], 0, None, None),
    "MiniWorld-OneRoom-v0": ("OneRoom", [10], 0, None, None),
    "MiniWorld-OneRoomS6-v0": ("OneRoom", [6], 100, None, None),
    "MiniWorld-OneRoomS6Fast-v0": ("OneRoom", [6], 50, _fast_params, False),
    "MiniWorld-FourRooms-v0": ("FourRooms", [], 0, None, None),
    "MiniWorld-Maze-v0": ("Maze", [8, 8, 3], 0, None, None),
    "MiniWorld-MazeS2-v0": ("Maze", [2, 2, 3], 0, None, None),
    "MiniWorld-MazeS3-v0": ("Maze", [3, 3, 3], 0, None, None),
    "MiniWorld-MazeS3Fast-v0": ("Maze", [3, 3, 3], 300, _fast_params, False),
    # the T-maze family (envs/tmaze.py); task_args as documented at MWB_TASK_TMAZE / MWB_TASK_TMAZE_TWOBOX
    "MiniWorld-TMaze-v0": ("TMaze", [0, 0, 0, 0], 0, None, None),
    "MiniWorld-TMazeLeft-v0": ("TMaze", [1, 10, -6, 0], 0, None, None),      # tmaze.py:69-71
    "MiniWorld-TMazeRight-v0": ("TMaze", [1, 10, 6, 0], 0, None, None),      # tmaze.py:73-75
    "MiniWorld-TMazeDynamic-v0": ("TMaze", [1, 10, -6, 100], 0, None, None),  # tmaze.py:77-96
    "MiniWorld-TMazeTwoBoxDynamic-v0": ("TMazeTwoBox", [0, 0, 0, 100], 0, None, None),                  # tmaze.py:108-149
    "MiniWorld-TMazeTwoBoxDynamicFeatures100K-v0": ("TMazeTwoBox", [1, 0, 0, 100000], 0, None, None),  # tmaze.py:220-251
    "MiniWorld-TMazeTwoBoxDynamicFeatures1M-v0": ("TMazeTwoBox", [1, 0, 0, 1000000], 0, None, None),
    "MiniWorld-TMazeTwoBoxDynamicFeatures10M-v0": ("TMazeTwoBox", [1, 0, 0, 10000000], 0, None, None),
    "MiniWorld-TMazeTwoBoxDynamicFeaturesDebug-v0": ("TMazeTwoBox", [1, 0, 0, 9000000000000], 0, None, None),
    # the sim-to-real rinks: own parameter table, domain randomisation forced on (simtorealgoto.py:27-33)
    "MiniWorld-SimToRealGoTo-v0": ("SimToRealGoTo", [], 0, sim_to_real_params, True),
    "MiniWorld-SimToRealPush-v0": ("SimToRealPush", [], 0, lambda: sim_to_real_params(push=True), True),
    # several boxes + the carry actions, envs/putnext.py
    "MiniWorld-PutNext-v0": ("PutNext", [12], 0, None, None),
    # rooms that are general convex polygons, envs/ymaze.py; task_args {goal given, x, z}
    "MiniWorld-YMaze-v0": ("YMaze", [0, 0, 0], 0, None, None),
    "MiniWorld-YMazeLeft-v0": ("YMaze", [1, 3.9, -7.0], 0, None, None),    # ymaze.py:96-98
    "MiniWorld-YMazeRight-v0": ("YMaze", [1, 3.9, 7.0], 0, None, None),    # ymaze.py:100-102
    # a general entity list: mesh entities (Ball, Key, MeshEnt), frames, entities leaving / re-entering the list
    "MiniWorld-PickupObjs-v0": ("PickupObjs", [12, 5], 0, None, None),         # pickupobjs.py:13-22
    "MiniWorld-RoomObjs-v0": ("RoomObjs", [10], 0, None, None),                # roomobjs.py:14-21
    "MiniWorld-CollectHealth-v0": ("CollectHealth", [16], 0, None, None),      # collecthealth.py:19-26
    "MiniWorld-ThreeRooms-v0": ("ThreeRooms", [], 0, None, None),              # threerooms.py:12-20: two openings in one wall
    "MiniWorld-Sign-v0": ("Sign", [10, 0, 0], 0, _sign_params, False),         # sign.py:41-71: its own params, domain_rand forced off
    "MiniWorld-Sidewalk-v0": ("Sidewalk", [], 0, None, None),
    "MiniWorld-WallGap-v0": ("WallGap", [], 0, None, None),
}



_BVH_CACHE = {}


def check_copy_indices(dst_idx, src_idx, n_dst, n_src, same_handle):
    """The rules mwb_copy_envs applies to its (destination, source) pairs on the device (csrc/mwb_copy_check.h), for index lists
    that live on the host: raises ValueError where the device would reject a pair - an index outside [0, n_dst) / [0, n_src), a
    destination named by more than one pair, or, on one handle, a destination that is also some pair's source (dst == src is
    valid there and copies nothing).  Returns the two lists as int32 arrays."""
    d = np.asarray(dst_idx)
    s = np.asarray(src_idx)
    if d.ndim != 1 or s.ndim != 1 or d.shape != s.shape:
        raise ValueError("copy_envs: dst_idx and src_idx must be one-dimensional and of equal length (%s, %s)" % (d.shape, s.shape))
    if d.size and not (np.issubdtype(d.dtype, np.integer) and np.issubdtype(s.dtype, np.integer)):
        raise ValueError("copy_envs: indices must be integers")
    d, s = d.astype(np.int64), s.astype(np.int64)
    bad = (d < 0) | (d >= n_dst)
    if bad.any():
        raise ValueError("copy_envs: destination index %d outside [0, %d)" % (d[bad][0], n_dst))
    bad = (s < 0) | (s >= n_src)
    if bad.any():
        raise ValueError("copy_envs: source index %d outside [0, %d)" % (s[bad][0], n_src))
    uniq, counts = np.unique(d, return_counts=True)
    if (counts > 1).any():
        raise ValueError("copy_envs: env %d is the destination of more than one pair" % uniq[counts > 1][0])
    if same_handle:
        moved = d != s   # an identity pair copies nothing
        both = np.intersect1d(d[moved], s[moved])
        if both.size:
            raise ValueError("copy_envs: env %d is a destination and a source of the same call" % both[0])
    return d.astype(np.int32), s.astype(np.int32)


def check_repeat_args(repeat, num_envs, n_actions, n_skip=None, n_counts=None, name="step_repeat: repeat"):
    """What step_repeat refuses before anything is launched: raises ValueError for a `repeat` that is no integer in
    1 .. MAX_REPEAT (mwb_step_repeat would answer MWB_EINVAL) and for actions / skip_mask / counts that do not have one entry
    per env.  `name`: what the messages call `repeat` (the VecEnv views check their frame_skip with it).  Returns repeat as an int."""
    if isinstance(repeat, bool) or not isinstance(repeat, (int, np.integer)):
        raise ValueError("%s must be an integer, not %r" % (name, repeat))
    if not 1 <= int(repeat) <= _lib.MAX_REPEAT:
        raise ValueError("%s %d outside 1 .. %d" % (name, repeat, _lib.MAX_REPEAT))
    for what, n in (("actions", n_actions), ("skip_mask", n_skip), ("counts", n_counts)):
        if n is not None and int(n) != int(num_envs):
            raise ValueError("step_repeat: %s has %d entries for %d envs" % (what, n, num_envs))
    return int(repeat)


def _check_index_list(index, limit, what, limit_text):
    """the shared body of the two checks below -> the list as a one-dimensional int64 array"""
    a = np.asarray(index)
    if a.size == 0:
        raise ValueError("rollout %s: the index list is empty" % what)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("rollout %s: indices must be integers, not %s" % (what, a.dtype))
    a = a.reshape(-1).astype(np.int64)
    if (a < 0).any():
        raise ValueError("rollout %s: negative index %d" % (what, a[a < 0][0]))
    if (a >= limit).any():
        raise ValueError("rollout %s: index %d outside [0, %d) = %s" % (what, a[a >= limit][0], limit, limit_text))
    return a


def check_rollout_indices(index, cursor, num_envs):
    """What Rollout.gather refuses before anything is launched, for an index list that lives on the host: raises ValueError for
    an empty list, for indices that are no integers and for an index outside [0, (cursor + 1) * num_envs) - a row the device
    would write as zeros and count (mwb_rollout_rejected).  index[i] = t * num_envs + e, t in 0 .. cursor.  Returns the list as
    a one-dimensional int64 array."""
    return _check_index_list(index, (int(cursor) + 1) * int(num_envs), "gather", "(cursor + 1) * num_envs with the cursor at %d" % cursor)


def check_rollout_column_indices(index, num_steps, num_envs):
    """What Rollout.minibatch refuses before anything is launched, for an index list that lives on the host: as
    check_rollout_indices, with the bound of the reference's [:-1] views: index[i] = t * num_envs + e with t in 0 .. num_steps - 1,
    so an index outside [0, num_steps * num_envs) raises ValueError."""
    return _check_index_list(index, int(num_steps) * int(num_envs), "minibatch", "num_steps * num_envs")


class Augment:
    """A per-row random window for Rollout.gather / obs / minibatch / feed_forward_generator (mwb_rollout_gather_window): the image
    augmentation of a minibatch applied while the rows are rebuilt from their single frames.  One draw per stacked observation,
    shared by all of its frames:
        Augment.shift(pad, seed=0)        DrQ / RAD random shift: replicate-pad by pad, crop back to W x H
        Augment.crop(w, h, seed=0)        random crop to w x h <= W x H
        Augment.center_crop(w, h)         the evaluation counterpart of crop
        Augment.translate(w, h, seed=0)   the frame at a random place of a black w x h >= W x H canvas
    `seed` and the counter `calls` key the draw (csrc/mwb_rollout_window_map.h): the offsets of gather index i in call c are
    offsets_of([i], c) wherever a permutation puts the row.  An Augment is bound to a frame size at first use (bind)."""

    def __init__(self, kind, a, b=None, seed=0):
        if kind not in ("shift", "crop", "center_crop", "translate"):
            raise ValueError("Augment: unknown kind %r" % (kind,))
        for v in (a,) if kind == "shift" else (a, b):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("Augment.%s: integer parameters required, not %r" % (kind, v))
        if kind == "shift" and not 0 <= a <= _lib.WINDOW_MAX_OFFSET:
            raise ValueError("Augment.shift: pad %d outside 0 .. %d" % (a, _lib.WINDOW_MAX_OFFSET))
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
            raise ValueError("Augment: seed must be an integer, not %r" % (seed,))
        self.kind, self.params, self.seed, self.calls = kind, (int(a),) if kind == "shift" else (int(a), int(b)), int(seed) & _M64, 0
        self.frame = None    # (W, H) once bound
        self.window = None   # (out_w, out_h, border, dx_lo, dx_hi, dy_lo, dy_hi) once bound

    @classmethod
    def shift(cls, pad, seed=0):
        return cls("shift", pad, seed=seed)

    @classmethod
    def crop(cls, w, h, seed=0):
        return cls("crop", w, h, seed=seed)

    @classmethod
    def center_crop(cls, w, h):
        return cls("center_crop", w, h)

    @classmethod
    def translate(cls, w, h, seed=0):
        return cls("translate", w, h, seed=seed)

    def bind(self, W, H):
        """Fix the frame size the window is cut from -> the window (out_w, out_h, border, dx_lo, dx_hi, dy_lo, dy_hi).  ValueError
        for a second, different size, for a crop larger or a translate smaller than the frame and for a window outside the
        library's limits (out sizes 1 .. 1024, out_w * out_h a multiple of 4, bounds within -32767 .. 32767)."""
        W, H = int(W), int(H)
        if self.frame is not None:
            if self.frame != (W, H):
                raise ValueError("Augment.%s: bound to %d x %d frames, not %d x %d" % ((self.kind,) + self.frame + (W, H)))
            return self.window
        kind, p = self.kind, self.params
        if kind == "shift":
            win = (W, H, _lib.WINDOW_BORDER_EDGE, -p[0], p[0], -p[0], p[0])
        elif kind in ("crop", "center_crop"):
            w, h = p
            if not (1 <= w <= W and 1 <= h <= H):
                raise ValueError("Augment.%s: %d x %d does not fit the %d x %d frame" % (kind, w, h, W, H))
            mid = ((W - w) // 2, (H - h) // 2)
            win = (w, h, _lib.WINDOW_BORDER_EDGE) + ((0, W - w, 0, H - h) if kind == "crop" else (mid[0], mid[0], mid[1], mid[1]))
        else:
            w, h = p
            if w < W or h < H:
                raise ValueError("Augment.translate: the %d x %d canvas is smaller than the %d x %d frame" % (w, h, W, H))
            win = (w, h, _lib.WINDOW_BORDER_ZERO, -(w - W), 0, -(h - H), 0)
        if not (1 <= win[0] <= _lib.WINDOW_MAX_OUT and 1 <= win[1] <= _lib.WINDOW_MAX_OUT):
            raise ValueError("Augment.%s: output %d x %d outside 1 .. %d" % (kind, win[0], win[1], _lib.WINDOW_MAX_OUT))
        if (win[0] * win[1]) % 4:
            raise ValueError("Augment.%s: out_w * out_h = %d x %d must be a multiple of 4" % (kind, win[0], win[1]))
        if max(abs(v) for v in win[3:]) > _lib.WINDOW_MAX_OFFSET:
            raise ValueError("Augment.%s: offset bounds outside -%d .. %d" % (kind, _lib.WINDOW_MAX_OFFSET, _lib.WINDOW_MAX_OFFSET))
        self.frame, self.window = (W, H), win
        return win

    def offsets_of(self, index, call=None):
        """The draws of the gather indices `index` in call `call` (None: the next one, self.calls) -> int32 [B, 2] = (dx, dy):
        csrc/mwb_rollout_window_map.h restated with Python integers.  The Augment must be bound (bind, or a first gather)."""
        if self.window is None:
            raise ValueError("Augment.%s: not bound to a frame size yet (bind(W, H))" % self.kind)
        _, _, _, dx_lo, dx_hi, dy_lo, dy_hi = self.window
        call = self.calls if call is None else int(call)
        key = _mix64((self.seed + _GOLD * (call + 1)) & _M64)
        out = np.empty((np.size(index), 2), np.int32)
        for i, ix in enumerate(np.asarray(index, dtype=object).reshape(-1)):
            h = _mix64((key + _GOLD * ((int(ix) & _M64) + 1)) & _M64)
            out[i, 0] = dx_lo + (((h >> 32) * (dx_hi - dx_lo + 1)) >> 32)
            out[i, 1] = dy_lo + (((h & 0xffffffff) * (dy_hi - dy_lo + 1)) >> 32)
        return out

    def _struct(self, W, H):
        return _lib.MwbRolloutWindow(*self.bind(W, H), 0)


def check_window_offsets(offsets, count):
    """What Rollout.gather refuses before anything is launched, for offsets that live on the host: ValueError unless they are
    integers of shape [count, 2] that fit int32.  Returns them as an int32 array."""
    a = np.asarray(offsets)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("rollout gather: offsets must be integers, not %s" % a.dtype)
    if a.shape != (int(count), 2):
        raise ValueError("rollout gather: offsets of shape %s for %d rows ([B, 2] = (dx, dy) required)" % (a.shape, count))
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise ValueError("rollout gather: offsets must fit int32")
    return a.astype(np.int32)


class Rollout:
    """The observation half of RolloutStorage (pytorch-a2c-ppo-acktr/storage.py) on the device, every frame stored once
    (BatchedMiniWorld.rollout_enable; include/miniworld_batch.h at mwb_rollout_enable):
        ro.push(after_reset=True) after reset(), ro.push() after every step()     rollouts.obs[step + 1].copy_(obs) + insert()
        ro.gather(idx)                                                            obs[:-1].view(-1, ...)[idx]
        ro.gather(idx, augment=Augment.shift(4))                                  ... followed by the trainer's random shift / crop
        ro.after_update()                                                         rollouts.after_update()
    rewards [T, N], masks [T+1, N], features [T+1, N, 2] and ages [T+1, N] are zero-copy views of the library's arrays.

    With learner=True (or learner_enable()) the rest of RolloutStorage lives here as well (mwb_rollout_learner_enable):
        ro.insert(value, log_prob, action) after the push                          the small columns of rollouts.insert()
        ro.compute_returns(next_value, use_gae, gamma, tau)                        rollouts.compute_returns(), one kernel
        ro.compute_psi_returns(next_psi, gamma)                                    rollouts.compute_psi_returns()
        ro.feed_forward_generator(advantages, num_mini_batch)                      rollouts.feed_forward_generator()
    actions [T, N] int64, action_log_probs [T, N], value_preds [T+1, N], returns [T+1, N], advantages [T, N], psi_returns
    [T+1, N, 2] and taken [T, N] int32 - the sub-steps of every transition, by which the returns discount: gamma ** taken -
    are zero-copy views too.  The recurrent hidden states stay with the trainer (their width is the policy's)."""

    def __init__(self, batch, num_steps, nstack, grey, learner=False):
        torch = batch.torch
        self.batch, self.L, self.torch = batch, batch.L, torch
        _lib.check(self.L.mwb_rollout_enable(batch.h, int(num_steps), int(nstack), _lib.ROLLOUT_GREY if grey else 0))
        info = self._info()
        N = batch.num_envs
        self.num_steps, self.nstack, self.grey, self.num_envs = int(info.num_steps), int(info.nstack), bool(info.grey), N
        self.channels = self.nstack * (1 if self.grey else 3)
        self.nbytes = int(info.ring_bytes + info.reward_bytes + info.mask_bytes + info.feature_bytes + info.age_bytes)
        as_t = functools.partial(_dev_tensor, batch)
        T = self.num_steps
        self.rewards = as_t(info.reward, (T, N), "<f4")
        self.masks = as_t(info.mask, (T + 1, N), "<f4")
        self.features = as_t(info.feature, (T + 1, N, 2), "<f4")
        self.ages = as_t(info.age, (T + 1, N), "|u1")
        self._arange = torch.arange(N, dtype=torch.int64, device=batch.device)
        self._keep = None
        self.learner = False
        if learner:
            self.learner_enable()

    def learner_enable(self):
        """Allocate the learner half (mwb_rollout_learner_enable); from now on every push records `taken`"""
        torch, b = self.torch, self.batch
        _lib.check(self.L.mwb_rollout_learner_enable(b.h))
        info = _lib.MwbRolloutLearnerInfo()
        _lib.check(self.L.mwb_rollout_learner_info(b.h, ctypes.byref(info)))
        as_t = functools.partial(_dev_tensor, b)
        T, N = self.num_steps, self.num_envs
        self.actions = as_t(info.action, (T, N), "<i8")
        self.action_log_probs = as_t(info.log_prob, (T, N), "<f4")
        self.value_preds = as_t(info.value, (T + 1, N), "<f4")
        self.taken = as_t(info.taken, (T, N), "<i4")
        self.returns = as_t(info.ret, (T + 1, N), "<f4")
        self.advantages = as_t(info.adv, (T, N), "<f4")
        self.psi_returns = as_t(info.psi_ret, (T + 1, N, 2), "<f4")
        self.nbytes += int(info.action_bytes + info.log_prob_bytes + info.value_bytes + info.taken_bytes + info.ret_bytes
                           + info.adv_bytes + info.psi_ret_bytes)
        self.learner = True

    def _info(self):
        info = _lib.MwbRolloutInfo()
        _lib.check(self.L.mwb_rollout_info(self.batch.h, ctypes.byref(info)))
        return info

    @property
    def step(self):
        """the cursor: the last logical time pushed (0 after the reset push and after after_update; -1 before the first push)"""
        return int(self._info().cursor)

    @property
    def full(self):
        return self.step >= self.num_steps

    def push(self, after_reset=False, fresh=None):
        """Record the batch's current outputs as one time step.  fresh (uint8 / bool [N]): for passes that are not steps -
        batch.reset(mask) (pass the mask) or the destinations of a copy_envs: the named envs start a new history."""
        b = self.batch
        f = None
        if fresh is not None:
            fresh = self.torch.as_tensor(fresh).to(device=b.device, dtype=self.torch.uint8).reshape(-1).contiguous()
            if fresh.numel() != self.num_envs:
                raise ValueError("rollout push: fresh has %d entries for %d envs" % (fresh.numel(), self.num_envs))
            f = ctypes.c_void_p(fresh.data_ptr())
        _lib.check(self.L.mwb_rollout_push(b.h, int(bool(after_reset)), f, b._stream()))
        self._keep = fresh   # alive until the asynchronous kernel has consumed it

    def gather(self, index, dtype=None, augment=None, offsets=None, return_offsets=False):
        """index[i] = t * N + e, t in 0 .. step -> [B, nstack * C, W, H]: the stacked observations VecPyTorchFrameStack held at
        those steps, bit for bit; float32, or dtype=torch.uint8 (RGB only).  A LongTensor on the batch's device is read in
        place, without synchronisation: a row whose index is out of range comes back as zeros and is counted (rejected()).
        Anything that lives on the host is checked first by check_rollout_indices: ValueError, nothing is launched.

        augment (an Augment): the rows come back through its window, [B, nstack * C, out_w, out_h], in the same single pass
        (mwb_rollout_gather_window).  offsets=None draws every row's (dx, dy) on the device with (augment.seed, augment.calls) and
        then increments augment.calls; an int32 [B, 2] tensor on the batch's device is read in place and clamped to the window's
        ranges on the device; host data is checked first (check_window_offsets).  return_offsets=True: (rows, the clamped int32
        [B, 2] device tensor that was used)."""
        torch, b = self.torch, self.batch
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError("rollout gather: dtype must be torch.float32 or torch.uint8")
        if augment is None and (offsets is not None or return_offsets):
            raise ValueError("rollout gather: offsets / return_offsets need an augment")
        win = None if augment is None else augment._struct(b.W, b.H)   # ValueError before anything is launched
        if torch.is_tensor(index) and index.device == b.device:
            idx = index.reshape(-1).to(torch.int64).contiguous()
        else:
            host = index.cpu().numpy() if torch.is_tensor(index) else index
            idx = torch.from_numpy(check_rollout_indices(host, self.step, self.num_envs)).to(b.device)
        if augment is not None:
            out, used = self._gather_window(idx, dtype, augment, win, offsets, None)
            return (out, used) if return_offsets else out
        out = torch.empty((idx.numel(), self.channels, b.W, b.H), dtype=dtype, device=b.device)
        _lib.check(self.L.mwb_rollout_gather(b.h, ctypes.c_void_p(idx.data_ptr()), int(idx.numel()), ctypes.c_void_p(out.data_ptr()),
                                             1 if dtype == torch.float32 else 0, b._stream()))
        self._keep_idx = idx
        return out

    def _gather_window(self, idx, dtype, augment, win, offsets, call):
        """the windowed gather of the device index list idx -> (rows, clamped offsets).  offsets None: drawn with call number
        `call`; call None: augment.calls, which then advances"""
        torch, b = self.torch, self.batch
        B = int(idx.numel())
        if offsets is None:
            offs = torch.empty((B, 2), dtype=torch.int32, device=b.device)
            number = augment.calls if call is None else call
            _lib.check(self.L.mwb_rollout_window_offsets(b.h, ctypes.byref(win), augment.seed, number, ctypes.c_void_p(idx.data_ptr()), B,
                                                         ctypes.c_void_p(offs.data_ptr()), b._stream()))
            if call is None:
                augment.calls += 1
            used = offs   # drawn inside the ranges
        else:
            if torch.is_tensor(offsets) and offsets.device == b.device:
                if offsets.dtype != torch.int32 or tuple(offsets.shape) != (B, 2):
                    raise ValueError("rollout gather: offsets on the device must be int32 [%d, 2], not %s %s" % (B, offsets.dtype, tuple(offsets.shape)))
                offs = offsets.contiguous()
            else:
                host = offsets.cpu().numpy() if torch.is_tensor(offsets) else offsets
                offs = torch.from_numpy(check_window_offsets(host, B)).to(b.device)
            lo = torch.tensor([win.dx_lo, win.dy_lo], dtype=torch.int32, device=b.device)
            hi = torch.tensor([win.dx_hi, win.dy_hi], dtype=torch.int32, device=b.device)
            used = torch.minimum(torch.maximum(offs, lo), hi)   # what the kernel computes from (it reads offs itself)
        out = torch.empty((B, self.channels, win.out_w, win.out_h), dtype=dtype, device=b.device)
        _lib.check(self.L.mwb_rollout_gather_window(b.h, ctypes.c_void_p(idx.data_ptr()), B, ctypes.byref(win), ctypes.c_void_p(offs.data_ptr()),
                                                    ctypes.c_void_p(out.data_ptr()), 1 if dtype == torch.float32 else 0, b._stream()))
        self._keep_idx, self._keep_offs = idx, offs
        return out, used

    def obs(self, t, dtype=None, augment=None):
        """rollouts.obs[t]: the stacked observations of every env at logical time t (0 .. step); augment: as gather()"""
        t = int(t)
        if not 0 <= t <= self.step:
            raise ValueError("rollout obs: t = %d outside 0 .. %d" % (t, self.step))
        return self.gather(self._arange + t * self.num_envs, dtype=dtype, augment=augment)

    def after_update(self):
        _lib.check(self.L.mwb_rollout_after_update(self.batch.h, self.batch._stream()))

    # ------------------------------------------------------------------------------- the learner half
    def _column(self, what, x, count, dtypes):
        """a caller's tensor as the contiguous device array the library reads: ValueError (nothing launched) unless it is a tensor
        on the batch's device, of one of `dtypes`, with `count` elements"""
        torch = self.torch
        if not torch.is_tensor(x) or x.device != self.batch.device:
            raise ValueError("rollout %s: a tensor on %s is required" % (what, self.batch.device))
        if x.dtype not in dtypes:
            raise ValueError("rollout %s: dtype %s, not %s" % (what, " or ".join(str(d) for d in dtypes), x.dtype))
        if x.numel() != count:
            raise ValueError("rollout %s: %d elements required, not %d" % (what, count, x.numel()))
        return x.reshape(-1).contiguous()

    def insert(self, value=None, log_prob=None, action=None):
        """value_preds[step - 1], action_log_probs[step - 1], actions[step - 1] of the transition that led to the last push
        (storage.py:57-61); None leaves that column as it is.  float32 [N] or [N, 1]; action int64 or int32."""
        torch, N = self.torch, self.num_envs
        v = None if value is None else self._column("insert: value", value, N, (torch.float32,))
        lp = None if log_prob is None else self._column("insert: log_prob", log_prob, N, (torch.float32,))
        a = None if action is None else self._column("insert: action", action, N, (torch.int64, torch.int32))
        ptr = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())   # noqa: E731
        a64, a32 = (a, None) if a is None or a.dtype == torch.int64 else (None, a)
        _lib.check(self.L.mwb_rollout_insert(self.batch.h, ptr(a64), ptr(a32), ptr(lp), ptr(v), self.batch._stream()))
        self._keep_cols = (v, lp, a)   # alive until the asynchronous kernel has consumed them

    def compute_returns(self, next_value, use_gae, gamma, tau, rewards=None):
        """RolloutStorage.compute_returns (storage.py:82-99) in one kernel, every transition discounted by gamma ** taken: fills
        returns, advantages (returns - value_preds, ppo.py:33) and value_preds[-1].  rewards [T, N]: read instead of the stored
        rewards (the sf=True branch's estimated rewards).  The rollout must be full."""
        torch, N = self.torch, self.num_envs
        nv = self._column("compute_returns: next_value", next_value, N, (torch.float32,))
        rw = None if rewards is None else self._column("compute_returns: rewards", rewards, self.num_steps * N, (torch.float32,))
        _lib.check(self.L.mwb_rollout_returns(self.batch.h, _lib.RETURNS_GAE if use_gae else _lib.RETURNS_DISCOUNTED, float(gamma), float(tau),
                                              ctypes.c_void_p(nv.data_ptr()), None, None if rw is None else ctypes.c_void_p(rw.data_ptr()),
                                              self.batch._stream()))
        self._keep_ret = (nv, rw)

    def compute_psi_returns(self, next_psi, gamma):
        """RolloutStorage.compute_psi_returns (storage.py:101-105): fills psi_returns from the stored features; next_psi [N, 2]"""
        np_ = self._column("compute_psi_returns: next_psi", next_psi, 2 * self.num_envs, (self.torch.float32,))
        _lib.check(self.L.mwb_rollout_returns(self.batch.h, _lib.RETURNS_PSI, float(gamma), 1.0, None, ctypes.c_void_p(np_.data_ptr()), None,
                                              self.batch._stream()))
        self._keep_ret = (np_,)

    def bootstrap_truncated(self, values, gamma):
        """The time-limit bootstrap (mwb_rollout_bootstrap): rewards[step - 1][e] += gamma ** taken * values[r] for every terminal
        row r of the last step() whose env e = terminal.row_env[r] ended by the clock alone (terminal.truncated) - a time-out is
        no terminal state, the return goes on with V(terminal observation).  values: float32 [capacity] or [capacity, 1] on the
        batch's device, V(terminal.rows); entries behind terminal.count are ignored.  Call after the push() of that step and
        before the batch's next pass; needs terminal_enable.  Envs whose row was dropped are skipped (terminal.dropped())."""
        b = self.batch
        if b.terminal is None:
            raise ValueError("rollout bootstrap_truncated: the batch has no terminal observations (terminal_enable)")
        if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.floating, np.integer)) or not np.isfinite(gamma):
            raise ValueError("rollout bootstrap_truncated: gamma must be a finite number, not %r" % (gamma,))
        v = self._column("bootstrap_truncated: values", values, b.terminal.capacity, (self.torch.float32,))
        _lib.check(self.L.mwb_rollout_bootstrap(b.h, ctypes.c_void_p(v.data_ptr()), float(gamma), b._stream()))
        self._keep_boot = v   # alive until the asynchronous kernel has consumed it

    def minibatch(self, index, advantages=None, augment=None):
        """index[i] = t * N + e with t in 0 .. T - 1 (the flat indices of the reference's [:-1] views) ->
        (obs, actions, returns, masks, old_log_probs, adv, values): obs as gather() returns it, the others [B, 1].  One gather and
        one kernel for the six small columns.  advantages [T, N]: the caller's (normalised) ones; None: the stored advantages.
        An index list on the host is checked first (check_rollout_column_indices: ValueError, nothing launched); a LongTensor on
        the device is read in place, a row out of range comes back as zeros and is counted (rejected()).
        augment (an Augment): obs is gather(index, augment=augment) - one draw, augment.calls advances; the columns are unchanged."""
        return self._minibatch(index, advantages, augment, None)

    def _minibatch(self, index, advantages, augment, call):
        torch, b = self.torch, self.batch
        win = None if augment is None else augment._struct(b.W, b.H)
        if torch.is_tensor(index) and index.device == b.device:
            idx = index.reshape(-1).to(torch.int64).contiguous()
        else:
            host = index.cpu().numpy() if torch.is_tensor(index) else index
            idx = torch.from_numpy(check_rollout_column_indices(host, self.num_steps, self.num_envs)).to(b.device)
        adv = None if advantages is None else self._column("minibatch: advantages", advantages, self.num_steps * self.num_envs, (torch.float32,))
        obs = self.gather(idx) if augment is None else self._gather_window(idx, torch.float32, augment, win, None, call)[0]
        B = idx.numel()
        cols = torch.empty((5, B, 1), dtype=torch.float32, device=b.device)
        act = torch.empty((B, 1), dtype=torch.int64, device=b.device)
        _lib.check(self.L.mwb_rollout_gather_cols(b.h, ctypes.c_void_p(idx.data_ptr()), int(B), None if adv is None else ctypes.c_void_p(adv.data_ptr()),
                                                  ctypes.c_void_p(cols.data_ptr()), ctypes.c_void_p(act.data_ptr()), b._stream()))
        self._keep_adv = adv
        return obs, act, cols[0], cols[4], cols[2], cols[3], cols[1]

    def feed_forward_generator(self, advantages, num_mini_batch, generator=None, augment=None):
        """RolloutStorage.feed_forward_generator (storage.py:110-131): yields (obs, None, actions, returns, masks, old_log_probs,
        adv_targ) - None where the reference has the recurrent hidden states - over a random permutation of the T * N transitions
        drawn on the device (generator: a torch.Generator of the batch's device), cut into batches of T * N // num_mini_batch as
        BatchSampler(drop_last=False) cuts them: the last one may be shorter.
        augment (an Augment): every obs comes through its window with ONE call number for the whole pass - augment.calls advances
        once, when the pass is exhausted - so every transition gets exactly one draw per epoch and a new one the next epoch."""
        torch = self.torch
        call = None if augment is None else augment.calls
        batch_size = self.num_steps * self.num_envs
        assert batch_size >= num_mini_batch, (
            "PPO requires the number of processes ({}) * number of steps ({}) = {} to be greater than or equal to the number of "
            "PPO mini batches ({}).".format(self.num_envs, self.num_steps, batch_size, num_mini_batch))
        mini_batch_size = batch_size // num_mini_batch
        perm = torch.randperm(batch_size, device=self.batch.device, generator=generator)
        for first in range(0, batch_size, mini_batch_size):
            obs, act, ret, mask, logp, adv, _ = self._minibatch(perm[first:first + mini_batch_size], advantages, augment, call)
            yield obs, None, act, ret, mask, logp, adv
        if augment is not None:
            augment.calls += 1

    def rejected(self):
        """rows of gathers whose index was out of range since the last call (synchronous)"""
        out = ctypes.c_ulonglong()
        _lib.check(self.L.mwb_rollout_rejected(self.batch.h, ctypes.byref(out)))
        return int(out.value)


def monitor_log_slots(total, capacity):
    """csrc/mwb_monitor_map.h restated once: the ring slots of the live records of the monitor's log, oldest first, for
    `total` episodes ever appended to a ring of `capacity` records (mwb_monitor_live / mwb_monitor_oldest / mwb_monitor_read_slot)"""
    total, capacity = int(total), int(capacity)
    live = min(total, capacity)
    oldest = 0 if total < capacity else total % capacity
    return [(oldest + i) % capacity for i in range(live)]


class Monitor:
    """The trainer's record of its own progress on the device (BatchedMiniWorld.monitor_enable; include/miniworld_batch.h at
    mwb_monitor_enable): per-env running return (float64, summed per episode), length in env steps and in step calls, the episode
    that ended last in every env, the log of the last `capacity` episodes in the order the reference's loop
        for idx, eps_done in enumerate(done): if eps_done: episode_rewards.append(...)     (pytorch-a2c-ppo-acktr/main.py:167-169)
    appends them, and for evaluation a table of every env's first quota_max episodes with a per-env quota.
        mon.update(skip_mask)      after every step (MiniWorldVecEnv(monitor=K) does it inside the step)
        mon.log(), mon.stats()     the deque, oldest first, and the statistics main.py:203-214 prints
        mon.set_quota(q)           from now on env e retires after q episodes: mon.retired is the next step's skip mask
    run_return, run_len, run_calls, last_return, last_len, last_calls, finished, retired, partial, logged [N] and tab_return,
    tab_len [quota_max, N] are zero-copy views of the library's arrays."""

    def __init__(self, batch, capacity, quota_max):
        torch = batch.torch
        self.batch, self.L, self.torch = batch, batch.L, torch
        _lib.check(self.L.mwb_monitor_enable(batch.h, int(capacity), int(quota_max)))
        info = _lib.MwbMonitorInfo()
        _lib.check(self.L.mwb_monitor_info(batch.h, ctypes.byref(info)))
        N, C, Q = int(info.num_envs), int(info.capacity), int(info.quota_max)
        self.num_envs, self.capacity, self.quota_max = N, C, Q
        as_t = functools.partial(_dev_tensor, batch)
        for name in ("run_return", "last_return"):
            setattr(self, name, as_t(getattr(info, name), (N,), "<f8"))
        for name in ("run_len", "run_calls", "last_len", "last_calls", "finished"):
            setattr(self, name, as_t(getattr(info, name), (N,), "<i4"))
        for name in ("partial", "retired", "logged"):
            setattr(self, name, as_t(getattr(info, name), (N,), "|u1"))
        self._log = (as_t(info.log_return, (C,), "<f8"), as_t(info.log_len, (C,), "<i4"), as_t(info.log_calls, (C,), "<i4"),
                     as_t(info.log_env, (C,), "<i4"))
        if Q:
            self.tab_return, self.tab_len = as_t(info.tab_return, (Q, N), "<f8"), as_t(info.tab_len, (Q, N), "<i4")
        else:
            self.tab_return = torch.empty((0, N), dtype=torch.float64, device=batch.device)
            self.tab_len = torch.empty((0, N), dtype=torch.int32, device=batch.device)
        # what a host-side consumer wants after every step, in one piece: last_return | last_len | last_calls | counts | logged | retired
        self.host_pack = as_t(info.host_pack, (int(info.host_pack_bytes),), "|u1")
        self.host_pack_offsets = {"last_return": 0, "last_len": 8 * N, "last_calls": 12 * N, "counts": 16 * N, "logged": 16 * N + 32,
                                  "retired": 17 * N + 32}
        assert int(info.host_pack_bytes) == 18 * N + 32 and ctypes.sizeof(_lib.MwbMonitorCounts) == 32
        self.quota = 0
        self._keep = None

    def _arg(self, x, dtype, what):
        if x is None:
            return None
        t = self.torch.as_tensor(x).to(device=self.batch.device, dtype=dtype).reshape(-1).contiguous()
        if t.numel() != self.num_envs:
            raise ValueError("monitor %s has %d entries for %d envs" % (what, t.numel(), self.num_envs))
        return t

    def update(self, skip_mask=None, reward=None, done=None, taken=None):
        """One pass (mwb_monitor_update) over the batch's own reward64 / done / sub-step counts, or over the arrays given in their
        place (float64 / uint8 / int32 [N]); skip_mask: the one the step was given."""
        torch = self.torch
        if skip_mask is None and reward is None and done is None and taken is None:   # the call of every step: no conversions
            rc = self.L.mwb_monitor_update(self.batch.h, None, None, None, None, self.batch._stream())
            if rc:
                _lib.check(rc)
            return
        ts = (self._arg(skip_mask, torch.uint8, "update: skip_mask"), self._arg(reward, torch.float64, "update: reward"),
              self._arg(done, torch.uint8, "update: done"), self._arg(taken, torch.int32, "update: taken"))
        ptr = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in ts]
        _lib.check(self.L.mwb_monitor_update(self.batch.h, ptr[0], ptr[1], ptr[2], ptr[3], self.batch._stream()))
        self._keep = ts   # alive until the asynchronous kernels have consumed them

    def clear(self, mask=None, partial=False):
        """Zero the accumulators of the masked envs (None: all).  partial=False: they start a fresh episode; partial=True: they
        are in the middle of an episode whose start was not seen, which is dropped, not logged, when it ends."""
        m = self._arg(mask, self.torch.uint8, "clear: mask")
        _lib.check(self.L.mwb_monitor_clear(self.batch.h, None if m is None else ctypes.c_void_p(m.data_ptr()), int(bool(partial)),
                                            self.batch._stream()))
        self._keep_clear = m

    def set_quota(self, q):
        """Per-env quota 0 .. quota_max (0: none): zeroes finished / retired, refills the table; the running episodes and the log stay."""
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 0 <= int(q) <= self.quota_max:
            raise ValueError("monitor quota %r outside 0 .. quota_max = %d" % (q, self.quota_max))
        _lib.check(self.L.mwb_monitor_quota(self.batch.h, int(q), self.batch._stream()))
        self.quota = int(q)

    def read(self):
        """(total, dropped, remaining): episodes ever logged, episodes dropped as partial, envs not retired (synchronous)"""
        c = _lib.MwbMonitorCounts()
        _lib.check(self.L.mwb_monitor_read(self.batch.h, ctypes.byref(c)))
        return int(c.total), int(c.dropped), int(c.remaining)

    def log(self):
        """The live records of the log, oldest first: (returns f64, lens i32, calls i32, envs i32) device tensors - what
        list(episode_rewards) holds, with the episode's length and env beside every return.  One read()."""
        total = self.read()[0]
        idx = self.torch.as_tensor(monitor_log_slots(total, self.capacity), dtype=self.torch.int64, device=self.batch.device)
        return tuple(a[idx] for a in self._log)

    def stats(self):
        """What the trainer prints at a log interval (main.py:203-214) from the log: n, mean, median, min, max, success_rate
        (returns > 0) and mean_len - computed by torch on the device views; an empty log gives n = 0 and None for the rest."""
        r, ln, _, _ = self.log()
        n = int(r.numel())
        if n == 0:
            return dict(n=0, mean=None, median=None, min=None, max=None, success_rate=None, mean_len=None)
        s = r.sort().values
        return dict(n=n, mean=float(r.sum()) / n, median=float((s[(n - 1) // 2] + s[n // 2]) / 2), min=float(s[0]), max=float(s[-1]),
                    success_rate=int((r > 0).sum()) / n, mean_len=float(ln.sum()) / n)


def check_terminal_args(capacity, num_envs, auto_reset=True, stack_args=None, dtype=None):
    """What terminal_enable refuses before anything is launched (mwb_terminal_enable would answer MWB_EINVAL): raises ValueError
    for a batch without auto-reset, for a `capacity` that is no integer in 1 .. num_envs (None: num_envs), for a frame stack
    that is not the fused one, and for a `dtype` other than "uint8" / "float32" or one that contradicts the stack's (the rows of a
    stacked batch take the stack's dtype).  stack_args: what stack_enable was given, or None.  Returns (capacity, rows are
    float32)."""
    if not auto_reset:
        raise ValueError("terminal_enable: the batch was created with auto_reset=False: its observation is the terminal frame already")
    if capacity is None:
        capacity = num_envs
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)):
        raise ValueError("terminal_enable: capacity must be an integer, not %r" % (capacity,))
    if not 1 <= int(capacity) <= int(num_envs):
        raise ValueError("terminal_enable: capacity %d outside 1 .. num_envs = %d" % (capacity, num_envs))
    if dtype not in (None, "uint8", "float32"):
        raise ValueError("terminal_enable: dtype must be 'uint8' or 'float32', not %r" % (dtype,))
    if stack_args is not None:
        if not stack_args.get("fused"):
            raise ValueError("terminal_enable: the frame stack is not the fused one (stack_enable(fused=True)): the terminal rows are "
                             "built from the fused window's history")
        if dtype is not None and dtype != stack_args["dtype"]:
            raise ValueError("terminal_enable: dtype %r, but the rows of a stacked batch take the stack's (%r)" % (dtype, stack_args["dtype"]))
        return int(capacity), stack_args["dtype"] == "float32"
    return int(capacity), dtype == "float32"


class Terminal:
    """What the auto-reset inside step() used to throw away (BatchedMiniWorld.terminal_enable; include/miniworld_batch.h at
    mwb_terminal_enable): the frame every episode ended on, why it ended, and the stacked observation the policy would have seen -
    the info["terminal_observation"] and info["TimeLimit.truncated"] of a modern VecEnv.  Zero-copy views, valid from the return
    of a step() until the batch's next pass:
        cause [N] uint8         END_CLOCK (1: step_count >= max_episode_steps) | END_TASK (2: a task rule), 0 = the episode goes on
        frames [N, ...]         shaped like obs: frames[e] is env e's frame at `done` wherever done[e] (stale elsewhere)
        grey [N, ...]           shaped like batch.grey (greyscale=True), else None
        count [1] int32         how many envs ended in the last step (may exceed capacity)
        row_of [N] int32        the compact row of env e's terminal observation, -1: it did not end, or count passed capacity
        row_env [capacity]      the env of row r, -1 behind the rows written
        rows [capacity, C * nstack, W, H]   the stacked terminal observations in the fused stack's dtype: the nstack - 1 frames
                                before the terminal one (zeros where the episode was shorter), then the terminal frame; without a
                                stack [capacity, ...] single frames shaped like obs, uint8 or float32
    reset(), reset(mask), render() and copy_envs() produce none: after them count = 0, row_of = -1, cause = 0."""

    def __init__(self, batch, capacity=None, dtype=None):
        torch = batch.torch
        self.batch, self.L, self.torch = batch, batch.L, torch
        capacity, is_float = check_terminal_args(capacity, batch.num_envs, batch._ctor["auto_reset"], batch._stack_args, dtype)
        _lib.check(self.L.mwb_terminal_enable(batch.h, capacity, _lib.TERMINAL_FLOAT if is_float and batch._stack_args is None else 0))
        info = _lib.MwbTerminalInfo()
        _lib.check(self.L.mwb_terminal_info(batch.h, ctypes.byref(info)))
        N, W, H, K = batch.num_envs, batch.W, batch.H, int(info.capacity)
        self.num_envs, self.capacity, self.nstack, self.channels = N, K, int(info.nstack), int(info.planes)
        as_t = functools.partial(_dev_tensor, batch)
        hwc = batch.layout == "HWC"
        self.cause = as_t(info.cause, (N,), "|u1")
        self.frames = as_t(info.frames, (N, H, W, 3) if hwc else (N, 3, W, H), "|u1")
        self.grey = as_t(info.grey, (N, H, W, 1) if hwc else (N, 1, W, H), "<f4") if info.grey else None
        self.row_of, self.row_env, self.count = as_t(info.row_of, (N,), "<i4"), as_t(info.row_env, (K,), "<i4"), as_t(info.count, (1,), "<i4")
        ts = "<f4" if info.rows_float else "|u1"
        if batch._stack_args is not None:
            self.rows = as_t(info.rows, (K, self.channels, W, H), ts)
        else:
            self.rows = as_t(info.rows, (K, H, W, 3) if hwc else (K, 3, W, H), ts)
        self.nbytes = int(info.frames_bytes + info.grey_bytes + info.rows_bytes)

    @property
    def truncated(self):
        """bool [N] on the device: the episode ended by the clock alone - the state is not terminal, bootstrap from it"""
        return self.cause == _lib.END_CLOCK

    @property
    def terminated(self):
        """bool [N] on the device: a task rule ended the episode (whatever the clock said)"""
        return (self.cause & _lib.END_TASK) != 0

    def dropped(self):
        """Ended envs that got no row because more than `capacity` ended in one step, since the last call (synchronous)"""
        n = ctypes.c_ulonglong()
        _lib.check(self.L.mwb_terminal_dropped(self.batch.h, ctypes.byref(n)))
        return int(n.value)


LEVEL_MODES = {"sequential": _lib.LEVELS_SEQUENTIAL, "uniform": _lib.LEVELS_UNIFORM, "table": _lib.LEVELS_TABLE}
_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def level_of(mode, g, n, L, stride=1, sampler_seed=0, request=-1):
    """The level of assignment n of the env with global index g in a set of L levels - csrc/mwb_levels_map.h restated with Python
    integers, for tests and for users who want to know ahead of time what an env will play.  mode: "sequential" ((g + n * stride)
    mod L), "uniform" (two rounds of splitmix64's mix over sampler_seed, g and n, then the high word of h * L), or "table" (the
    request where 0 <= request < L, the uniform level otherwise)."""
    mode = LEVEL_MODES[mode] if isinstance(mode, str) else int(mode)
    g, n, L = int(g), int(n), int(L)
    if mode == _lib.LEVELS_SEQUENTIAL:
        return (g + n * int(stride)) % L
    if mode == _lib.LEVELS_TABLE and 0 <= int(request) < L:
        return int(request)
    a = _mix64((int(sampler_seed) + _GOLD * (g + 1)) & _M64)
    h = _mix64((a + _GOLD * (n + 1)) & _M64)
    return (h * L) >> 64


def check_levels_args(num_levels, start_level=0, seeds=None, mode="uniform", sampler_seed=0, tally=True, env_stride=None, num_envs=1):
    """What levels_enable refuses before anything is created (mwb_levels_enable would answer MWB_EINVAL): raises ValueError for a
    num_levels that is no integer in 1 .. 2^31 - 1, a seed table of another length or of more than 2^24 levels, seeds or a start
    level outside uint64, an unknown mode, a stride below 1, tallies beyond 2^22 levels.  Returns (num_levels, start_level, seeds as
    a uint64 array or None, mode number, sampler_seed, tally, env_stride)."""
    def integer(x, what):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise ValueError("levels_enable: %s must be an integer, not %r" % (what, x))
        return int(x)
    L = integer(num_levels, "num_levels")
    if not 1 <= L <= _lib.LEVELS_MAX:
        raise ValueError("levels_enable: num_levels %d outside 1 .. 2^31 - 1" % L)
    start = integer(start_level, "start_level")
    sampler_seed = integer(sampler_seed, "sampler_seed")
    for what, x in (("start_level", start), ("sampler_seed", sampler_seed)):
        if not 0 <= x <= _M64:
            raise ValueError("levels_enable: %s %d outside uint64" % (what, x))
    if isinstance(mode, str) and mode in LEVEL_MODES:
        mode = LEVEL_MODES[mode]
    elif isinstance(mode, bool) or mode not in LEVEL_MODES.values():
        raise ValueError("levels_enable: mode must be one of %s, not %r" % (sorted(LEVEL_MODES), mode))
    table = None
    if seeds is not None:
        vals = [integer(x, "every seed") for x in (seeds.tolist() if isinstance(seeds, np.ndarray) else list(seeds))]
        if len(vals) != L:
            raise ValueError("levels_enable: %d seeds for num_levels = %d" % (len(vals), L))
        if L > _lib.LEVELS_MAX_TABLE:
            raise ValueError("levels_enable: a seed table holds at most 2^24 levels")
        if any(not 0 <= x <= _M64 for x in vals):
            raise ValueError("levels_enable: seeds outside uint64")
        table = np.array(vals, dtype=np.uint64)
    stride = max(1, int(num_envs)) if env_stride is None else integer(env_stride, "env_stride")
    if stride < 1:
        raise ValueError("levels_enable: env_stride %d < 1" % stride)
    if tally and L > _lib.LEVELS_MAX_TALLY:
        raise ValueError("levels_enable: tally=True takes at most 2^22 levels (num_levels = %d)" % L)
    return L, start, table, int(mode), sampler_seed, bool(tally), stride


class Levels:
    """A level set (BatchedMiniWorld.levels_enable; include/miniworld_batch.h at mwb_levels_enable): Procgen's num_levels /
    start_level for this batch.  Every regeneration of an env - the auto-reset inside step(), reset(mask), reset() - starts from the
    generator stream of a level seed chosen on the device, so the episode equals the first episode of a reference env after
    env.seed(level_seed); env.reset().  Zero-copy device views:
        index [N] int32        the level every env is in (-1 before its first assignment, or after a copy from a batch without levels)
        prev_index [N] int32   the level of its previous episode (-1: none)
        episode_no [N] int64   assignments since enable / restart()
        next_level [N] int32   mode "table": write the level an env is to play next; consumed (set to -1) when it is taken
        episodes, steps, successes [L] int64   with tally=True: per level, the episodes that ended in a step(), their env steps and
                               how many ended with a reward > 0 (the sparse-reward tasks' success; it means little for PickupObjs
                               and CollectHealth); None otherwise.  reset() abandons episodes and tallies nothing.
    The T-maze family's episode_count / task_step_count / goal_idx carry on across a regeneration, as across env.seed()."""

    def __init__(self, batch, args, env_offset):
        torch = batch.torch
        self.batch, self.L = batch, batch.L
        self.num_levels, self.start_level, self._seeds, self._mode, self._sampler_seed, self.tally, self.env_stride = args
        self.env_offset = int(env_offset)
        _lib.check(self.L.mwb_levels_enable(batch.h, self.num_levels, self.start_level,
                                            self._seeds.ctypes.data_as(ctypes.c_void_p) if self._seeds is not None else None, self._mode,
                                            self._sampler_seed, self.env_offset, self.env_stride, _lib.LEVELS_TALLY if self.tally else 0))
        info = _lib.MwbLevelsInfo()
        _lib.check(self.L.mwb_levels_info(batch.h, ctypes.byref(info)))
        N, nl = batch.num_envs, self.num_levels
        as_t = functools.partial(_dev_tensor, batch)
        self.index, self.prev_index = as_t(info.index, (N,), "<i4"), as_t(info.prev_index, (N,), "<i4")
        self.next_level, self.episode_no = as_t(info.next_level, (N,), "<i4"), as_t(info.episode_no, (N,), "<i8")
        self.index_pair = as_t(info.index, (2, N), "<i4")   # index | prev_index are one allocation: a VecEnv's host mirror is one copy
        assert info.prev_index == info.index + 4 * N
        self.episodes = self.steps = self.successes = None
        if info.tallies:   # (counts stay far below 2^63: int64 views of the uint64 words)
            t = as_t(info.tallies, (3, nl), "<i8")
            self.episodes, self.steps, self.successes = t[0], t[1], t[2]

    @property
    def mode(self):
        return {v: k for k, v in LEVEL_MODES.items()}[self._mode]

    @property
    def sampler_seed(self):
        return self._sampler_seed

    def params(self):
        """the keyword arguments that enable the same set on another batch (archive())"""
        return dict(num_levels=self.num_levels, start_level=self.start_level, seeds=self._seeds, mode=self._mode,
                    sampler_seed=self._sampler_seed, tally=self.tally, env_stride=self.env_stride)

    def restart(self, mode=None, sampler_seed=None, clear_tally=True):
        """episode_no = 0 for every env - the sequence of levels starts over - and, with clear_tally, zero tallies; mode and
        sampler_seed change where given.  A small kernel on the current stream; index and prev_index stay."""
        args = check_levels_args(1, 0, None, self._mode if mode is None else mode, self._sampler_seed if sampler_seed is None else sampler_seed, False, 1)
        _lib.check(self.L.mwb_levels_restart(self.batch.h, args[3], args[4], 1 if clear_tally else 0, self.batch._stream()))
        self._mode, self._sampler_seed = args[3], args[4]

    def rejected(self):
        """next_level entries other than -1 that were out of range since the last call (synchronous)"""
        n = ctypes.c_ulonglong()
        _lib.check(self.L.mwb_levels_rejected(self.batch.h, ctypes.byref(n)))
        return int(n.value)

    def seed_of(self, index):
        """level index (an int, or an array of them) -> its seed as a Python int (a list of them); -1 -> None.  Host arithmetic."""
        def one(i):
            i = int(i)
            if i < 0:
                return None
            if i >= self.num_levels:
                raise IndexError("level %d of %d" % (i, self.num_levels))
            return int(self._seeds[i]) if self._seeds is not None else (self.start_level + i) & _M64
        return one(index) if np.isscalar(index) else [one(i) for i in np.asarray(index).reshape(-1).tolist()]

    def level_of(self, env, n):
        """the level env `env` of this batch takes at its n-th assignment under the current mode (no request)"""
        return level_of(self._mode, self.env_offset + int(env), n, self.num_levels, self.env_stride, self._sampler_seed)


class _DevView:
    """Exposes a library-owned device buffer through __cuda_array_interface__ (zero-copy)."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}
        self._owner = owner   # keeps the handle alive while views exist


def _dev_tensor(owner, ptr, shape, typestr):
    """Zero-copy torch view of a library-owned device buffer of the BatchedMiniWorld `owner` (which the view keeps alive)."""
    return owner.torch.as_tensor(_DevView(ptr, shape, typestr, owner), device=owner.device)


class BatchedMiniWorld:
    """N environments of one task on one GPU.

    reset()/step() mirror VecEnv semantics of the reference's SubprocVecEnv worker
    (vec_env/subproc_vec_env.py:5-33): env i is seeded `seed + first_env_index + i`
    (pytorch-a2c-ppo-acktr/envs.py:36), a finished env is reset inside step() and the returned
    observation is the first one of the new episode while reward/done are the terminal ones.
    """

    def __init__(self, env_id="MiniWorld-OneRoom-v0", num_envs=1, seed=None, domain_rand=False, obs_width=80,
                 obs_height=60, want_depth=False, layout="HWC", device=0, max_episode_steps=None, params=None,
                 task=None, task_args=None, first_env_index=0, auto_reset=True, greyscale=False, _assets=True):
        import torch
        # what archive() builds a sibling from (before the env id's defaults are folded in: the sibling folds them in again)
        self._ctor = dict(env_id=env_id, domain_rand=domain_rand, obs_width=obs_width, obs_height=obs_height, want_depth=want_depth,
                          layout=layout, device=device, max_episode_steps=max_episode_steps, params=params, task=task,
                          task_args=task_args, auto_reset=auto_reset, greyscale=greyscale)
        self._stack_args = None
        self.monitor = None   # monitor_enable()
        self.terminal = None  # terminal_enable()
        self.levels = None    # levels_enable()
        self.torch = torch
        self.L = _lib.load()
        if task is None:
            if env_id not in ENV_SPECS:
                raise KeyError("unknown or out-of-scope env id %r; supported: %s" % (env_id, sorted(ENV_SPECS)))
            task, spec_args, spec_steps, spec_params, spec_dr = ENV_SPECS[env_id]
            task_args = spec_args if task_args is None else task_args
            if max_episode_steps is None:
                max_episode_steps = spec_steps
            if params is None and spec_params is not None:
                params = spec_params()
            if spec_dr is not None:
                domain_rand = spec_dr
        self.env_id, self.task = env_id, task
        self.task_args = list(task_args or []) + [0, 0, 0, 0]
        facts = task_facts(task, task_args, max_episode_steps)   # (tasks.py; the library resolves its own part in mwb_create)
        self.num_envs = int(num_envs)
        self.W, self.H = int(obs_width), int(obs_height)
        self.want_depth = bool(want_depth)
        self.layout = layout
        self.domain_rand = bool(domain_rand)
        self.params = params if params is not None else DEFAULT_PARAMS
        self.first_env_index = int(first_env_index)
        if not torch.cuda.is_available():
            raise _lib.MwbError("BatchedMiniWorld needs a GPU (torch.cuda.is_available() is False); no CPU path exists")
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)

        cfg = _lib.MwbConfig()
        cfg.abi_version = _lib.ABI_VERSION
        cfg.task = _lib.TASK_IDS[task]
        cfg.num_envs = self.num_envs
        cfg.obs_width, cfg.obs_height = self.W, self.H
        cfg.want_depth = int(self.want_depth)
        cfg.layout = {"HWC": _lib.LAYOUT_HWC, "CWH": _lib.LAYOUT_CWH}[layout]
        cfg.domain_rand = int(self.domain_rand)
        cfg.max_episode_steps = int(max_episode_steps or 0)
        cfg.device = self.device_index
        for i in range(4):
            cfg.task_args[i] = float(self.task_args[i])
        cfg.use_default_params = 0
        cfg.no_auto_reset = 0 if auto_reset else 1
        table = self.params.to_table()
        for i in range(_lib.NPARAM):
            for j in range(9):
                cfg.params[i][j] = float(table[i, j])
        h = ctypes.c_void_p()
        _lib.check(self.L.mwb_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.greyscale = bool(greyscale)
        if self.greyscale:   # before anything renders: the render kernels fill the grey buffer in the pass that writes obs
            _lib.check(self.L.mwb_grey_enable(self.h))
        if _assets:   # (an archive is never rendered or reset: it needs neither textures nor meshes)
            self._load_textures()
            if facts.meshes:
                self._load_meshes(facts.meshes)
        out = _lib.MwbOutputs()
        _lib.check(self.L.mwb_get_outputs(self.h, ctypes.byref(out)))
        N, W, H = self.num_envs, self.W, self.H
        obs_shape = (N, H, W, 3) if layout == "HWC" else (N, 3, W, H)
        as_t = functools.partial(_dev_tensor, self)
        self.obs = as_t(out.obs, obs_shape, "|u1")
        self.depth = as_t(out.depth, (N, H, W, 1), "<f4") if self.want_depth else None
        # GreyscaleWrapper's observation as float32 (wrappers.py:29-45 + .float()): [N,H,W,1], or [N,1,W,H] transposed; zero-copy
        self.grey = None
        if self.greyscale:
            gp, gb = ctypes.c_void_p(), ctypes.c_size_t()
            _lib.check(self.L.mwb_grey_output(self.h, ctypes.byref(gp), ctypes.byref(gb)))
            assert gb.value == N * W * H * 4
            self.grey = as_t(gp.value, (N, H, W, 1) if layout == "HWC" else (N, 1, W, H), "<f4")
        self.reward = as_t(out.reward, (N,), "<f4")
        self.reward64 = as_t(out.reward64, (N,), "<f8")
        self.done = as_t(out.done, (N,), "|u1")
        self.ep_steps = as_t(out.ep_steps, (N,), "<i4")
        self.feature = as_t(out.feature, (N, 2), "<f4")     # info['feature'] (tmaze.py:311-318); zeros elsewhere
        self.goal_pos = as_t(out.goal_pos, (N, 3), "<f8")   # info['goal_pos'] of the T-maze family
        # the six small outputs above are parts of one allocation: a host-side consumer copies `pack` once per step
        self.pack = as_t(out.pack, (out.pack_bytes,), "|u1")
        self.pack_offsets = {k: int(getattr(out, k)) - int(out.pack) for k in ("reward64", "goal_pos", "reward", "feature", "ep_steps", "done")}
        tp = ctypes.c_void_p()
        _lib.check(self.L.mwb_repeat_taken(self.h, ctypes.byref(tp)))
        self.taken = as_t(tp.value, (N,), "<i4")   # sub-steps every env took in the last step_repeat (zero-copy)
        self.n_boxes = int(self.L.mwb_num_boxes(self.h))   # 1; 2 (TMazeTwoBox, SimToRealPush); 6 (PutNext)
        self.ent_task = _lib.TASK_IDS[task] >= _lib.ENT_TASK_FIRST
        self.max_episode_steps, self.agent_radius, self.n_actions = facts.max_episode_steps, facts.agent_radius, facts.n_actions
        self.has_health, self.has_features, self.has_goal_pos = facts.has_health, facts.has_features, facts.has_goal_pos
        if seed is not None:
            self.seed(seed)

    def _load_textures(self):
        from PIL import Image
        for tid, name in enumerate(TEX_FILES[:self.L.mwb_num_textures(self.h)]):
            with Image.open(os.path.join(TEX_DIR, name + ".png")) as im:
                img = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
            _lib.check(self.L.mwb_set_texture(self.h, tid, img.shape[1], img.shape[0],
                                              img.ctypes.data_as(ctypes.c_void_p)))

    def _load_meshes(self, meshes):
        """ObjMesh.get for every mesh the task's entities use (objmesh.py:16-216) + the BVH the render kernel walks, and
        MeshEnt.__init__'s scale / radius (entity.py:118-127) evaluated here with the reference's expressions"""
        from . import meshes as M
        vp = ctypes.c_void_p
        done = set()
        for geom, height in meshes:
            name = geom + "_red" if geom in ("ball", "key") else geom   # the colour variants share their geometry
            m = M.get(name)
            if geom not in done:
                done.add(geom)
                octants = os.environ.get("MWB_BVH_OCTANTS", "1") != "0"   # 0: one threading for every ray direction (A/B timing)
                leaf = int(os.environ.get("MWB_BVH_LEAF", "8"))   # leaves of up to 8 triangles: 4 and 16 are 2-5 % slower, 2 and 1 10-35 %
                key = (name, octants, leaf)
                if key not in _BVH_CACHE:   # a second of NumPy per mesh: built once per process
                    _BVH_CACHE[key] = M.build_bvh(m.verts, leaf_size=leaf, octants=octants)
                nodes, perm = _BVH_CACHE[key]
                n_orders = 8 if octants else 1
                tex = TEX_FILES.index("../meshes/" + geom) if m.chunks[0][2] is not None else -1
                assert len(m.chunks) == 1, "one material per mesh"
                arrs = [np.ascontiguousarray(a, np.float32) for a in (m.verts, m.norms, m.texcs, m.min_coords, m.max_coords, nodes)]
                perm = np.ascontiguousarray(perm, np.int32)
                _lib.check(self.L.mwb_set_mesh(self.h, _lib.MESH_GEOMS.index(geom), m.n_tris, arrs[0].ctypes.data_as(vp), arrs[1].ctypes.data_as(vp),
                                               arrs[2].ctypes.data_as(vp), tex, arrs[3].ctypes.data_as(vp), arrs[4].ctypes.data_as(vp),
                                               nodes.shape[0] // n_orders, n_orders, arrs[5].ctypes.data_as(vp), perm.ctypes.data_as(vp)))
            scale, radius = M.mesh_ent_dims(name, height)
            _lib.check(self.L.mwb_set_mesh_dims(self.h, _lib.MESH_GEOMS.index(geom), float(height), float(scale), float(radius),
                                                int(isinstance(radius, np.float32))))

    # -------------------------------------------------------------------------------- lifecycle
    def close(self):
        if getattr(self, "h", None):
            self.torch.cuda.synchronize(self.device)
            self.L.mwb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------------------- simulation
    def seed(self, seed):
        """int -> env i gets seed + first_env_index + i (envs.py:36); or an explicit array of N seeds."""
        if np.isscalar(seed):
            seeds = (int(seed) + self.first_env_index + np.arange(self.num_envs, dtype=np.uint64)).astype(np.uint64)
        else:
            seeds = np.asarray(seed, dtype=np.uint64)
            assert seeds.shape == (self.num_envs,)
        seeds = np.ascontiguousarray(seeds)
        _lib.check(self.L.mwb_seed(self.h, seeds.ctypes.data_as(ctypes.c_void_p)))
        return [seed]

    def reset(self, mask=None):
        m = None
        if mask is not None:
            mask = mask.to(device=self.device, dtype=self.torch.uint8).contiguous()
            m = ctypes.c_void_p(mask.data_ptr())
        _lib.check(self.L.mwb_reset(self.h, m, self._stream()))
        if self.monitor is not None:   # the reset envs start a fresh episode
            self.monitor.clear(mask)
        return self.obs

    def step(self, actions, skip_mask=None):
        """actions: int tensor [N] (any int dtype / device); returns views (obs, reward, done) of the
        library-owned buffers, valid until the next call."""
        torch = self.torch
        a = torch.as_tensor(actions)
        i64 = a.dtype == torch.int64 and a.device == self.device   # the policy's LongTensor: read in place (mwb_step_i64)
        a = (a if i64 else a.to(device=self.device, dtype=torch.int32)).reshape(-1).contiguous()
        assert a.numel() == self.num_envs
        m = None
        if skip_mask is not None:
            skip_mask = torch.as_tensor(skip_mask).to(device=self.device, dtype=torch.uint8).contiguous()
            m = ctypes.c_void_p(skip_mask.data_ptr())
        _lib.check((self.L.mwb_step_i64 if i64 else self.L.mwb_step)(self.h, ctypes.c_void_p(a.data_ptr()), m, self._stream()))
        self._keep = (a, skip_mask)   # keep inputs alive until the async kernels have consumed them
        return self.obs, self.reward, self.done

    def step_repeat(self, actions, repeat, skip_mask=None, counts=None):
        """Action repeat on the device (mwb_step_repeat): every env takes up to `repeat` sub-steps of step() with its one action -
        counts[i] of them, clamped to 1 .. repeat on the device, when `counts` (int [N]) is given - stops at the sub-step that
        ends its episode, and only the frame after its last sub-step is rendered.  reward / reward64 are the sums over the
        sub-steps, done / ep_steps / feature / goal_pos the last sub-step's, `taken` the number of sub-steps.  int32 and int64
        actions on this device are read in place.  Returns the views (obs, reward, done, taken)."""
        torch = self.torch
        a = torch.as_tensor(actions)
        m = None if skip_mask is None else torch.as_tensor(skip_mask)
        c = None if counts is None else torch.as_tensor(counts)
        repeat = check_repeat_args(repeat, self.num_envs, a.numel(), None if m is None else m.numel(), None if c is None else c.numel())
        i64 = a.dtype == torch.int64 and a.device == self.device
        a = (a if i64 else a.to(device=self.device, dtype=torch.int32)).reshape(-1).contiguous()
        if m is not None:
            m = m.to(device=self.device, dtype=torch.uint8).reshape(-1).contiguous()
        if c is not None:
            c = c.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
        _lib.check(self.L.mwb_step_repeat(self.h, None if i64 else ptr(a), ptr(a) if i64 else None, ptr(m), repeat, ptr(c), self._stream()))
        self._keep = (a, m, c)   # keep inputs alive until the async kernels have consumed them
        return self.obs, self.reward, self.done, self.taken

    def step_longtensor(self, actions):
        """step() for the one shape a trainer's loop produces every time - a contiguous int64 tensor [N] on this device - without
        the generic conversions (the host time before the first kernel launch is on the critical path of a VecEnv step)"""
        rc = self.L.mwb_step_i64(self.h, actions.data_ptr(), None, self._stream())
        if rc:
            _lib.check(rc)
        self._keep = (actions, None)

    def render(self):
        _lib.check(self.L.mwb_render(self.h, self._stream()))
        return self.obs

    def visible_ents(self):
        """MiniWorldEnv.get_visible_ents() for every env (miniworld.py:1222-1315): int32 [N] on the device, bit b = box b
        (entity-list order) passes its occlusion query"""
        out = self.torch.empty((self.num_envs,), dtype=self.torch.int32, device=self.device)
        _lib.check(self.L.mwb_visible_ents(self.h, out.data_ptr(), self._stream()))
        return out

    def render_top_view(self, width=None, height=None):
        """MiniWorldEnv.render_top_view(frame_buffer) for every env (miniworld.py:1087-1158): uint8 [N, height, width, 3] on
        the device, default the observation size (the reference's default frame buffer is obs_fb).  Every task: the entity tasks'
        view draws the current entity list - box tops, the up-facing triangles of meshes, the frames' top strips."""
        W, H = int(width or self.W), int(height or self.H)
        out = self.torch.empty((self.num_envs, H, W, 3), dtype=self.torch.uint8, device=self.device)
        _lib.check(self.L.mwb_render_top_view(self.h, out.data_ptr(), W, H, self._stream()))
        return out

    def render_view(self, width, height, depth=False):
        """MiniWorldEnv.render_obs(frame_buffer) with another frame buffer than the observation's (miniworld.py:1160-1205), e.g.
        the 800 x 600 human view of render(mode='rgb_array'): uint8 [N, height, width, 3] (and float32 [N, height, width, 1]
        metres with depth=True) on the device, any size (rendered in tiles)"""
        W, H = int(width), int(height)
        out = self.torch.empty((self.num_envs, H, W, 3), dtype=self.torch.uint8, device=self.device)
        dep = self.torch.empty((self.num_envs, H, W, 1), dtype=self.torch.float32, device=self.device) if depth else None
        _lib.check(self.L.mwb_render_view(self.h, out.data_ptr(), dep.data_ptr() if depth else None, W, H, self._stream()))
        return (out, dep) if depth else out

    def grey_convert(self, rgb, layout="HWC"):
        """GreyscaleWrapper.observation + .float() (wrappers.py:38-45) for any uint8 RGB frames on this device, with the conversion the
        render kernels use (mwb_grey_convert): [n, H, W, 3] -> float32 [n, H, W, 1] (layout "HWC"), or [n, 3, W, H] -> [n, 1, W, H]
        ("CWH"); e.g. render_view()'s frames, or the observations of a batch whose frames are rendered in tiles"""
        torch = self.torch
        rgb = torch.as_tensor(rgb).to(device=self.device, dtype=torch.uint8).contiguous()
        if layout == "HWC":
            n, H, W, c = rgb.shape
            shape = (n, H, W, 1)
        else:
            n, c, W, H = rgb.shape
            shape = (n, 1, W, H)
        assert c == 3, "grey_convert: RGB frames"
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.check(self.L.mwb_grey_convert(self.h, rgb.data_ptr(), out.data_ptr(), int(n), int(W), int(H),
                                           {"HWC": _lib.LAYOUT_HWC, "CWH": _lib.LAYOUT_CWH}[layout], self._stream()))
        return out

    # ----------------------------------------------------------------- clone, snapshot, restore
    def _copy_index(self, idx):
        t = self.torch.as_tensor(idx)
        return t.to(device=self.device, dtype=self.torch.int32).reshape(-1).contiguous()

    def copy_envs(self, dst_idx, src_idx, src=None, render=True):
        """Env dst_idx[i] of this batch becomes a twin of env src_idx[i] of `src` (another BatchedMiniWorld of the same
        configuration, e.g. an archive(); None = this batch) without leaving the device (mwb_copy_envs): from then on the two
        agree bit for bit when stepped with the same actions.  Index lists that are tensors on this device are used in place
        (int32, contiguous; other dtypes are converted on the device) and validated on the device: a pair that breaks a rule is
        skipped and counted (copy_rejected()).  Host sequences / ndarrays are checked first by check_copy_indices, which raises
        ValueError before anything is launched.  render=True: the destinations' obs / depth / grey are rendered as render()
        renders them, nobody else's outputs change; render=False: only state moves, their frames are stale until rendered.
        Frame stack: see mwb_copy_envs (the window of a destination env becomes a copy of the source env's when both batches
        have the same stack; the source's must be current: stack_update() after its last pass).  Returns obs."""
        torch = self.torch
        src = self if src is None else src
        on_dev = [torch.is_tensor(i) and i.device == self.device for i in (dst_idx, src_idx)]
        if not all(on_dev):   # a list that lives on the host is checked on the host (a device list: by the validation kernel)
            to_host = lambda i: i.cpu().numpy() if torch.is_tensor(i) else i   # noqa: E731
            check_copy_indices(to_host(dst_idx), to_host(src_idx), self.num_envs, src.num_envs, src is self)
        d, s = self._copy_index(dst_idx), self._copy_index(src_idx)
        if d.numel() != s.numel():
            raise ValueError("copy_envs: dst_idx and src_idx differ in length")
        _lib.check(self.L.mwb_copy_envs(self.h, ctypes.c_void_p(d.data_ptr()), src.h, ctypes.c_void_p(s.data_ptr()), int(d.numel()),
                                        0 if render else _lib.COPY_NO_RENDER, self._stream()))
        self._keep_copy = (d, s, src)   # alive until the asynchronous kernels have consumed them
        if self.monitor is not None and d.numel():
            # the destinations are now in the middle of their sources' episodes, whose start this monitor did not see: dropped when
            # they end.  Every index the list names inside the batch is flagged, pairs the device-side validation rejected included
            # (one episode of such an env goes unlogged); an index outside the batch addresses nothing here
            ok = (d >= 0) & (d < self.num_envs)
            hit = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            hit.index_put_((d.clamp(0, self.num_envs - 1).long(),), ok.to(torch.int32), accumulate=True)
            self.monitor.clear(hit != 0, partial=True)
        return self.obs

    def copy_rejected(self):
        """pairs of copy_envs calls INTO this batch that the device-side validation rejected since the last call (synchronous)"""
        out = ctypes.c_ulonglong()
        _lib.check(self.L.mwb_copy_rejected(self.h, ctypes.byref(out)))
        return int(out.value)

    def archive(self, capacity):
        """A sibling batch of `capacity` slots with this batch's constructor arguments (and its frame stack, if one is enabled):
        unseeded, never reset or rendered, without textures or meshes - a place to save() env states to and restore() them from.  The
        archive of a batch with level sets has the same set (without tallies), so that save / restore keep an env's level index."""
        a = BatchedMiniWorld(num_envs=int(capacity), seed=None, _assets=False, **self._ctor)
        if self._stack_args is not None:
            a.stack_enable(**self._stack_args)
        if self.levels is not None:   # save / restore keep the level index (an archive never steps: it needs no tallies)
            a.levels_enable(**dict(self.levels.params(), tally=False))
        return a

    def save(self, archive, slots, envs):
        """envs of this batch -> slots of the archive (state only)"""
        archive.copy_envs(slots, envs, src=self, render=False)

    def restore(self, archive, slots, envs):
        """slots of the archive -> envs of this batch, rendered; returns obs"""
        return self.copy_envs(envs, slots, src=archive, render=True)

    # ---------------------------------------------------------------------------- introspection
    def check(self):
        """Synchronous: raises if world generation ever flagged a failure (see mwb_check)."""
        _lib.check(self.L.mwb_check(self.h))

    def _state_shape(self, shape):
        """the shape of a row of _lib.STATE_FIELDS after [count], for this batch's B"""
        return tuple({"B": self.n_boxes, "B+1": self.n_boxes + 1}.get(s, s) for s in shape)

    def get_state(self, first=0, count=None, rng_state=False):
        """Host snapshot of the env range (mwb_get_state).  Box fields come as "boxes_pos" [count, B, 3],
        "boxes_dir", "boxes_color", "boxes_size" and, for the one- and two-box tasks, also under the
        reference's attribute names: "box_*" = entity 0 (env.box / red_box), "box2_*" = entity 1."""
        self.check()
        count = self.num_envs - first if count is None else count
        # every field of the table; the general entity list (per slot kind / flags / dimensions, the list order, the task's
        # counters) for the entity tasks only, the 625 words per env of the generator on request
        arrays = {name: np.zeros((count,) + self._state_shape(shape), dt) for name, dt, shape, _, ent in _lib.STATE_FIELDS
                  if (self.ent_task or not ent) and (rng_state or name != "rng_state")}
        st = _lib.MwbState()
        for k, v in arrays.items():
            setattr(st, k, v.ctypes.data_as(ctypes.c_void_p))
        _lib.check(self.L.mwb_get_state(self.h, first, count, ctypes.byref(st)))
        out = {k: v for k, v in arrays.items() if not k.startswith("box_")}
        if self.ent_task:
            m = out["ent_meta"]
            out.update({"ent_kind": m & 15, "ent_geom": (m >> 4) & 15, "ent_static": (m >> 8) & 1, "ent_alive": (m >> 9) & 1,
                        "ent_rad_f32": (m >> 10) & 1, "ent_color": ((m >> 12) & 15) - 1})
        for k, v in arrays.items():
            if k.startswith("box_"):
                out["boxes_" + k[4:]] = v
                out[k] = v[:, 0]
                out["box2_" + k[4:]] = v[:, 1] if self.n_boxes > 1 else np.zeros_like(v[:, 0])
        return out

    def set_state(self, first, **fields):
        """Overwrite simulator state of envs first .. first+count-1 (mwb_set_state).  Keys as returned by
        get_state(): agent_pos [count,3], agent_dir, boxes_pos [count,B,3], boxes_dir, boxes_color, boxes_size,
        cam, sky_color, light_*, step_count, goal_idx, episode_count, task_step_count, goal_dist, carrying,
        rng_state [count,625]; for the entity tasks also ent_meta (the alive bit), ent_order, task_f, task_i."""
        writable = {name: (dt, shape) for name, dt, shape, w, _ in _lib.STATE_FIELDS if w}
        st = _lib.MwbState()
        keep, count = [], None
        for k, v in fields.items():
            name = "box_" + k[6:] if k.startswith("boxes_") else k
            if name not in writable:
                raise KeyError("set_state: %r is not a writable state field" % k)
            dt, shape = writable[name]
            a = np.ascontiguousarray(np.asarray(v, dtype=dt).reshape((-1,) + self._state_shape(shape)))
            if count is not None and a.shape[0] != count:
                raise ValueError("set_state: fields disagree on the number of envs")
            count = a.shape[0]
            keep.append(a)
            setattr(st, name, a.ctypes.data_as(ctypes.c_void_p))
        if count:
            _lib.check(self.L.mwb_set_state(self.h, int(first), int(count), ctypes.byref(st)))

    def set_agent(self, first, pos_xz=None, dir=None, step_count=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dt) for a, dt in
                ((pos_xz, np.float64), (dir, np.float64), (step_count, np.int32))]
        count = next(len(a) if a.ndim else 1 for a in arrs if a is not None)
        ptrs = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrs]
        _lib.check(self.L.mwb_set_agent(self.h, first, count, *ptrs))

    def set_domain_rand(self, flag):
        """`env.domain_rand = flag` of the reference (run_tests.py:64-66); effective from the next reset / step."""
        _lib.check(self.L.mwb_set_domain_rand(self.h, int(bool(flag))))
        self.domain_rand = bool(flag)

    def set_task_state(self, first, episode_count=None, task_step_count=None, goal_idx=None):
        """Overwrite the goal-alternation state of the T-maze family (test hook, mwb_set_task_state)."""
        arrs = [None if a is None else np.ascontiguousarray(np.atleast_1d(a), dt) for a, dt in
                ((episode_count, np.int64), (task_step_count, np.int64), (goal_idx, np.int32))]
        count = next(len(a) for a in arrs if a is not None)
        ptrs = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in arrs]
        _lib.check(self.L.mwb_set_task_state(self.h, first, count, *ptrs))

    def intersect(self, env, x, z, radius=0.4, ent=None):
        """MiniWorldEnv.intersect(ent, pos, radius) of env `env` (miniworld.py:933-959).  ent = index of the
        querying entity in the entity list (boxes first, the agent last; default: the agent), -1 = nobody is
        skipped.  Returns 0 none, 1 wall, 2 + k = entity k."""
        r = ctypes.c_int()
        ent = self.n_boxes if ent is None else int(ent)
        _lib.check(self.L.mwb_intersect(self.h, env, ent, float(x), float(z), float(radius), ctypes.byref(r)))
        return r.value

    def get_geometry(self, env, max_rooms=512, max_segs=2048):
        """(rooms [n_rooms, mwb_room_words] f32, segs [n_segs, 4] f64) of one env as the kernels see them: the rectangle
        room table, or for YMaze the polygon one (layouts: include/miniworld_batch.h at mwb_get_geometry)."""
        rooms = np.zeros((max_rooms, int(self.L.mwb_room_words(self.h))), np.float32)
        segs = np.zeros((max_segs, 4), np.float64)
        nr, ns = ctypes.c_int(), ctypes.c_int()
        _lib.check(self.L.mwb_get_geometry(self.h, env, rooms.ctypes.data_as(ctypes.c_void_p), max_rooms,
                                           segs.ctypes.data_as(ctypes.c_void_p), max_segs, ctypes.byref(nr),
                                           ctypes.byref(ns)))
        return rooms[:nr.value], segs[:ns.value]

    # ------------------------------------------------------------------------------ frame stack
    def stack_enable(self, nstack=4, dtype="float32", sliding=True, fused=False, grey=False):
        """Library-owned [N, nstack*3, W, H] stack kept by one fused HIP pass per step
        (VecPyTorchFrameStack + .float(), pytorch-a2c-ppo-acktr/envs.py:117-165). Needs layout='CWH'.
        sliding=True: the stack is a window that moves over a longer run of planes per env, so a step writes the new frame only
        (1/4 of the shifting stack's HBM traffic); stack_update() then returns a strided view [N, nstack*3, W, H] of it (same
        values; a different view object every step).  sliding=False: the shifting stack in one fixed contiguous tensor.
        fused=True (implies sliding): reset() / step() write each new frame into the window themselves, straight from the render
        kernel's LDS frame, and zero the history of the envs they regenerate - stack_update() then only returns the view.
        grey=True (needs greyscale=True at construction and float32): the stack of the grey frames, [N, nstack, W, H] - one plane
        per frame (MWB_STACK_GREY); every form above."""
        torch = self.torch
        is_f = {"float32": 1, "uint8": 0}[dtype]
        sliding = sliding or fused
        if self.terminal is not None:
            raise ValueError("stack_enable: after terminal_enable (which lays its rows out for the stack it finds); a batch with "
                             "terminal observations takes stack_enable(fused=True) before terminal_enable")
        _lib.check(self.L.mwb_stack_enable(self.h, int(nstack), is_f | (_lib.STACK_SLIDING if sliding else 0) | (_lib.STACK_FUSED if fused else 0) |
                                           (_lib.STACK_GREY if grey else 0)))
        out = _lib.MwbOutputs()
        _lib.check(self.L.mwb_get_outputs(self.h, ctypes.byref(out)))
        first, planes = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.L.mwb_stack_window(self.h, ctypes.byref(first), ctypes.byref(planes)))
        self._stack_args = dict(nstack=nstack, dtype=dtype, sliding=sliding, fused=fused, grey=grey)
        self._stack_c, self._stack_sliding = nstack * (1 if grey else 3), bool(sliding)
        shape = (self.num_envs, planes.value, self.W, self.H)
        self._stack_base = _dev_tensor(self, out.stack, shape, "<f4" if is_f else "|u1")
        self.stack = self._stack_base[:, first.value:first.value + self._stack_c]
        return self.stack

    def stack_update(self, after_reset=False):
        _lib.check(self.L.mwb_stack_update(self.h, int(bool(after_reset)), self._stream()))
        if self._stack_sliding:
            first = ctypes.c_int32()
            _lib.check(self.L.mwb_stack_window(self.h, ctypes.byref(first), None))
            self.stack = self._stack_base[:, first.value:first.value + self._stack_c]
        return self.stack

    # --------------------------------------------------------------------------- rollout storage
    def rollout_enable(self, num_steps, nstack=4, grey=False, learner=False):
        """The observation half of the trainer's RolloutStorage on the device (mwb_rollout_enable): a ring of num_steps + nstack
        single frames - uint8 RGB, or with grey=True (needs greyscale=True at construction) the float32 grey frames - instead of
        num_steps + 1 stacked float32 observations, and the rewards / masks / features rows.  Needs layout='CWH'.  Returns the
        Rollout (also self.rollout): push() after every reset() / step(), gather(idx) for the minibatches.  learner=True: the
        learner half as well (Rollout.learner_enable): actions, log-probs, value predictions, `taken`, the returns / GAE scan and
        the minibatch tuples."""
        self.rollout = Rollout(self, num_steps, nstack, grey, learner=learner)
        return self.rollout

    def monitor_enable(self, capacity=100, quota_max=0):
        """The episode monitor on the device (mwb_monitor_enable): returns, lengths, the log of the last `capacity` episodes - the
        trainer's deque(maxlen=100) and its loop over the envs after every step (pytorch-a2c-ppo-acktr/main.py:141,167-169) - and
        per-env evaluation quotas up to quota_max.  Returns the Monitor (also self.monitor); from now on reset() / reset(mask)
        clear the reset envs' running episodes and copy_envs() marks its destinations as partial.  Call monitor.update() after
        every step."""
        if self.monitor is not None:
            _lib.check(self.L.mwb_monitor_enable(self.h, int(capacity), int(quota_max)))   # raises the library's MWB_ESTATE message
        mon = Monitor(self, capacity, quota_max)
        self.monitor = mon
        return mon

    def terminal_enable(self, capacity=None, dtype=None):
        """Terminal observations and the cause of every episode's end (mwb_terminal_enable): from now on step() / step_repeat()
        render the frame of every env that ends BEFORE regenerating it and report why it ended.  capacity (None: num_envs): the
        stacked rows kept per step; dtype ("uint8" / "float32"): of the rows of a batch without a frame stack (a stacked batch's
        rows take the stack's).  Call before the first reset(), after stack_enable(fused=True) where a stack is used; a
        non-fused stack is refused.  Returns the Terminal (also self.terminal)."""
        if getattr(self, "terminal", None) is not None:
            raise ValueError("terminal_enable: already enabled")
        self.terminal = Terminal(self, capacity, dtype)
        return self.terminal

    def levels_enable(self, num_levels, start_level=0, seeds=None, mode="uniform", sampler_seed=0, tally=True, env_stride=None):
        """Level sets (mwb_levels_enable; Procgen's num_levels / start_level): from now on every regeneration of an env starts
        from the generator stream of a level seed chosen on the device - seeds[i] where a table of num_levels seeds is given,
        start_level + i otherwise.  mode: "sequential" (env g plays (g + n * env_stride) mod num_levels in its n-th episode),
        "uniform" (a hash of sampler_seed, g and n) or "table" (levels.next_level, uniform where it holds none); g =
        first_env_index + e, env_stride defaults to num_envs.  tally: per-level episode / step / success counts (num_levels <=
        2^22).  The batch needs no seed() afterwards.  Once per batch; returns the Levels (also self.levels)."""
        if getattr(self, "levels", None) is not None:
            raise ValueError("levels_enable: already enabled")
        args = check_levels_args(num_levels, start_level, seeds, mode, sampler_seed, tally, env_stride, self.num_envs)
        self.levels = Levels(self, args, self.first_env_index)
        return self.levels

    def frame_reuse_stats(self):
        """(frames reused, frames rendered) by the step passes since the last call (mwb_frame_reuse_stats; synchronous).  A step
        that leaves an env as it was - a move a wall blocks - copies the env's last frame from a private cache instead of
        rendering it; MWB_NO_FRAME_REUSE=1 in the environment when the batch is created turns that off."""
        out = (ctypes.c_ulonglong * 2)()
        _lib.check(self.L.mwb_frame_reuse_stats(self.h, out))
        return int(out[0]), int(out[1])

    def bulk_variant(self):
        """1 if the bulk render launch of step() runs the kernel compiled for 80 x 60 frames (render_fixed_kernel), 0 if the
        generic one (mwb_bulk_variant): the same frames either way.  MWB_NO_FIXED=1 in the environment when the batch is
        created keeps the generic kernel."""
        return int(self.L.mwb_bulk_variant(self.h))

    def timing_enable(self, on=True):
        """on: False / True, or an int n > 1 to time every n-th pass only (the events cost ~20 us per pass)."""
        _lib.check(self.L.mwb_timing_enable(self.h, int(on)))

    def timing_read(self):
        v = [ctypes.c_double() for _ in range(4)]
        n = ctypes.c_int()
        _lib.check(self.L.mwb_timing_read(self.h, *[ctypes.byref(x) for x in v], ctypes.byref(n)))
        return {"step": v[0].value, "reset": v[1].value, "prep": v[2].value, "render": v[3].value, "n": n.value}
