"""GPU: observation sizes at the render kernel's own limits, derived from the code instead of listed by habit.

* The 16-bit pixel queue (mwb_lds_layout.h: a queued pixel is (py << bits(W)) | px, the bits left over carry the count of shared
  portal crossings): sizes with 14, 15 and 16 coordinate bits, one past a power of two, and H << bits(W) == 65536 both ways.
* The 160 KB LDS bound that switches a handle to 75 x 60 tiles: per task, at W = 256, the last frame one workgroup renders whole
  and the first one rendered in tiles, computed with the host build of mwb_lds_layout.h (tests/lds_host.py) and confirmed on the
  handle.
* Tile remainders: 76 x 61 and 151 x 121 leave a one-pixel column, a one-pixel row and a 1 x 1 corner tile.
* The smallest frames, from 1 x 1: accepted and right, or refused with MWB_EINVAL - never accepted and wrong.

Four tasks (one box, six boxes, polygon rooms, entities), 4 envs, domain randomisation on, both layouts.  For every accepted size:
reset and 3 random steps; obs +-1 LSB and depth 1e-4 m against the oracle; the interior-pixel fast path equal to the full-sample
path bit for bit (MWB_DEBUG=9, MWB_DEBUG=1); render_view at the observation's size equal to obs / depth bit for bit wherever the
observation itself is not tiled."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from lds_host import LDS_LIMIT, build_lds_host, frame_words

pytestmark = pytest.mark.gpu

N_ENVS, SEED, STEPS = 4, 640, 3
# env id -> (oracle task, task_args, actions, render_lds arguments of the handle: R_max, room words, frame words, textures, entity task)
TASKS = {
    "MiniWorld-Hallway-v0": ("Hallway", None, 3, (1, 24, frame_words(1), 7, 0)),
    "MiniWorld-PutNext-v0": ("PutNext", None, 8, (1, 24, frame_words(6), 7, 0)),
    "MiniWorld-YMaze-v0": ("YMaze", [0, 0, 0, 0], 3, (6, 52, frame_words(1), 7, 0)),
    "MiniWorld-WallGap-v0": ("WallGap", None, 3, (8, 24, frame_words(20), 25, 1)),   # the entity kernels are laid out for every slot
}
QUEUE_SIZES = [(128, 128),    # both exact powers of two: 7 + 7 = 14 bits
               (129, 128),    # one past a power of two: 8 + 7 = 15 bits
               (256, 128),    # 8 + 7 = 15 bits
               (256, 192),    # 8 + 8 = 16 bits: no spare bit for the shared-crossing count
               (1024, 64),    # H << 10 == 65536: the queue's limit itself (LDS forces tiles)
               (64, 1024)]    # the same limit the other way
LDS_SIZES = ["lds-last-whole", "lds-first-tiled"]   # (256, H) and (256, H + 1), H per task: lds_boundary()
SMALL_SIZES = [(1, 1), (2, 2), (4, 1), (1, 16), (16, 1)]
EINVAL = r"error -1: "   # MWB_EINVAL as _lib.check reports it


def whole_frame(env_id, W, H):
    """mwb_create's rule: one workgroup renders the frame whole when its launch fits 160 KB of LDS and its pixels the 16-bit queue"""
    L = build_lds_host()
    return L.lds_launch_bytes(*TASKS[env_id][3], W, H, 0, 0) <= LDS_LIMIT and bool(L.lds_pixel_queue_fits(W, H))


def lds_boundary(env_id):
    """the largest H at W = 256 that is still rendered whole"""
    hs = [h for h in range(1, 257) if whole_frame(env_id, 256, h)]
    assert hs and max(hs) < 256 and hs == list(range(1, max(hs) + 1)), (env_id, "the LDS bound is not what ends the range")
    return max(hs)


def resolve(env_id, size):
    if size == "lds-last-whole":
        return 256, lds_boundary(env_id)
    if size == "lds-first-tiled":
        return 256, lds_boundary(env_id) + 1
    return size


def make(env_id, W, H, layout, n=N_ENVS):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    return BatchedMiniWorld(env_id, num_envs=n, seed=SEED, domain_rand=True, obs_width=W, obs_height=H, layout=layout, want_depth=True)


def action_list(env_id):
    rng = np.random.default_rng(8)
    return [rng.integers(0, TASKS[env_id][2], size=N_ENVS).astype(np.int32) for _ in range(STEPS)]


_ORACLE = {}


def oracle_frames(O, env_id, W, H):
    """the oracle's rollout of the case, once per (task, size) - both layouts and the view tests share it: {"reset" / "end":
    (rgb [n, H, W, 3], depth [n, H, W]), "done": [steps, n]}.  The envs render in threads (the oracle's globals are read-only)."""
    key = (env_id, W, H)
    if key in _ORACLE:
        return _ORACLE[key]
    task, args, _, _ = TASKS[env_id]
    envs = [O.OracleEnv(task, seed=SEED + i, domain_rand=True, task_args=args, obs_width=W, obs_height=H) for i in range(N_ENVS)]
    ent = O.TASKS[task] >= 10
    out = {}
    with ThreadPoolExecutor(N_ENVS) as pool:
        def frames(step_frame):
            got = list(pool.map(lambda ef: ef[0].render_obs(depth=True, step_frame=ef[1]), zip(envs, step_frame)))
            return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
        for e in envs:
            e.reset(render=False)
        out["reset"] = frames([False] * N_ENVS)
        dones = []
        for a in action_list(env_id):
            done = [e.step(int(a[i]))[2] for i, e in enumerate(envs)]
            dones.append(done)
            for e, dn in zip(envs, done):
                if dn:
                    e.reset(render=False)
        out["end"] = frames([ent and not dn for dn in dones[-1]])   # an entity task's step frame shows the entities as the step saw them
    out["done"] = np.array(dones, dtype=bool)
    _ORACLE[key] = out
    return out


def hwc(b):
    obs = b.obs.cpu().numpy()
    return obs.transpose(0, 3, 2, 1) if b.layout == "CWH" else obs   # [N, 3, W, H] -> [N, H, W, 3]


def assert_close_to_oracle(rgb, dep, ref, tag):
    ref_rgb, ref_dep = ref
    assert rgb.shape == ref_rgb.shape and dep.shape == ref_dep.shape, (tag, rgb.shape, ref_rgb.shape)
    for i in range(len(rgb)):
        d = np.abs(rgb[i].astype(np.int16) - ref_rgb[i].astype(np.int16))
        assert d.max() <= 1, (tag, i, int(d.max()), int((d > 1).sum()))
        dd = float(np.abs(dep[i] - ref_dep[i]).max())
        assert dd <= 1e-4, (tag, i, "depth", dd)


def run_case(O, env_id, W, H, layout, monkeypatch, tiled):
    """three handles - as built, MWB_DEBUG=9 (every pixel by the full 8-sample path, each traversal from the eye's room), MWB_DEBUG=1
    (full path, shared crossings skipped) - through reset and STEPS steps"""
    import torch
    fast = make(env_id, W, H, layout)
    monkeypatch.setenv("MWB_DEBUG", "9")
    full = make(env_id, W, H, layout)
    monkeypatch.setenv("MWB_DEBUG", "1")
    full_skip = make(env_id, W, H, layout)
    monkeypatch.delenv("MWB_DEBUG")
    ref = oracle_frames(O, env_id, W, H)
    tag = (env_id, W, H, layout)

    def check(when):
        assert torch.equal(fast.obs, full.obs) and torch.equal(fast.depth, full.depth), (tag, when, "the fast path changed a frame")
        assert torch.equal(full_skip.obs, full.obs) and torch.equal(full_skip.depth, full.depth), (tag, when, "prefix skipping changed a frame")
        assert tuple(fast.depth.shape) == (N_ENVS, H, W, 1)
        assert_close_to_oracle(hwc(fast), fast.depth.cpu().numpy()[..., 0], ref[when], tag + (when,))
        if not tiled:   # the same frame through mwb_render_view's tiles
            view, vdep = fast.render_view(W, H, depth=True)
            assert np.array_equal(view.cpu().numpy(), hwc(fast)) and torch.equal(vdep, fast.depth), (tag, when, "render_view differs from obs")

    for h in (fast, full, full_skip):
        h.reset()
    check("reset")
    for t, a in enumerate(action_list(env_id)):
        for h in (fast, full, full_skip):
            h.step(torch.from_numpy(a))
        assert np.array_equal(fast.done.cpu().numpy().astype(bool), ref["done"][t]), (tag, t)
        assert torch.equal(fast.obs, full.obs) and torch.equal(fast.depth, full.depth), (tag, t, "the fast path changed a frame")
        assert torch.equal(fast.reward64, full.reward64) and torch.equal(fast.reward64, full_skip.reward64), (tag, t)
    check("end")
    for h in (fast, full, full_skip):
        h.check()
        h.close()


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
@pytest.mark.parametrize("size", QUEUE_SIZES + LDS_SIZES, ids=lambda s: s if isinstance(s, str) else "%dx%d" % s)
@pytest.mark.parametrize("env_id", list(TASKS))
def test_sizes_at_the_queue_and_lds_limits(oracle_mod, env_id, size, layout, monkeypatch):
    W, H = resolve(env_id, size)
    tiled = not whole_frame(env_id, W, H)
    if size == "lds-last-whole":
        assert not tiled and not whole_frame(env_id, W, H + 1)
    if size in ("lds-first-tiled", (1024, 64), (64, 1024)):
        assert tiled
    run_case(oracle_mod, env_id, W, H, layout, monkeypatch, tiled)


@pytest.mark.parametrize("env_id", list(TASKS))
def test_the_handle_switches_to_tiles_where_the_layout_says(env_id):
    """mwb_grey_enable refuses a handle whose observations are rendered in tiles: the last whole frame takes it, the first tiled
    one does not - the boundary computed on the host is the one mwb_create applies"""
    from gym_miniworld_amd._lib import MwbError
    from gym_miniworld_amd.batch import BatchedMiniWorld
    H = lds_boundary(env_id)
    kw = dict(num_envs=1, seed=SEED, obs_width=256, greyscale=True)
    BatchedMiniWorld(env_id, obs_height=H, **kw).close()
    with pytest.raises(MwbError, match=EINVAL + ".*rendered in tiles"):
        BatchedMiniWorld(env_id, obs_height=H + 1, **kw)


@pytest.mark.parametrize("size", [(76, 61), (151, 121)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("env_id", list(TASKS))
def test_view_tiles_with_one_pixel_remainders(oracle_mod, env_id, size):
    """mwb_render_view's 75 x 60 tiles over 76 x 61 and 151 x 121: the last column of tiles is one pixel wide, the last row one
    pixel high, the corner tile a single pixel - after the reset and after the steps, from a handle of the default size"""
    import torch
    W, H = size
    ref = oracle_frames(oracle_mod, env_id, W, H)
    b = make(env_id, 80, 60, "HWC")
    b.reset()
    img, dep = b.render_view(W, H, depth=True)
    assert_close_to_oracle(img.cpu().numpy(), dep.cpu().numpy()[..., 0], ref["reset"], (env_id, W, H, "reset"))
    for a in action_list(env_id):
        b.step(torch.from_numpy(a))
    # the view shows the current state, which is what the step's own frame showed: these steps end no episode and remove no entity
    assert not ref["done"].any() and not b.done.any()
    img, dep = b.render_view(W, H, depth=True)
    assert_close_to_oracle(img.cpu().numpy(), dep.cpu().numpy()[..., 0], ref["end"], (env_id, W, H, "end"))
    b.close()


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
def test_entity_observations_in_tiles_with_one_pixel_remainders(oracle_mod, layout, monkeypatch):
    """MWB_TILE=75x60 at 76 x 61: the entity tasks' tiled observations (reset and step) with the same remainders"""
    monkeypatch.setenv("MWB_TILE", "75x60")
    run_case(oracle_mod, "MiniWorld-WallGap-v0", 76, 61, layout, monkeypatch, tiled=True)


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("env_id", list(TASKS))
def test_smallest_frames_are_right_or_refused(oracle_mod, env_id, size, layout, monkeypatch):
    """accepted: the frame meets the oracle's bars like any other; refused: MwbError with MWB_EINVAL from the constructor, and the
    process goes on working.  Accepted and wrong is the failure."""
    from gym_miniworld_amd._lib import MwbError
    W, H = size
    try:
        make(env_id, W, H, layout).close()
    except MwbError as err:
        assert EINVAL.strip() in str(err) and "mwb_create" in str(err), str(err)
        b = make(env_id, 80, 60, layout)   # the process stays usable
        b.reset()
        assert 0 < float(b.obs.float().mean()) < 255
        b.close()
        return
    run_case(oracle_mod, env_id, W, H, layout, monkeypatch, tiled=False)
