"""GPU: what happens at episode boundaries, at the batch sizes and frame shapes where that code branches.

1. Mass time-outs: envs started together time out together, so the regenerated-env list holds (nearly) the whole batch and
   reset_kernel (1024 blocks) and the side stream's render_kernel (1280 blocks) go round their grid-stride loops a second time,
   reusing their LDS - against per-env oracles: rewards / dones / step counts exact at every step, the state bit for bit,
   frames +-1 LSB, depth 1e-4 m.
2. The fused frame stack of that batch (whole-frame AND half-frame writers, history zeroing, the wrap copy on a time-out step)
   against the restatement of VecPyTorchFrameStack (tests/stack_ref.py): exact.
3. Every frame-stack implementation - shifting, sliding, fused - at the nstack / dtype / frame sizes where it takes another
   path, also with a skip mask: exact against the same restatement; the documented refusals of mwb_stack_enable.
4. mwb_reset(mask), the partial reset: masked envs equal the oracle's reset, the others do not change by a bit, nothing is
   regenerated a second time afterwards; its documented rule for the fused stack.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------ 1. mass time-out
N_MASS, MES_MASS, SEED_MASS, STEPS_MASS = 1536, 3, 500, 7   # 1536: the smallest round size above both list grids (1024, 1280)
LIST_GRID = 1280                                            # the larger of the two grids: more dones than this = a second trip
TIMEOUT_STEPS = (3, 6)

# env id -> (oracle task, task_args, domain_rand, layout, depth)
MASS_CASES = {
    "MiniWorld-MazeS3-v0": ("Maze", [3, 3, 3], 0, "HWC", True),
    "MiniWorld-Hallway-v0": ("Hallway", None, 1, "CWH", False),
    # Sign(MiniWorldEnv) switches domain randomisation off itself (sign.py:62-71) - the handle does the same with the flag it
    # is given, and the oracle gets the flag the handle ended up with; only actions 0..2 (3 = pickup ends Sign's episode)
    "MiniWorld-Sign-v0": ("Sign", [10, 0, 0, 0], 1, "HWC", False),
    "MiniWorld-PickupObjs-v0": ("PickupObjs", [12, 5, 0, 0], 1, "HWC", False),
}


def mass_actions():
    rng = np.random.default_rng(0)
    while True:
        yield rng.integers(0, 3, size=N_MASS).astype(np.int32)


def make_mass_pair(O, env_id, n=N_MASS, **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld, ENV_SPECS
    task, args, dr, layout, depth = MASS_CASES[env_id]
    b = BatchedMiniWorld(env_id, num_envs=n, seed=SEED_MASS, domain_rand=dr, want_depth=depth, layout=layout, max_episode_steps=MES_MASS, **kw)
    prm = ENV_SPECS[env_id][3]
    table = prm().to_table() if prm else None
    envs = [O.OracleEnv(task, seed=SEED_MASS + i, domain_rand=b.domain_rand, task_args=args, max_episode_steps=MES_MASS, params=table)
            for i in range(n)]
    return b, envs


def oracle_step_all(envs, a):
    """one VecEnv step of the per-env oracles (subproc_vec_env.py:9-14: a finished env is reset in the step): reward, done, step
    count at the end of the step (before the reset)"""
    n = len(envs)
    rew, done, sc = np.zeros(n), np.zeros(n, bool), np.zeros(n, np.int32)
    for i, e in enumerate(envs):
        _, rew[i], done[i], _ = e.step(int(a[i]))
        sc[i] = e.state().step_count
        if done[i]:
            e.reset(render=False)
    return rew, done, sc


def assert_step_outputs(b, rew, done, sc, tag):
    got = (b.reward64.cpu().numpy(), b.done.cpu().numpy().astype(bool), b.ep_steps.cpu().numpy())
    for name, g, want in zip(("reward64", "done", "ep_steps"), got, (rew, done, sc)):
        bad = np.nonzero(g != want)[0]
        assert bad.size == 0, (tag, name, "envs", bad[:8].tolist(), len(bad), g[bad[:4]].tolist(), want[bad[:4]].tolist())


def assert_full_state(b, envs, tag):
    if b.ent_task:
        from test_gpu_ents import assert_state_equal
        assert_state_equal(b, b.get_state(), envs, tag)
    else:
        from test_gpu_parity import assert_state_equal
        assert_state_equal(b.get_state(), [e.state() for e in envs], tag=tag)


def assert_frames(b, envs, idx, done, tag):
    """the step's own frames of the envs `idx` against the oracle: +-1 LSB, depth 1e-4 m.  An env that ended shows the first
    frame of its new episode, any other the frame its step saw (entity tasks: step_frame)"""
    obs = b.obs.cpu().numpy()
    if b.layout == "CWH":
        obs = obs.transpose(0, 3, 2, 1)   # [N, 3, W, H] -> [N, H, W, 3]
    dep = b.depth.cpu().numpy()[..., 0] if b.want_depth else None
    for i in idx:
        i = int(i)
        sf = bool(b.ent_task and done is not None and not done[i])
        if dep is not None:
            ref, refd = envs[i].render_obs(depth=True, step_frame=sf)
            dd = float(np.abs(dep[i] - refd).max())
            assert dd <= 1e-4, (tag, i, "depth", dd)
        else:
            ref = envs[i].render_obs(step_frame=sf)
        d = np.abs(obs[i].astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1, (tag, i, int(d.max()), int((d > 1).sum()))


@pytest.mark.parametrize("env_id", list(MASS_CASES))
def test_mass_timeout_matches_oracle(oracle_mod, env_id):
    """1536 envs with max_episode_steps = 3: (nearly) all of them end in steps 3 and 6 - the second trip round the list loops of
    reset_kernel and of the side stream's render_kernel - and come back as the oracle's envs do."""
    import torch
    b, envs = make_mass_pair(oracle_mod, env_id)
    n = N_MASS
    cheap = "PickupObjs" not in env_id   # the oracle renders a frame of the box tasks / Sign in milliseconds, one of PickupObjs in 0.4 s
    sample24 = np.linspace(0, n - 1, 24).round().astype(int)
    sample16 = np.linspace(0, n - 1, 16).round().astype(int)   # incl. 0 and N - 1
    b.reset()
    for e in envs:
        e.reset(render=False)
    acts = mass_actions()
    dones_per_step = []
    for t in range(1, STEPS_MASS + 1):
        a = next(acts)
        b.obs.zero_()
        b.step(torch.from_numpy(a))
        tag = "%s step %d" % (env_id, t)
        rew, done, sc = oracle_step_all(envs, a)
        dones_per_step.append(int(done.sum()))
        assert_step_outputs(b, rew, done, sc, tag)
        if t in TIMEOUT_STEPS:   # the path this test is about was taken: more regenerated envs than either list grid has blocks
            assert int(b.done.sum()) > LIST_GRID, (tag, int(b.done.sum()))
        blank = (b.obs.reshape(n, -1).max(dim=1).values == 0).nonzero().flatten().tolist()
        assert not blank, (tag, "envs that were not rendered", blank[:8], len(blank))
        if t == 3:
            assert_full_state(b, envs, tag)
            assert_frames(b, envs, range(n) if cheap else sample16, done, tag)
        elif t == 6:
            assert_frames(b, envs, sample24 if cheap else sample16, done, tag)
        elif t == 7:
            assert_full_state(b, envs, tag)
            if cheap:
                assert_frames(b, envs, sample24, done, tag)
        if t in TIMEOUT_STEPS:   # a plain render of the same state reproduces the time-out step's frames (actions 0..2: no rule removes an entity)
            step_obs = b.obs.clone()
            step_dep = b.depth.clone() if b.want_depth else None
            b.render()
            diff = (step_obs != b.obs).reshape(n, -1).any(dim=1).nonzero().flatten().tolist()
            assert not diff, (tag, "render() differs from the step's frame in envs", diff[:8], len(diff))
            assert step_dep is None or torch.equal(step_dep, b.depth)
    assert dones_per_step[2] > LIST_GRID and dones_per_step[5] > LIST_GRID, dones_per_step   # ... and by the oracle alone
    b.check()
    b.close()


def test_mass_timeout_single_stream_equals_overlapped(monkeypatch):
    """MWB_NO_OVERLAP=1 (read at mwb_create): regeneration and render on the caller's stream, one launch after the other - the
    same observations, rewards and dones as the forked path, bit for bit, through two mass time-outs."""
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    kw = dict(num_envs=N_MASS, seed=SEED_MASS, want_depth=True, max_episode_steps=MES_MASS)
    forked = BatchedMiniWorld("MiniWorld-MazeS3-v0", **kw)
    monkeypatch.setenv("MWB_NO_OVERLAP", "1")
    single = BatchedMiniWorld("MiniWorld-MazeS3-v0", **kw)
    monkeypatch.delenv("MWB_NO_OVERLAP")
    assert torch.equal(forked.reset(), single.reset()) and torch.equal(forked.depth, single.depth)
    acts = mass_actions()
    for t in range(1, STEPS_MASS + 1):
        a = torch.from_numpy(next(acts))
        forked.step(a); single.step(a)
        assert torch.equal(forked.done, single.done) and torch.equal(forked.reward64, single.reward64), t
        assert torch.equal(forked.ep_steps, single.ep_steps), t
        diff = (forked.obs != single.obs).reshape(N_MASS, -1).any(dim=1).nonzero().flatten().tolist()
        assert not diff, (t, "envs with differing frames", diff[:8], len(diff))
        assert torch.equal(forked.depth, single.depth), t
        if t in TIMEOUT_STEPS:
            assert int(single.done.sum()) > LIST_GRID, (t, int(single.done.sum()))
    forked.close(); single.close()


# --------------------------------------------------------------------------- 2. the fused stack of the large batch
def stack_window(b):
    """(first plane of the current window, planes per env): mwb_stack_window"""
    from gym_miniworld_amd import _lib
    first, planes = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(b.L.mwb_stack_window(b.h, ctypes.byref(first), ctypes.byref(planes)))
    return first.value, planes.value


@pytest.mark.parametrize("to_float", [True, False])
def test_fused_stack_through_mass_timeouts_and_wraps(to_float):
    """make_vec_envs' stack at 1536 envs (768 whole-frame + 768 half-frame writers in the bulk pass, whole-frame writers walking
    the list on the side stream) with a time-out every 3 steps and a wrap of the window every 9: exact against the restatement
    every step, compared on the device."""
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    from stack_ref import FrameStackRef
    n, nstack = N_MASS, 4
    kw = dict(seed=SEED_MASS, to_float=to_float, max_episode_steps=MES_MASS)
    v = MiniWorldVecEnv("MiniWorld-MazeS3-v0", n, frame_stack=nstack, **kw)
    plain = MiniWorldVecEnv("MiniWorld-MazeS3-v0", n, frame_stack=0, **kw)
    assert v.batch.num_envs > 768   # split_envs = min(768, N): both whole-frame and half-frame workgroups in the bulk pass
    dtype = torch.float32 if to_float else torch.uint8
    ref = FrameStackRef(n, nstack, (3, 80, 60), dtype=dtype, device=v.device)
    st = v.reset()
    assert st.dtype == dtype and tuple(st.shape) == (n, 12, 80, 60)
    assert torch.equal(st, ref.reset(plain.reset()))
    assert stack_window(v.batch) == (0, 12 + 3 * _lib.STACK_SLACK_FRAMES)
    acts = mass_actions()
    wrap_with_mass_timeout = []
    pos = 0
    for t in range(1, 31):
        a = torch.from_numpy(next(acts).astype(np.int64)).unsqueeze(1)
        st, _, done, _ = v.step(a)
        ob, _, done2, _ = plain.step(a)
        assert np.array_equal(done, done2), t
        want = ref.step(ob, done)
        if not torch.equal(st, want):
            bad = (st != want).reshape(n, -1).any(dim=1).nonzero().flatten().tolist()
            raise AssertionError((t, "envs whose stack differs", bad[:8], len(bad), "of them done", int(done[bad].sum())))
        prev, pos = pos, stack_window(v.batch)[0]
        assert pos == prev + 3 or pos == 0, (t, prev, pos)
        if pos == 0 and done.sum() > LIST_GRID:   # the window came back to plane 0 in a step (no full reset happens in this loop)
            wrap_with_mass_timeout.append((t, int(done.sum())))
    assert wrap_with_mass_timeout, "no step had the wrap copy and a mass time-out together"
    v.close(); plain.close()


# ------------------------------------------------------------- 3. every stack implementation where it branches
# Frame sizes (W, H).  The fused writer of a half-frame workgroup (every env of a batch <= 768) writes the columns [0, midx) or
# [midx, W) of each channel plane, midx = half_strips * (TILE_CX - 1) = ((W + 14) / 15 + 1) / 2 * 15: byte range
# [(q W + xa) H, (q W + xb) H) of the LDS frame.
SIZE_DEFAULT = (80, 60)    # midx * H = 45 * 60: every range a multiple of 16 -> float4 / uint4 paths
# midx * H % 4 != 0 -> the scalar branch of the float writer.  34 x 18 cannot get there: n_strips = 3, midx = 30, 30 * 18 = 540
# is a multiple of 4 (and with W = 34 no H can do it: midx * H needs an odd H, W * H % 4 == 0 an even one).  The nearest size
# that does: 30 x 18 - n_strips = 2, midx = 15, 15 * 18 = 270 = 2 (mod 4), W * H = 540 = 0 (mod 4).  540 % 16 != 0, so a fused
# uint8 stack is refused at this size.
SIZE_F32_SCALAR = (30, 18)
# W * H % 16 == 0 (fused uint8 allowed), odd H, midx = 30, 30 * 15 = 450 = 2 (mod 4): copy_frame_range's byte path for uint8
# and again the scalar branch for float
SIZE_U8_UNALIGNED = (48, 15)
# test_gpu_view.py's tile test: 320 x 240 x 3 bytes do not fit one workgroup's LDS (mwb_create: mwb_render_lds_bytes > 160 KB),
# the observation is rendered in tiles -> MWB_STACK_FUSED is refused, the sliding window is what a front-end falls back to
SIZE_TILED = (320, 240)

FORMS = {"shifting": dict(sliding=False, fused=False), "sliding": dict(sliding=True, fused=False), "fused": dict(sliding=True, fused=True)}
# (dtype, nstack, size, the fused form is refused): with every form each dtype, each nstack and each size at least once
SHAPES = [
    ("float32", 1, SIZE_F32_SCALAR, False),    # C - 3 = 0: no history at all; float scalar branch
    ("uint8", 2, SIZE_U8_UNALIGNED, False),    # uint8 byte path
    ("float32", 5, SIZE_DEFAULT, False),       # not the 4 every other test uses
    ("uint8", 1, SIZE_DEFAULT, False),
    ("float32", 2, SIZE_U8_UNALIGNED, False),  # float scalar branch, odd H
    ("uint8", 5, SIZE_F32_SCALAR, True),       # fused uint8 needs W * H % 16 == 0
    ("float32", 2, SIZE_TILED, True),          # fused needs whole-frame workgroups
]
EINVAL = r"error -1: "   # MWB_EINVAL as _lib.check reports it


def small_pair(W, H, n=6, mes=7, seed=77):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    kw = dict(num_envs=n, seed=seed, layout="CWH", obs_width=W, obs_height=H, max_episode_steps=mes)
    return BatchedMiniWorld("MiniWorld-OneRoomS6-v0", **kw), BatchedMiniWorld("MiniWorld-OneRoomS6-v0", **kw)


def run_small_stack(form, dtype, nstack, size, steps, skip_mask=None):
    """n = 6 OneRoomS6 envs with max_episode_steps = 7, `steps` steps: the stack of handle `b` (stack_enable / stack_update driven
    directly) against the restatement fed with the frames of the plain handle `p`.  Returns (dones that were time-outs, early
    finishes, wraps of the window)."""
    import torch
    from stack_ref import FrameStackRef
    W, H = size
    n = 6
    b, p = small_pair(W, H, n=n)
    tdt = {"float32": torch.float32, "uint8": torch.uint8}[dtype]
    C = 3 * nstack
    b.stack_enable(nstack, dtype, **FORMS[form])
    ref = FrameStackRef(n, nstack, (3, W, H), dtype=tdt)
    b.reset(); p.reset()
    st = b.stack_update(after_reset=True)
    assert st.dtype == tdt and tuple(st.shape) == (n, C, W, H)
    assert torch.equal(st.cpu(), ref.reset(p.obs.cpu())), (form, "reset")
    rng = np.random.default_rng(4)
    n_timeout = n_early = n_wrap = 0
    pos = 0
    for t in range(1, steps + 1):
        a = torch.from_numpy(rng.choice(3, size=n, p=[0.2, 0.2, 0.6]).astype(np.int32))
        m = skip_mask if (skip_mask is not None and t % 2 == 0) else None
        prev_frame = p.obs.clone()
        b.step(a, skip_mask=m); p.step(a, skip_mask=m)
        st = b.stack_update()
        done, eps = b.done.cpu().numpy().astype(bool), b.ep_steps.cpu().numpy()
        assert np.array_equal(done, p.done.cpu().numpy().astype(bool)) and torch.equal(b.obs, p.obs), (form, t)
        if m is not None:   # subproc_vec_env.py:26-31
            rew = b.reward.cpu().numpy()
            assert np.all(rew[m != 0] == -99) and not done[m != 0].any(), (form, t)
        n_timeout += int((done & (eps == 7)).sum())
        n_early += int((done & (eps < 7)).sum())
        want = ref.step(p.obs.cpu(), done)
        got = st.cpu()
        if not torch.equal(got, want):
            bad = (got != want).reshape(n, -1).any(dim=1).nonzero().flatten().tolist()
            raise AssertionError((form, dtype, nstack, size, t, "envs whose stack differs", bad, "done", done.tolist()))
        if form != "shifting":
            prev, pos = pos, stack_window(b)[0]
            n_wrap += pos == 0
            assert pos == (0 if prev + 3 + C > stack_window(b)[1] else prev + 3), (form, t, prev, pos)
            if nstack == 1 and pos >= 3:
                # no history to zero: nothing outside the window may be touched - the three planes before it still hold the
                # previous frame of EVERY env, finished or not
                assert torch.equal(b._stack_base[:, pos - 3:pos], prev_frame.to(tdt)), (form, t, "planes before the window were written")
    b.close(); p.close()
    return n_timeout, n_early, n_wrap


@pytest.mark.parametrize("dtype,nstack,size,fused_refused", SHAPES, ids=["%s-n%d-%dx%d" % (d, k, s[0], s[1]) for d, k, s, _ in SHAPES])
@pytest.mark.parametrize("form", list(FORMS))
def test_stack_forms_at_branching_shapes(form, dtype, nstack, size, fused_refused):
    """shifting stack_kernel / stack_slide_kernel modes 0-2 / the fused writer of render_env + the mode-3 wrap copy, each at
    nstack 1, 2, 5, float32 and uint8, the default frame, the two sizes that take the unaligned branches (see SIZE_*) and a
    tiled size - through time-outs, early finishes and three wraps of the window."""
    if form == "fused" and fused_refused:
        from gym_miniworld_amd._lib import MwbError
        b, p = small_pair(*size)
        with pytest.raises(MwbError, match=EINVAL):
            b.stack_enable(nstack, dtype, **FORMS[form])
        b.close(); p.close()
        return
    n_timeout, n_early, n_wrap = run_small_stack(form, dtype, nstack, size, steps=30)
    assert n_timeout > 0 and n_early > 0, (n_timeout, n_early)   # any_done, of both kinds
    if form != "shifting":
        assert n_wrap >= 3, n_wrap


@pytest.mark.parametrize("form", list(FORMS))
def test_stack_forms_with_skip_mask(form):
    """the fork's `mask` (subproc_vec_env.py:26-31,58-67) on a third of the envs on every other step: a skipped env is not
    stepped, reports reward -99 / done False, and its re-rendered current frame is appended to the shifted stack"""
    mask = np.array([1, 0, 0, 1, 0, 0], dtype=np.uint8)
    assert mask.any() and not mask.all()
    n_timeout, n_early, n_wrap = run_small_stack(form, "float32", 4, SIZE_DEFAULT, steps=30, skip_mask=mask)
    assert n_timeout + n_early > 0
    assert form == "shifting" or n_wrap >= 3


def test_stack_enable_refusals():
    """what mwb_stack_enable documents: W * H must be a multiple of 4 (every form); a fused uint8 stack needs a multiple of 16;
    a fused stack needs frames that one workgroup renders whole.  Every refusal is MWB_EINVAL and leaves the handle usable."""
    from gym_miniworld_amd._lib import MwbError
    b, p = small_pair(33, 17)   # 561 = 1 (mod 4)
    for form in FORMS:
        with pytest.raises(MwbError, match=EINVAL):
            b.stack_enable(2, "float32", **FORMS[form])
    b.close(); p.close()
    b, p = small_pair(*SIZE_F32_SCALAR)   # 540 = 12 (mod 16)
    with pytest.raises(MwbError, match=EINVAL):
        b.stack_enable(2, "uint8", **FORMS["fused"])
    b.stack_enable(2, "float32", **FORMS["fused"])   # ... and float is fine there, on the handle that was just refused
    b.close(); p.close()
    b, p = small_pair(*SIZE_TILED)
    with pytest.raises(MwbError, match=EINVAL):
        b.stack_enable(2, "float32", **FORMS["fused"])
    b.stack_enable(2, "float32", **FORMS["sliding"])
    b.close(); p.close()


# ------------------------------------------------------------------------------------------ 4. partial reset
def _rows(st, rows):
    return {k: v[rows] for k, v in st.items() if isinstance(v, np.ndarray)}


@pytest.mark.parametrize("env_id,task,args,dr", [("MiniWorld-FourRooms-v0", "FourRooms", None, 1),
                                                 ("MiniWorld-CollectHealth-v0", "CollectHealth", [16, 0, 0, 0], 0)])
def test_partial_reset_matches_oracle(oracle_mod, env_id, task, args, dr):
    """batch.reset(mask) = mwb_reset with a mask: the masked envs are regenerated as the oracle's reset() does it (state and
    geometry bit for bit, RNG stream continued, step_count 0), the others keep every bit, every frame is the current state's -
    with a mixed mask, an all-zero one and an all-one one - and the steps that follow regenerate nobody a second time."""
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    O = oracle_mod
    n, seed = 40, 61
    b = BatchedMiniWorld(env_id, num_envs=n, seed=seed, domain_rand=dr, want_depth=True)
    envs = [O.OracleEnv(task, seed=seed + i, domain_rand=dr, task_args=args) for i in range(n)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(12)

    def steps(k, tag):
        for t in range(k):
            a = rng.integers(0, b.n_actions, size=n).astype(np.int32)
            b.step(torch.from_numpy(a))
            rew, done, sc = oracle_step_all(envs, a)
            assert_step_outputs(b, rew, done, sc, "%s %s %d" % (env_id, tag, t))

    steps(10, "before")
    mixed = (np.random.default_rng(3).random(n) < 0.4).astype(np.uint8)
    assert 0 < mixed.sum() < n   # zeros and ones
    for name, mask in (("mixed", mixed), ("none", np.zeros(n, np.uint8)), ("all", np.ones(n, np.uint8))):
        tag = "%s mask %s" % (env_id, name)
        m = mask.astype(bool)
        before = b.get_state(rng_state=True)
        b.reset(torch.from_numpy(mask))
        for i in np.nonzero(m)[0]:
            envs[i].reset(render=False)
        after = b.get_state(rng_state=True)
        for k, v in _rows(after, ~m).items():   # not masked: not a bit changes (the MT19937 state included)
            assert np.array_equal(v, _rows(before, ~m)[k]), (tag, k, "an env outside the mask changed")
        assert np.all(after["step_count"][m] == 0), tag
        assert_full_state(b, envs, tag)   # masked: the oracle after reset(); the others: the oracle that was left alone
        for i in range(n):
            assert np.array_equal(b.get_geometry(i)[1], envs[i].geometry()["wall_segs"]), (tag, i, "segs")
        assert_frames(b, envs, range(n), None, tag)
    steps(6, "after")   # a list or reset_set left over from the partial resets would regenerate envs here
    assert_full_state(b, envs, env_id + " end")
    b.check()
    b.close()


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_partial_reset_with_fused_stack(dtype):
    """include/miniworld_batch.h at MWB_STACK_FUSED: a partial mwb_reset(mask) is a step for the window - it moves three planes
    on, the masked envs get a zeroed history and their first frame, the others their re-rendered current frame once more
    (FrameStackRef.partial_reset; the reference has no partial reset).  In mid-rollout, as the pass that wraps the window,
    and on across the next wrap."""
    import torch
    from stack_ref import FrameStackRef
    n, nstack = 12, 4
    b, p = small_pair(80, 60, n=n, mes=7, seed=19)
    tdt = {"float32": torch.float32, "uint8": torch.uint8}[dtype]
    b.stack_enable(nstack, dtype, **FORMS["fused"])
    K = stack_window(b)[1]
    ref = FrameStackRef(n, nstack, (3, 80, 60), dtype=tdt)
    b.reset(); p.reset()
    assert torch.equal(b.stack_update(after_reset=True).cpu(), ref.reset(p.obs.cpu()))
    rng = np.random.default_rng(6)
    mask_rng = np.random.default_rng(7)
    any_done = False
    wrapped_by_partial_reset = wrapped_after = False
    pos, passes = 0, 0
    # passes since the full reset: 4 steps, a partial reset, 3 steps, a partial reset that is the window's 9th pass (the
    # wrap), then 12 steps across the next wrap
    for kind in ["step"] * 4 + ["reset"] + ["step"] * 3 + ["reset"] + ["step"] * 12:
        passes += 1
        if kind == "step":
            a = torch.from_numpy(rng.choice(3, size=n, p=[0.2, 0.2, 0.6]).astype(np.int32))
            b.step(a); p.step(a)
            flags = b.done.cpu().numpy().astype(bool)
            assert np.array_equal(flags, p.done.cpu().numpy().astype(bool)), passes
            any_done |= bool(flags.any())
            want = ref.step(p.obs.cpu(), flags)
        else:
            mask = (mask_rng.random(n) < 0.4).astype(np.uint8)
            assert 0 < mask.sum() < n
            mt = torch.from_numpy(mask)
            b.reset(mt); p.reset(mt)
            flags = mask.astype(bool)
            want = ref.partial_reset(p.obs.cpu(), mask)
        assert torch.equal(b.obs, p.obs), (passes, kind)
        prev, pos = pos, stack_window(b)[0]
        wrap = prev + 3 + 3 * nstack > K
        assert pos == (0 if wrap else prev + 3), (passes, kind, prev, pos)   # three planes on, also for the partial reset
        wrapped_by_partial_reset |= wrap and kind == "reset"
        wrapped_after |= wrap and kind == "step"
        got = b.stack_update().cpu()
        if not torch.equal(got, want):
            bad = (got != want).reshape(n, -1).any(dim=1).nonzero().flatten().tolist()
            raise AssertionError((dtype, passes, kind, "envs whose stack differs", bad, "regenerated", flags.tolist()))
    assert any_done and wrapped_by_partial_reset and wrapped_after
    b.close(); p.close()
