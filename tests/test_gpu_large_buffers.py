"""GPU: per-env buffers that end just past 4 GiB - every address the kernels and the Python views compute from an env index and a
per-env size, executed beyond 2^31 and 2^32 bytes for the first time.

Each case takes the buffer it targets and the smallest batch whose buffer passes 4 GiB by a margin of 64 envs:
N = ceil(2^32 / bytes per env) + 64.  The buffers (and everything larger that comes with them: depth, the last-frame caches)
are checked as a whole on the device with tests/periodic.py - env i is seeded and driven as env i % 13 of Hallway with domain
randomisation, so every buffer must repeat with period 13, every env and every byte - or against the restatement of the frame
stack on the device (tests/stack_ref.py); only the first 13 envs go to the host, where the oracle holds them to +-1 LSB / 1e-4 m.
A truncated offset would land 2^31 or 2^32 bytes early; none of the frame sizes divides 2^31, so that is never an env of the same
class.

Between 5 and 25 GB per case; skipped only on a device of less than 64 GB (an MI355X has 288 GB)."""
import time
import types

import numpy as np
import pytest

from periodic import assert_periodic, periodic_actions, periodic_seeds

pytestmark = pytest.mark.gpu

P = 13
SEED = 4240   # among these 13 worlds a wall blocks one to three forward moves in every step of the action streams below
ENV_ID, TASK = "MiniWorld-Hallway-v0", "Hallway"
FORMS = {"shifting": dict(sliding=False, fused=False), "sliding": dict(sliding=True, fused=False), "fused": dict(sliding=True, fused=True)}


def batch_size(bytes_per_env):
    n = -(-2 ** 32 // bytes_per_env) + 64
    assert (n - 64) * bytes_per_env >= 2 ** 32 > (n - 65) * bytes_per_env and 2 ** 31 % bytes_per_env != 0
    return n


@pytest.fixture(autouse=True)
def device_memory():
    """a device of 64 GB or more; nothing of one case is left allocated for the next; the case's wall time and peak memory printed"""
    import torch
    total = torch.cuda.mem_get_info()[1]
    if total < 64 * 2 ** 30:
        pytest.skip("needs a device of at least 64 GB (this one reports %.1f GB): the buffers under test are larger than 4 GiB each" % (total / 2 ** 30))
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print("  [%.1f s, peak of torch's allocations %.2f GB]" % (time.time() - t0, torch.cuda.max_memory_allocated() / 2 ** 30), end="")


def library_bytes():
    """what the device holds that torch did not allocate: the handles' own buffers"""
    import torch
    free, total = torch.cuda.mem_get_info()
    return total - free - torch.cuda.memory_reserved()


def make(n, W=80, H=60, layout="CWH", mes=None, **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld(ENV_ID, num_envs=n, domain_rand=True, obs_width=W, obs_height=H, layout=layout, max_episode_steps=mes, **kw)
    b.seed(periodic_seeds(n, P, SEED))
    return b


def make_oracles(O, W, H, mes=0):
    return [O.OracleEnv(TASK, seed=SEED + k, domain_rand=True, max_episode_steps=mes, obs_width=W, obs_height=H) for k in range(P)]


def actions(rng, n, p=(0.2, 0.2, 0.6)):
    import torch
    a = rng.choice(3, size=P, p=list(p)).astype(np.int32)
    return a, torch.from_numpy(periodic_actions(a, n))


# ---------------------------------------------------------------------------------------------------- frame stacks
def run_stack(form, dtype, n, copy_across=False):
    """the stacked handle against a plain handle + FrameStackRef on the device, whole stack, exact, after the reset and after each
    of 12 steps; max_episode_steps = 5: histories are zeroed (steps 5 and 10) and the sliding window wraps (step 9) with live
    history.  copy_across: after step 6, MiniWorldVecEnv.copy_envs makes the last 13 envs twins of the first 13 - their windows
    are copied across the 4 GiB line by copy_stack_kernel."""
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    from stack_ref import FrameStackRef
    W, H, nstack = 80, 60, 4
    tdt = {"float32": torch.float32, "uint8": torch.uint8}[dtype]
    b, p = make(n, mes=5), make(n, mes=5)
    st = b.stack_enable(nstack, dtype, **FORMS[form])
    planes = b._stack_base.shape[1]
    assert b._stack_base.numel() * b._stack_base.element_size() == n * planes * W * H * st.element_size() > 2 ** 32
    ref = FrameStackRef(n, nstack, (3, W, H), dtype=tdt, device=b.device)
    b.reset(); p.reset()
    st = b.stack_update(after_reset=True)
    assert st.dtype == tdt and tuple(st.shape) == (n, 3 * nstack, W, H)
    assert torch.equal(st, ref.reset(p.obs)), (form, dtype, "reset")
    rng = np.random.default_rng(4)
    dst, src = list(range(n - P, n)), list(range(P))
    assert all(d % P != s % P for d, s in zip(dst, src))   # the copy changes its destinations
    twins = False
    any_done = 0
    for t in range(1, 13):
        _, a = actions(rng, n)
        if twins:
            a[dst] = a[src]
        b.step(a); p.step(a)
        st = b.stack_update()
        assert torch.equal(b.done, p.done) and torch.equal(b.obs, p.obs), (form, dtype, t)
        any_done += int(p.done.sum())
        want = ref.step(p.obs, p.done)
        if not torch.equal(st, want):
            bad = (st != want).reshape(n, -1).any(dim=1).nonzero().flatten().tolist()
            raise AssertionError((form, dtype, t, "envs whose stack differs", bad[:8], len(bad)))
        if not twins:
            assert_periodic(st, P, "%s %s stack, step %d" % (form, dtype, t))
        if copy_across and t == 6:
            vec = types.SimpleNamespace(batch=b, nstack=nstack, greyscale=False, to_float=True)   # the VecEnv's method on this handle's stack form
            st = MiniWorldVecEnv.copy_envs(vec, dst, src)
            p.copy_envs(dst, src)
            ref.stacked[dst] = ref.stacked[src]
            assert torch.equal(st[dst], st[src]) and torch.equal(st, ref.stacked), (form, "after the copy across the 4 GiB line")
            assert torch.equal(b.obs, p.obs)
            twins = True
    assert any_done >= n, any_done
    if twins:
        assert torch.equal(st[dst], st[src]) and torch.equal(b.obs[dst], b.obs[src])
        assert_periodic(st[:n - P], P, "%s %s stack, the envs that were not copied" % (form, dtype))
    print("  [library %.2f GB]" % (library_bytes() / 2 ** 30), end="")
    b.close(); p.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_float32_stack_past_4_gib(form):
    """80 x 60 CWH, the workload's own frame.  Shifting: 12 planes, 230 400 B per env, N = 18 706.  Sliding and fused: a window
    over 36 planes, 691 200 B per env, N = 6 278."""
    n = batch_size(230400 if form == "shifting" else 691200)
    assert n == (18706 if form == "shifting" else 6278)
    run_stack(form, "float32", n, copy_across=form == "sliding")


def test_uint8_shifting_stack_past_4_gib():
    """57 600 B per env, N = 74 630: also more than 65 535 envs at the default frame"""
    n = batch_size(57600)
    assert n == 74630 and n > 65535
    run_stack("shifting", "uint8", n)


# ------------------------------------------------------------------------------- observation, depth, frame caches
def hwc(obs, layout):
    obs = obs.cpu().numpy()
    return obs.transpose(0, 3, 2, 1) if layout == "CWH" else obs


def assert_first_frames(b, envs, tag):
    obs, dep = hwc(b.obs[:P], b.layout), b.depth[:P].cpu().numpy()[..., 0]
    for i, e in enumerate(envs):
        ref, refd = e.render_obs(depth=True)
        d = np.abs(obs[i].astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1, (tag, i, int(d.max()), int((d > 1).sum()))
        dd = float(np.abs(dep[i] - refd).max())
        assert dd <= 1e-4, (tag, i, "depth", dd)


def run_frames(O, W, H, layout, tiled):
    """reset and 4 steps, forward-heavy so that walls block some moves (the bulk pass then copies those envs' frames and depth
    maps out of the last-frame caches: reuse_frame, where frames are reused at all - not in tiles)"""
    n = batch_size(W * H * 3)
    b = make(n, W, H, layout, want_depth=True)
    assert b.obs.numel() > 2 ** 32 and b.depth.numel() * 4 > b.obs.numel()
    envs = make_oracles(O, W, H)
    b.reset()
    for e in envs:
        e.reset(render=False)
    tag = "%dx%d %s" % (W, H, layout)
    assert_periodic(b.obs, P, tag + " obs, reset")
    assert_periodic(b.depth, P, tag + " depth, reset")
    assert_first_frames(b, envs, tag + " reset")
    b.frame_reuse_stats()
    rng = np.random.default_rng(11)
    blocked = 0
    for t in range(4):
        a, a_all = actions(rng, n, p=(0.1, 0.1, 0.8))
        b.obs.zero_(); b.depth.zero_()
        b.step(a_all)
        for i, e in enumerate(envs):
            before = list(e.state().agent_pos)
            _, _, done, _ = e.step(int(a[i]))
            blocked += a[i] == 2 and not done and list(e.state().agent_pos) == before
            assert done == bool(b.done[i]), (tag, t, i)
            if done:
                e.reset(render=False)
        assert_periodic(b.obs, P, "%s obs, step %d" % (tag, t))
        assert_periodic(b.depth, P, "%s depth, step %d" % (tag, t))
    assert_first_frames(b, envs, tag + " end")
    reused, rendered = b.frame_reuse_stats()
    assert blocked > 0, "no forward move of the 13 classes was blocked: the action mix does not reach reuse_frame"
    if tiled:
        assert reused == 0   # tiles: no last-frame cache (mwb_frame_reuse_stats)
    else:
        assert reused > 0 and reused + rendered == 4 * n, (reused, rendered)
        assert reused >= blocked * (n // P), (reused, blocked)   # every env of a blocked class, to the last one
    b.check()
    print("  [library %.2f GB]" % (library_bytes() / 2 ** 30), end="")
    b.close()


def test_obs_depth_and_frame_caches_past_4_gib(oracle_mod):
    """256 x 192 HWC with depth, one workgroup per frame: obs and the frame cache 147 456 B per env (N = 29 192: 4.0 GiB each),
    depth and the depth cache 5.3 GiB each"""
    assert batch_size(256 * 192 * 3) == 29192
    run_frames(oracle_mod, 256, 192, "HWC", tiled=False)


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
def test_tiled_obs_and_depth_past_4_gib(oracle_mod, layout):
    """512 x 384, rendered in 75 x 60 tiles: 589 824 B per env, N = 7 346; CWH: the plane-strided tile write-out"""
    assert batch_size(512 * 384 * 3) == 7346
    run_frames(oracle_mod, 512, 384, layout, tiled=True)


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
def test_grey_past_4_gib(layout):
    """greyscale=True at 256 x 192: the float32 grey buffer is 196 608 B per env, N = 21 910"""
    import torch
    from grey_ref import grey_ref
    W, H = 256, 192
    n = batch_size(W * H * 4)
    assert n == 21910
    b = make(n, W, H, layout, greyscale=True)
    assert b.grey.numel() * 4 > 2 ** 32
    b.reset()
    rng = np.random.default_rng(12)
    for t in range(5):
        if t:
            b.grey.zero_()
            b.step(actions(rng, n, p=(0.1, 0.1, 0.8))[1])
        assert_periodic(b.grey, P, "grey %s, pass %d" % (layout, t))
        assert_periodic(b.obs, P, "obs %s, pass %d" % (layout, t))
        assert np.array_equal(b.grey[:P].cpu().numpy(), grey_ref(b.obs[:P].cpu().numpy(), layout)), (layout, t)
    assert b.frame_reuse_stats()[0] > 0   # grey frames computed from the last-frame cache were among them
    assert torch.count_nonzero(b.grey[n - 1]) > 0
    print("  [library %.2f GB]" % (library_bytes() / 2 ** 30), end="")
    b.close()
