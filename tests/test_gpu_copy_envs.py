"""GPU: copying environments on the device (mwb_copy_envs): clone inside a handle, snapshot into an archive handle and restore.

The yardstick is the library's own uncopied path, which the parity tests pin to the oracle (the twin method of
tests/test_gpu_frame_reuse.py): a copied env must be indistinguishable from its source - stepped with the same actions the two
agree BIT FOR BIT at every later step, through episode ends and auto-resets - and the envs a copy does not name must be what they
are in a handle that never saw a copy.  Every comparison is equality; there are no tolerances.  Out-of-range indices are never
sent to the GPU here (tests/test_copy_envs_host.py covers them on the CPU)."""
import types

import numpy as np
import pytest

from stack_ref import FrameStackRef
from test_gpu_frame_reuse import pose, scribble

pytestmark = pytest.mark.gpu
N, HALF = 96, 48   # not a multiple of 64


def make(env_id, n=N, seed=11, **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    return BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)


def dev_idx(b, v):
    import torch
    return torch.as_tensor(np.asarray(v, np.int32)).to(b.device)


def frames(b):
    """every per-step output buffer that holds frames"""
    out = {"obs": b.obs}
    if b.depth is not None:
        out["depth"] = b.depth
    if b.grey is not None:
        out["grey"] = b.grey
    return out


def assert_frames_equal(a, ia, b, ib, tag):
    import torch
    fa, fb = frames(a), frames(b)
    for k in fa:
        x, y = fa[k][ia], fb[k][ib]
        assert torch.equal(x, y), (tag, k, "envs differing:", int((x != y).reshape(x.shape[0], -1).any(dim=1).sum()))


def assert_transition_equal(a, ia, b, ib, tag):
    import torch
    for k in ("reward64", "done", "ep_steps"):
        assert torch.equal(getattr(a, k)[ia], getattr(b, k)[ib]), (tag, k)


def assert_state_equal(a, ia, b, ib, tag, geometry=True):
    """the whole mwb_get_state (MT19937 words and entity order included) and mwb_get_geometry, bit for bit"""
    sa, sb = a.get_state(rng_state=True), b.get_state(rng_state=True)
    assert set(sa) == set(sb)
    for k in sa:
        x, y = np.ascontiguousarray(sa[k][ia]), np.ascontiguousarray(sb[k][ib])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, k)
    if geometry:
        for ea, eb in zip(ia, ib):
            (ra, ga), (rb, gb) = a.get_geometry(int(ea)), b.get_geometry(int(eb))
            assert ra.shape == rb.shape and ra.tobytes() == rb.tobytes() and ga.shape == gb.shape and ga.tobytes() == gb.tobytes(), (tag, "geometry", ea, eb)


def random_policy(rng):
    return lambda b, t: rng.integers(0, b.n_actions, b.num_envs).astype(np.int32)


def putnext_fetch_policy(rng):
    """the box-fetching policy of tests/test_gpu_putnext.py, fed from the library's own state"""
    from test_gpu_putnext import fetch_action

    def policy(b, t):
        st = b.get_state()
        return np.array([fetch_action(types.SimpleNamespace(agent_pos=st["agent_pos"][i], agent_dir=st["agent_dir"][i], boxes_pos=st["boxes_pos"][i],
                                                            boxes_size=st["boxes_size"][i], carrying=int(st["carrying"][i])), rng)
                         for i in range(b.num_envs)], dtype=np.int32)
    return policy


def recorded_stream_policy(aseed, column0, n_actions):
    """the action streams tests/test_gpu_frame_reuse.py chose on the CPU oracle (some env picks an object up within ten steps):
    env i of this batch replays column column0 + i of np.random.default_rng(aseed).integers(0, n_actions, (60, 64)) while it has one,
    everybody ends on a turn - a pick-up in the very last step would leave the source's observation showing the step's own frame
    (the object still drawn) where a copy renders the current state"""
    table = np.random.default_rng(aseed).integers(0, n_actions, (60, 64))
    rng = np.random.default_rng(aseed + 1)

    def policy(b, t):
        a = rng.integers(0, n_actions, b.num_envs)
        k = min(b.num_envs, 64 - column0)
        a[:k] = table[t, column0:column0 + k]
        if t == PRE_STEPS - 1:
            a[:] = 0
        return a.astype(np.int32)
    return policy


PRE_STEPS = 25


def carrying_somewhere(a, st0):
    st = a.get_state()
    assert (st["carrying"][:HALF] >= 0).any(), "no source env carries a box at the copy: the policy / seed no longer produce the case"
    assert (st["boxes_pos"][:HALF, :, 1] > 0).any()


def order_changed(a, st0):
    st = a.get_state()
    same_episode = st["step_count"][:HALF] == PRE_STEPS
    assert (same_episode & (st["ent_order"][:HALF] != st0["ent_order"][:HALF]).any(axis=1)).any(), \
        "no source env's entity list has changed by the copy: the recorded action stream no longer picks anything up"


CLONE_CASES = {
    # id: (env id, constructor arguments, policy before the copy, what must hold among the sources at the copy, steps before it)
    "maze-dr0-hwc": ("MiniWorld-Maze-v0", dict(domain_rand=False, layout="HWC"), None, None, PRE_STEPS),
    "maze-dr1-hwc": ("MiniWorld-Maze-v0", dict(domain_rand=True, layout="HWC"), None, None, PRE_STEPS),
    "maze-dr0-cwh": ("MiniWorld-Maze-v0", dict(domain_rand=False, layout="CWH"), None, None, PRE_STEPS),
    "maze-dr1-cwh": ("MiniWorld-Maze-v0", dict(domain_rand=True, layout="CWH"), None, None, PRE_STEPS),
    "putnext-carrying": ("MiniWorld-PutNext-v0", dict(seed=40, max_episode_steps=100), putnext_fetch_policy, carrying_somewhere, 60),
    # seed 700 + 43 / 700 + 48: env 0 here is env 43 / 48 of the batches tests/test_gpu_frame_reuse.py drives with these streams
    "collecthealth-pickup": ("MiniWorld-CollectHealth-v0", dict(seed=743), lambda rng: recorded_stream_policy(0, 43, 8), order_changed, PRE_STEPS),
    "pickupobjs-pickup": ("MiniWorld-PickupObjs-v0", dict(seed=748), lambda rng: recorded_stream_policy(41, 48, 5), order_changed, PRE_STEPS),
    "tmaze-twobox-counters": ("MiniWorld-TMazeTwoBoxDynamicFeaturesDebug-v0", dict(domain_rand=True), None, None, PRE_STEPS),
    "ymaze-polygon-rooms": ("MiniWorld-YMaze-v0", dict(domain_rand=True), None, None, PRE_STEPS),
    "sign-text": ("MiniWorld-Sign-v0", dict(), None, None, PRE_STEPS),
    "simtorealpush-sizes": ("MiniWorld-SimToRealPush-v0", dict(), None, None, PRE_STEPS),
}


@pytest.mark.parametrize("case", sorted(CLONE_CASES))
def test_clone_inside_a_handle(case):
    import torch
    env_id, kw, policy, holds, pre = CLONE_CASES[case]
    kw = dict(dict(seed=11, max_episode_steps=40, want_depth=True, greyscale=True), **kw)
    a, b = make(env_id, **kw), make(env_id, **kw)   # b: the twin that takes no copies
    a.reset(); b.reset()
    st0 = a.get_state()
    rng = np.random.default_rng(3)
    policy = (policy or random_policy)(rng)
    for t in range(pre):
        acts = torch.from_numpy(policy(a, t))
        a.step(acts); b.step(acts)
    if holds is not None:
        holds(a, st0)
    lo, hi = np.arange(HALF), np.arange(HALF, N)
    before = {k: v[:HALF].clone() for k, v in frames(a).items()}
    a.copy_envs(dev_idx(a, hi), dev_idx(a, lo))
    assert a.copy_rejected() == 0
    for k, v in before.items():
        assert torch.equal(frames(a)[k][:HALF], v), (case, "the copy wrote a source's", k)
    assert_frames_equal(a, hi, a, lo, (case, "copy"))
    assert_state_equal(a, hi, a, lo, (case, "copy"))
    assert_frames_equal(a, lo, b, lo, (case, "copy, sources against the twin"))
    assert_state_equal(a, lo, b, lo, (case, "copy, sources against the twin"), geometry=False)
    regenerated = 0
    for t in range(1, 61):
        acts = rng.integers(0, a.n_actions, N).astype(np.int32)
        acts[HALF:] = acts[:HALF]
        acts = torch.from_numpy(acts)
        scribble(a, b)
        a.step(acts); b.step(acts)
        assert_frames_equal(a, hi, a, lo, (case, t))
        assert_transition_equal(a, hi, a, lo, (case, t))
        assert_frames_equal(a, lo, b, lo, (case, t, "sources against the twin"))
        assert_transition_equal(a, lo, b, lo, (case, t, "sources against the twin"))
        regenerated += int(a.done[HALF:].sum())
        if t in (1, 20, 60):
            assert_state_equal(a, hi, a, lo, (case, t))
    assert regenerated > 0, "no copied env ended and regenerated"
    a.check()
    a.close(); b.close()


def test_snapshot_and_restore_across_handles_of_different_size():
    import torch
    a = make("MiniWorld-Maze-v0", domain_rand=True, want_depth=True, max_episode_steps=40, seed=5)
    a.reset()
    rng = np.random.default_rng(9)
    for t in range(15):
        a.step(torch.from_numpy(rng.integers(0, 3, N).astype(np.int32)))
    envs, slots = [3, 64, 95, 17], [9, 0, 4, 5]
    arch = a.archive(10)
    assert arch.num_envs == 10
    a.save(arch, slots, envs)
    saved = {k: v[envs].clone() for k, v in frames(a).items()}
    acts = rng.integers(0, 3, (30, N)).astype(np.int32)

    def run(which, columns):
        rec = []
        for t in range(30):
            step = acts[t].copy()
            step[which] = acts[t][columns]
            scribble(a)
            a.step(torch.from_numpy(step))
            rec.append({k: getattr(a, k)[which].clone() for k in ("obs", "depth", "reward64", "done", "ep_steps")})
        st = a.get_state(rng_state=True)
        return rec, {k: np.ascontiguousarray(v[which]).tobytes() for k, v in st.items()}

    first, state_first = run(envs, envs)
    assert sum(int(r["done"].sum()) for r in first) > 0   # the recording runs through episode ends
    for which in (envs, [0, 50, 70, 33]):   # the same envs, then four others: the archive was not disturbed
        others = np.setdiff1d(np.arange(N), which)
        keep = {k: v[others].clone() for k, v in frames(a).items()}
        a.restore(arch, slots, which)
        assert a.copy_rejected() == 0
        for k, v in saved.items():
            assert torch.equal(frames(a)[k][which], v), ("restore", k)
        for k, v in keep.items():
            assert torch.equal(frames(a)[k][others], v), ("restore wrote another env's", k)
        again, state_again = run(which, envs)
        for t in range(30):
            for k in first[t]:
                assert torch.equal(first[t][k], again[t][k]), ("replay", which, t, k)
        assert state_again == state_first
    assert arch.copy_rejected() == 0
    # one pair
    a.copy_envs([5], [20])
    assert_state_equal(a, [5], a, [20], "count 1")
    assert_frames_equal(a, [5], a, [20], "count 1")
    # every env at once, permuted, from a second handle of the same size
    c = make("MiniWorld-Maze-v0", domain_rand=True, want_depth=True, max_episode_steps=40, seed=77)
    c.reset()
    for t in range(3):
        c.step(torch.from_numpy(rng.integers(0, 3, N).astype(np.int32)))
    perm = rng.permutation(N)
    a.copy_envs(dev_idx(a, np.arange(N)), dev_idx(a, perm), src=c)
    assert a.copy_rejected() == 0
    assert_state_equal(a, np.arange(N), c, perm, "count N")
    assert_frames_equal(a, np.arange(N), c, perm, "count N")
    step = rng.integers(0, 3, N).astype(np.int32)
    a.step(torch.from_numpy(step)); c.step(torch.from_numpy(step[np.argsort(perm)]))   # env perm[i] of c takes env i's action
    assert_frames_equal(a, np.arange(N), c, perm, "count N, one step on")
    assert_transition_equal(a, np.arange(N), c, perm, "count N, one step on")
    a.close(); arch.close(); c.close()


STACK_FORMS = {"fused-f32": dict(dtype="float32", fused=True), "fused-grey": dict(dtype="float32", fused=True, grey=True),
               "sliding-u8": dict(dtype="uint8", sliding=True), "shifting-f32": dict(dtype="float32", sliding=False)}


@pytest.mark.parametrize("nstack", [4, 2])
@pytest.mark.parametrize("form", sorted(STACK_FORMS))
def test_frame_stack_window_is_copied(form, nstack):
    """rule 2: both handles (here: one) have the same stack - the destination's visible window becomes the source's"""
    import torch
    n, half = 32, 16
    a = make("MiniWorld-MazeS3-v0", n=n, layout="CWH", greyscale="grey" in form, max_episode_steps=30, seed=2)
    a.stack_enable(nstack, **STACK_FORMS[form])
    a.reset()
    a.stack_update(after_reset=True)
    rng = np.random.default_rng(4)
    for t in range(5):
        a.step(torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)))
        a.stack_update()
    lo, hi = np.arange(half), np.arange(half, n)
    assert not torch.equal(a.stack[half:], a.stack[:half])
    a.copy_envs(dev_idx(a, hi), dev_idx(a, lo))
    assert torch.equal(a.stack[half:], a.stack[:half]), (form, nstack, "copy")
    assert (a.stack[half:, :-a.stack.shape[1] // nstack] != 0).any(), "the copied history is not empty"
    a.render()   # the destinations are no longer marked as regenerated: a render leaves their history alone
    assert torch.equal(a.stack[half:], a.stack[:half]), (form, nstack, "render after the copy")
    assert (a.stack[half:, :-a.stack.shape[1] // nstack] != 0).any()
    for t in range(12):   # past a wrap of the sliding window (MWB_STACK_SLACK_FRAMES = 8)
        acts = rng.integers(0, 3, n).astype(np.int32)
        acts[half:] = acts[:half]
        a.step(torch.from_numpy(acts))
        st = a.stack_update()
        assert torch.equal(st[half:], st[:half]), (form, nstack, t)
    a.close()


def test_frame_stack_forms_may_differ_between_the_handles():
    """rule 2 across handles: a sliding window (window position moving) into a fused one of another size"""
    import torch
    src = make("MiniWorld-MazeS3-v0", n=24, layout="CWH", seed=2)
    dst = make("MiniWorld-MazeS3-v0", n=40, layout="CWH", seed=90)
    src.stack_enable(4, dtype="float32", sliding=True)
    dst.stack_enable(4, dtype="float32", fused=True)
    src.reset(); src.stack_update(after_reset=True)
    dst.reset()
    rng = np.random.default_rng(4)
    for t in range(6):
        src.step(torch.from_numpy(rng.integers(0, 3, 24).astype(np.int32)))
        src.stack_update()
    for t in range(3):
        dst.step(torch.from_numpy(rng.integers(0, 3, 40).astype(np.int32)))
    d, s = np.arange(10, 34), rng.permutation(24)
    untouched = dst.stack_update()[:10].clone()
    dst.copy_envs(dev_idx(dst, d), dev_idx(dst, s), src=src)
    assert torch.equal(dst.stack[d], src.stack[s]) and torch.equal(dst.stack[:10], untouched)
    for t in range(12):
        acts = rng.integers(0, 3, 24).astype(np.int32)
        full = rng.integers(0, 3, 40).astype(np.int32)
        full[d] = acts[s]
        src.step(torch.from_numpy(acts)); dst.step(torch.from_numpy(full))
        assert torch.equal(dst.stack_update()[d], src.stack_update()[s]), t
    src.close(); dst.close()


@pytest.mark.parametrize("nstack", [4, 2])
def test_fused_stack_without_a_source_stack_starts_a_new_history(nstack):
    """rule 3, against tests/stack_ref.py: zero history + the new frame, then the window builds up"""
    import torch
    from gym_miniworld_amd import _lib
    n, half = 32, 16
    a = make("MiniWorld-MazeS3-v0", n=n, layout="CWH", max_episode_steps=30, seed=2)
    plain = make("MiniWorld-MazeS3-v0", n=half, layout="CWH", max_episode_steps=30, seed=50)   # no stack
    a.stack_enable(nstack, dtype="float32", fused=True)
    ref = FrameStackRef(n, nstack, (3, a.W, a.H), device=a.device)
    a.reset(); plain.reset()
    ref.reset(a.obs)
    rng = np.random.default_rng(4)
    for t in range(5):
        a.step(torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)))
        plain.step(torch.from_numpy(rng.integers(0, 3, half).astype(np.int32)))
        assert torch.equal(a.stack_update(), ref.step(a.obs, a.done))
    hi = np.arange(half, n)
    with pytest.raises(_lib.MwbError, match="error -1"):   # no frame to start the new history with
        a.copy_envs(dev_idx(a, hi), dev_idx(a, np.arange(half)), src=plain, render=False)
    assert torch.equal(a.stack, ref.stacked)
    a.copy_envs(dev_idx(a, hi), dev_idx(a, np.arange(half)), src=plain)
    ref.stacked[half:] = 0
    ref.stacked[half:, -3:] = a.obs[half:].float()
    assert torch.equal(a.stack, ref.stacked)
    plain.render()
    assert torch.equal(a.obs[half:], plain.obs)
    for t in range(nstack + 1):
        a.step(torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)))
        assert torch.equal(a.stack_update(), ref.step(a.obs, a.done)), t
    a.close(); plain.close()


def test_a_stack_that_is_not_fused_needs_a_source_stack_of_its_kind():
    """rule 4"""
    from gym_miniworld_amd import _lib
    a = make("MiniWorld-MazeS3-v0", n=8, layout="CWH")
    plain = make("MiniWorld-MazeS3-v0", n=8, layout="CWH")
    other = make("MiniWorld-MazeS3-v0", n=8, layout="CWH")
    a.stack_enable(4, dtype="float32", sliding=True)
    other.stack_enable(2, dtype="float32", sliding=True)
    for h in (a, plain, other):
        h.reset()
    a.stack_update(after_reset=True); other.stack_update(after_reset=True)
    before = a.stack.clone()
    st = a.get_state(rng_state=True)
    for src in (plain, other):
        for render in (True, False):
            with pytest.raises(_lib.MwbError, match="error -1"):
                a.copy_envs([0, 1], [2, 3], src=src, render=render)
    assert all(np.array_equal(v, a.get_state(rng_state=True)[k]) for k, v in st.items())
    assert (a.stack == before).all()
    plain.copy_envs([0, 1], [2, 3], src=a)   # rule 1: only the source has a stack - nothing to do about it
    assert_state_equal(plain, [0, 1], a, [2, 3], "rule 1")
    for h in (a, plain, other):
        h.close()


def test_last_frame_reuse_after_a_copy_and_envs_a_copy_does_not_name():
    import torch
    n = 24
    a = make("MiniWorld-OneRoom-v0", n=n, seed=9, want_depth=True)   # the room is (0, 10) x (0, 10), agent radius 0.4
    a.reset()
    fwd = torch.full((n,), 2, dtype=torch.int32)
    z = np.linspace(3.0, 7.0, 8)
    a.set_agent(0, pos_xz=np.stack([np.full(8, 10.0 - 0.4 - 0.01), z], axis=1), dir=np.zeros(8))   # touching the east wall, facing it
    a.step(fwd)
    src = np.arange(8)
    # state only: nobody's frames change; the first step afterwards renders the destinations
    d1 = np.arange(8, 16)
    obs0, dep0 = a.obs.clone(), a.depth.clone()
    a.copy_envs(dev_idx(a, d1), dev_idx(a, src), render=False)
    torch.cuda.synchronize()
    assert torch.equal(a.obs, obs0) and torch.equal(a.depth, dep0)
    assert_state_equal(a, d1, a, src, "state only")
    def blocked_step():
        """one move_forward for everybody -> (frames reused, frames rendered, which envs the step left exactly as they were)"""
        a.frame_reuse_stats()
        prev = pose(a.get_state())
        scribble(a)
        a.step(fwd)
        still = (pose(a.get_state()) == prev).all(axis=1) & (a.done.cpu().numpy() == 0)
        return a.frame_reuse_stats() + (still,)

    reused, rendered, still = blocked_step()
    assert still[src].all() and still[d1].all(), "the move was meant to be blocked"
    not_d1 = np.setdiff1d(np.arange(n), d1)
    # the sources stand still and reuse their frames; the destinations stand still too, but their frame on record is stale
    assert reused == int(still[not_d1].sum()) and reused + rendered == n, (reused, rendered)
    assert_frames_equal(a, d1, a, src, "first step after a copy without render")
    again = a.obs.clone()
    a.render()
    assert torch.equal(a.obs, again)
    # rendered: the copy leaves the frame on record, so the blocked move that follows reuses it
    d2 = np.arange(16, 24)
    others = np.arange(16)
    keep_obs, keep_dep = a.obs[others].clone(), a.depth[others].clone()
    a.copy_envs(dev_idx(a, d2), dev_idx(a, src))
    assert torch.equal(a.obs[others], keep_obs) and torch.equal(a.depth[others], keep_dep)
    assert_frames_equal(a, d2, a, src, "copy")
    reused, rendered, still = blocked_step()
    assert still[src].all() and still[d1].all() and still[d2].all()
    assert reused == int(still.sum()) and reused + rendered == n, (reused, rendered)   # the destinations' frames are on record
    assert_frames_equal(a, d2, a, src, "blocked step after the copy")
    assert_frames_equal(a, d1, a, src, "blocked step after the copy")
    again = a.obs.clone()
    a.render()
    assert torch.equal(a.obs, again)
    a.close()


def test_rejected_pairs_are_left_alone_and_counted():
    import torch
    n = 16
    a = make("MiniWorld-MazeS3-v0", n=n, seed=21, want_depth=True)
    a.reset()
    rng = np.random.default_rng(1)
    for t in range(6):
        a.step(torch.from_numpy(rng.integers(0, 3, n).astype(np.int32)))
    assert a.copy_rejected() == 0   # before any copy
    #        duplicate destination   fine    3 is also a source   fine     identity
    pairs = [(8, 0), (8, 1),         (9, 2), (3, 4), (10, 3),     (11, 5), (12, 12)]
    dst, src = [p[0] for p in pairs], [p[1] for p in pairs]
    with pytest.raises(ValueError):   # a host list is checked on the host ...
        a.copy_envs(dst, src)
    st0 = a.get_state(rng_state=True)
    fr0 = {k: v.clone() for k, v in frames(a).items()}
    a.copy_envs(dev_idx(a, dst), dev_idx(a, src))   # ... a device list by the validation kernel
    assert a.copy_rejected() == 3
    assert a.copy_rejected() == 0
    st1 = a.get_state(rng_state=True)
    copied = [9, 10, 11]
    left = np.setdiff1d(np.arange(n), copied)   # the rejected pairs' destinations 8 and 3, the identity pair's 12, everybody else
    for k in st0:
        assert np.ascontiguousarray(st0[k][left]).tobytes() == np.ascontiguousarray(st1[k][left]).tobytes(), k
    for k, v in fr0.items():
        assert torch.equal(frames(a)[k][left], v[left]), k
    assert_state_equal(a, copied, a, [2, 3, 5], "accepted pairs")
    assert_frames_equal(a, copied, a, [2, 3, 5], "accepted pairs")
    # the scratch of the validation is clean again: the same destinations are accepted by the next call
    a.copy_envs(dev_idx(a, [8, 3]), dev_idx(a, [0, 4]))
    assert a.copy_rejected() == 0
    assert_state_equal(a, [8, 3], a, [0, 4], "second call")
    a.copy_envs(dev_idx(a, []), dev_idx(a, []))   # count 0: a no-op
    assert a.copy_rejected() == 0
    a.close()


def test_config_mismatch_and_handles_that_cannot_take_part():
    from gym_miniworld_amd import _lib
    a = make("MiniWorld-MazeS3-v0", n=8, seed=1)
    a.reset()
    st0 = a.get_state(rng_state=True)
    obs0 = a.obs.clone()
    for field, other in (("task", make("MiniWorld-OneRoom-v0", n=8, seed=1)),
                         ("obs_width", make("MiniWorld-MazeS3-v0", n=8, seed=1, obs_width=64)),
                         ("max_episode_steps", make("MiniWorld-MazeS3-v0", n=8, seed=1, max_episode_steps=77))):
        other.reset()
        for render in (True, False):
            with pytest.raises(_lib.MwbError, match="error -1.*`%s`" % field):
                a.copy_envs([0], [1], src=other, render=render)
        other.close()
    fresh = make("MiniWorld-MazeS3-v0", n=4, seed=None)   # never reset: MWB_ESTATE as a source ...
    with pytest.raises(_lib.MwbError, match="error -4"):
        a.copy_envs([0], [1], src=fresh)
    with pytest.raises(_lib.MwbError, match="error -4"):   # ... and, unseeded, as the destination of a rendering copy
        fresh.copy_envs([0], [1], src=a)
    fresh.copy_envs([0], [1], src=a, render=False)   # state alone needs nothing of the destination
    assert_state_equal(fresh, [0], a, [1], "into an unseeded handle")
    st1 = a.get_state(rng_state=True)
    assert all(np.array_equal(st0[k], st1[k]) for k in st0) and (a.obs == obs0).all()
    a.close(); fresh.close()


def test_vec_env_copy_returns_the_views_own_observation():
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    v = MiniWorldVecEnv("MiniWorld-MazeS3-v0", 12, seed=4, frame_stack=4)
    v.reset()
    for t in range(3):
        v.step(torch.randint(0, 3, (12, 1), device=v.device))
    obs = v.copy_envs(list(range(6, 12)), list(range(6)))
    assert obs.shape == (12, 12, 80, 60) and obs.dtype == torch.float32
    assert torch.equal(obs[6:], obs[:6]) and (obs[6:, :9] != 0).any()
    arch = v.batch.archive(3)
    v.batch.save(arch, [0, 1, 2], [9, 10, 11])
    want = obs[9:12].clone()
    v.step(torch.randint(0, 3, (12, 1), device=v.device))
    obs = v.copy_envs([3, 4, 5], [0, 1, 2], src=arch)
    assert torch.equal(obs[3:6], want)
    plain = MiniWorldVecEnv("MiniWorld-MazeS3-v0", 12, seed=4, to_float=False)
    plain.reset()
    o = plain.copy_envs([1], [0])
    assert o.dtype == torch.uint8 and torch.equal(o[1], o[0])
    other = MiniWorldVecEnv("MiniWorld-MazeS3-v0", 4, seed=8, to_float=False)
    other.reset()
    o = plain.copy_envs([2, 3], [3, 0], src=other)
    assert torch.equal(o[2], other.batch.obs[3]) and torch.equal(o[3], other.batch.obs[0])
    for e in (v, plain, other):
        e.close()
    arch.close()
