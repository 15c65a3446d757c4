"""GPU: the rollout storage (mwb_rollout_* / BatchedMiniWorld.rollout_enable / MiniWorldVecEnv(rollout_steps=T)).

The yardstick is tests/stack_ref.py::FrameStackRef - the reference's VecPyTorchFrameStack restated in torch - fed with the cloned
batch.obs (or batch.grey) and batch.done of every step, never the rollout's own output: what the rollout rebuilds from its ring
of single frames must equal, bit for bit, the stacked observation FrameStackRef held at that step.  Snapshots of the reference
are kept per logical time of the window; after_update makes snapshot[T] snapshot[0], as RolloutStorage.after_update does."""
import ctypes

import numpy as np
import pytest

from stack_ref import FrameStackRef

pytestmark = pytest.mark.gpu

N = 16
EPISODE = 6   # max_episode_steps of the staggered batches: with step counters 0 .. 5 at the start, envs end on every step


def make(env_id, n=N, seed=3, **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    kw.setdefault("layout", "CWH")
    return BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)


def actions(rng, n=N):
    import torch
    return torch.from_numpy(np.where(rng.random(n) < 0.6, 2, rng.integers(0, 2, n)).astype(np.int32))


class Driver:
    """a batch, its rollout and the reference beside it"""

    def __init__(self, b, num_steps, nstack, grey=False, stagger=True):
        import torch
        self.torch, self.b, self.T, self.nstack, self.grey = torch, b, num_steps, nstack, grey
        self.ro = b.rollout_enable(num_steps=num_steps, nstack=nstack, grey=grey)
        self.ref = FrameStackRef(b.num_envs, nstack, (1 if grey else 3, b.W, b.H), device=b.device)
        self.snap = {}
        self.stagger = stagger
        self.windows = 0
        self.seen = {"done_t1": 0, "done_tT": 0, "prev_window": 0, "ages_after_update": set()}

    def frame(self):
        return (self.b.grey if self.grey else self.b.obs).clone()

    def reset(self):
        b = self.b
        b.reset()
        if self.stagger:   # episode ends fall on every step of the window
            b.set_agent(0, step_count=(np.arange(b.num_envs) % EPISODE).astype(np.int32))
        self.ro.push(after_reset=True)
        self.snap = {0: self.ref.reset(self.frame()).clone()}
        assert self.ro.step == 0

    def record(self, news):
        """after a pass and its push: the reference takes the same frame with the flags `news`"""
        t = self.ro.step
        self.snap[t] = self.ref.step(self.frame(), news).clone()
        self.seen["done_t1"] += int(t == 1 and bool(self.torch.as_tensor(news).any()))
        self.seen["done_tT"] += int(t == self.T and bool(self.torch.as_tensor(news).any()))
        ages = self.ro.ages[:t + 1].cpu().numpy()
        self.seen["prev_window"] += int(self.windows > 0 and (ages > np.arange(t + 1)[:, None]).any())   # a frame of time t - j < 0 is read
        return t

    def step(self, a):
        self.b.step(a)
        self.ro.push()
        return self.record(self.b.done.clone())

    def update(self):
        assert self.ro.step == self.T
        self.ro.after_update()
        self.windows += 1
        self.snap = {0: self.snap[self.T]}
        assert self.ro.step == 0
        self.seen["ages_after_update"] |= set(self.ro.ages[0].cpu().numpy().tolist())

    def check_all(self, tag, dtypes):
        torch = self.torch
        for t in range(self.ro.step + 1):
            for dt in dtypes:
                got = self.ro.obs(t, dtype=dt)
                assert got.dtype == dt and got.shape == self.snap[t].shape, (tag, t, got.shape)
                assert torch.equal(got, self.snap[t].to(dt)), (tag, "t", t, str(dt), int((got != self.snap[t].to(dt)).sum()))


# ------------------------------------------------------------------------------------- 4. every stored step equals the frame stack
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("nstack", [1, 4])
@pytest.mark.parametrize("size", [(80, 60), (10, 6)])   # W*H % 16 == 0: 16-byte units; 60 pixels: the 4-byte path
@pytest.mark.parametrize("form", ["rgb", "grey"])
def test_every_stored_step_equals_the_frame_stack(form, size, nstack, T):
    import torch
    grey = form == "grey"
    b = make("MiniWorld-Hallway-v0", obs_width=size[0], obs_height=size[1], max_episode_steps=EPISODE, greyscale=grey)
    d = Driver(b, T, nstack, grey=grey)
    dtypes = [torch.float32] if grey else [torch.float32, torch.uint8]
    assert d.ro.nstack == nstack and d.ro.num_steps == T and d.ro.grey == grey
    frame_bytes = size[0] * size[1] * (4 if grey else 3)
    assert d.ro.nbytes == (T + nstack) * N * frame_bytes + (T + 1) * N * (1 + 4 + 8) + T * N * 4
    rng = np.random.default_rng(7)
    windows = max(3, -(-nstack // T) + 1)
    d.reset()
    d.check_all((form, size, nstack, T, "reset"), dtypes)
    for w in range(windows):
        for _ in range(T):
            t = d.step(actions(rng))
            d.check_all((form, size, nstack, T, w, t), dtypes)   # older entries survive later writes into the ring
        d.update()
        d.check_all((form, size, nstack, T, w, "after_update"), dtypes)
    assert d.seen["done_t1"] and d.seen["done_tT"], d.seen
    assert d.seen["ages_after_update"] == set(range(nstack)), d.seen
    if nstack > 1:
        assert d.seen["prev_window"], d.seen
    b.close()


# ------------------------------------------------------------------------------------- 5. / 6. arbitrary index lists
@pytest.fixture(scope="module")
def pushed():
    """a Hallway batch with nstack 4, T = 8, one window behind it and the cursor at 5"""
    b = make("MiniWorld-Hallway-v0", max_episode_steps=EPISODE)
    d = Driver(b, 8, 4)
    rng = np.random.default_rng(11)
    d.reset()
    for _ in range(8):
        d.step(actions(rng))
    d.update()
    for _ in range(5):
        d.step(actions(rng))
    yield d
    b.close()


def want_rows(d, idx, dtype):
    import torch
    return torch.stack([d.snap[int(i) // N][int(i) % N] for i in idx]).to(dtype)


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_gather_with_an_arbitrary_index_list(pushed, dtype):
    import torch
    from gym_miniworld_amd import _lib
    d, b = pushed, pushed.b
    dt = getattr(torch, dtype)
    rng = np.random.default_rng(13)
    total = (d.ro.step + 1) * N
    idx = np.concatenate([rng.permutation(total)[:29], rng.integers(0, total, 8)])   # B = 37, duplicates, any order
    idx[3] = idx[30]
    rng.shuffle(idx)
    dev_idx = torch.from_numpy(idx).to(b.device)
    got = d.ro.gather(dev_idx, dtype=dt)
    assert got.shape == (37, 12, 80, 60)
    assert torch.equal(got, want_rows(d, idx, dt))
    assert torch.equal(d.ro.gather(idx.tolist(), dtype=dt), got)   # a host list: checked on the host, then the same gather
    # through the C ABI into the middle of a larger buffer: the rows before and after keep their canary
    canary = 171
    big = torch.full((39, 12, 80, 60), canary, dtype=dt, device=b.device)
    _lib.check(b.L.mwb_rollout_gather(b.h, ctypes.c_void_p(dev_idx.data_ptr()), 37, ctypes.c_void_p(big[1].data_ptr()), int(dtype == "float32"),
                                      b._stream()))
    assert torch.equal(big[1:38], got) and bool((big[0] == canary).all()) and bool((big[38] == canary).all())
    # count == 0 is a no-op
    _lib.check(b.L.mwb_rollout_gather(b.h, None, 0, None, 1, b._stream()))
    assert d.ro.gather(torch.zeros(0, dtype=torch.int64, device=b.device)).shape == (0, 12, 80, 60)
    assert d.ro.rejected() == 0
    with pytest.raises(ValueError):
        d.ro.gather([0, total])   # a host list is refused before anything is launched
    assert d.ro.rejected() == 0


def test_rejected_rows(pushed):
    import torch
    d, b = pushed, pushed.b
    total = (d.ro.step + 1) * N
    idx = np.array([5, -1, total - 1, total, 0, 2 ** 40, 17, 5], np.int64)
    bad = np.array([1, 3, 5])
    assert d.ro.rejected() == 0
    got = d.ro.gather(torch.from_numpy(idx).to(b.device))
    assert d.ro.rejected() == 3 and d.ro.rejected() == 0
    assert not got[bad].any()
    good = np.setdiff1d(np.arange(len(idx)), bad)
    assert torch.equal(got[good], want_rows(d, idx[good], torch.float32))
    assert got[good].any()


# ------------------------------------------------------------------------------------- 7. the small arrays
def test_rewards_masks_and_features_rows():
    import torch
    T = 4
    b = make("MiniWorld-TMazeTwoBoxDynamicFeaturesDebug-v0", max_episode_steps=EPISODE)
    ro = b.rollout_enable(num_steps=T, nstack=4)
    assert ro.rewards.shape == (T, N) and ro.masks.shape == (T + 1, N) and ro.features.shape == (T + 1, N, 2) and ro.ages.shape == (T + 1, N)
    rng = np.random.default_rng(17)
    b.reset()
    b.set_agent(0, step_count=(np.arange(N) % EPISODE).astype(np.int32))
    # env 0 one metre from its red box, env 1 one metre from its blue one, on the side of the stem: near() holds at their first step
    boxes = b.get_state(0, 2)["boxes_pos"]   # [env, box, xyz]
    spots = [[boxes[e, e, 0], boxes[e, e, 2] - np.sign(boxes[e, e, 2])] for e in range(2)]
    b.set_agent(0, pos_xz=np.array(spots), dir=np.zeros(2))
    ro.push(after_reset=True)
    assert bool((ro.masks[0] == 1).all()) and not ro.features[0].any() and not ro.ages[0].any()
    want_r, want_m, want_f = {}, {0: ro.masks[0].clone()}, {0: ro.features[0].clone()}
    some_feature = some_reward = some_done = 0
    for w in range(2):
        for t in range(1, T + 1):
            b.step(torch.from_numpy(rng.integers(0, 2, N).astype(np.int32)))   # turns only: nobody walks away from its box
            ro.push()
            want_r[t - 1], want_m[t], want_f[t] = b.reward.clone(), 1.0 - b.done.float(), b.feature.clone()
            some_feature += int(b.feature.any()); some_reward += int((b.reward != 0).any()); some_done += int(b.done.any())
            for k in range(t + 1):
                assert torch.equal(ro.masks[k], want_m[k]) and torch.equal(ro.features[k], want_f[k]), (w, t, k)
            for k in range(t):
                assert torch.equal(ro.rewards[k], want_r[k]), (w, t, k)
        if w == 0:
            ro.after_update()   # row T becomes row 0
            want_m, want_f, want_r = {0: want_m[T]}, {0: want_f[T]}, {}
            assert torch.equal(ro.masks[0], want_m[0]) and torch.equal(ro.features[0], want_f[0])
    assert some_feature and some_reward and some_done, (some_feature, some_reward, some_done, spots)
    b.close()


# ------------------------------------------------------------------------------------- 8. passes that are not steps
def test_passes_that_are_not_steps():
    import torch
    b = make("MiniWorld-Hallway-v0", max_episode_steps=EPISODE)
    d = Driver(b, 8, 4)
    dtypes = [torch.float32]
    rng = np.random.default_rng(19)
    d.reset()
    d.step(actions(rng))
    # a step with a skip mask: a skipped env is an env that is not done
    skip = torch.zeros(N, dtype=torch.uint8)
    skip[::3] = 1
    b.step(actions(rng), skip_mask=skip)
    d.ro.push()
    assert not b.done[::3].any() and bool((b.reward[::3] == -99).all())
    t = d.record(b.done.clone())
    assert bool((d.ro.rewards[t - 1][::3] == -99).all())
    d.check_all("skip", dtypes)
    # action repeat: one frame per call
    b.step_repeat(actions(rng), 3)
    d.ro.push()
    t = d.record(b.done.clone())
    assert t == 3 and torch.equal(d.ro.rewards[t - 1], b.reward)
    d.check_all("repeat", dtypes)
    # a partial reset is a step for the history: the masked envs start over, the others append their frame once more
    mask = torch.zeros(N, dtype=torch.uint8)
    mask[1::4] = 1
    b.reset(mask)
    d.ro.push(fresh=mask)
    t = d.ro.step
    d.snap[t] = d.ref.partial_reset(d.frame(), mask).clone()
    assert t == 4 and not d.ro.rewards[t - 1].any()
    assert torch.equal(d.ro.masks[t], 1.0 - mask.float().to(b.device)) and not d.ro.ages[t][1::4].any()
    d.check_all("partial reset", dtypes)
    d.step(actions(rng))
    d.check_all("step after", dtypes)
    b.close()


# ------------------------------------------------------------------------------------- 9. errors
def rollout_state(ro):
    info = ro._info()
    return (info.cursor, info.base, ro.ages.clone(), ro.masks.clone(), ro.rewards.clone(), ro.obs(ro.step) if info.cursor >= 0 else None)


def same_state(a, b):
    import torch
    return a[:2] == b[:2] and all(torch.equal(x, y) for x, y in zip(a[2:5], b[2:5])) and (a[5] is None or torch.equal(a[5], b[5]))


def expect(code, text, call):
    from gym_miniworld_amd import _lib
    with pytest.raises(_lib.MwbError) as ei:
        call()
    assert ("error %d:" % code) in str(ei.value) and text in str(ei.value), str(ei.value)


def no_rollout(b):
    from gym_miniworld_amd import _lib
    return b.L.mwb_rollout_info(b.h, ctypes.byref(_lib.MwbRolloutInfo())) == -4


def test_errors_leave_the_rollout_unchanged():
    import torch
    EINVAL, ESTATE = -1, -4
    b = make("MiniWorld-Hallway-v0", max_episode_steps=EPISODE)
    assert no_rollout(b)
    expect(ESTATE, "mwb_grey_enable", lambda: b.rollout_enable(2, 4, grey=True))   # grey without greyscale=True
    expect(EINVAL, "bad num_steps", lambda: b.rollout_enable(0, 4))
    expect(EINVAL, "bad num_steps", lambda: b.rollout_enable(2, 17))
    assert no_rollout(b)
    ro = b.rollout_enable(2, 4)
    expect(ESTATE, "already enabled", lambda: b.rollout_enable(2, 4))
    b.reset()
    expect(ESTATE, "after_reset", lambda: ro.push())   # a push before the reset push
    expect(ESTATE, "nothing has been pushed", lambda: ro.gather(torch.zeros(1, dtype=torch.int64, device=b.device)))
    assert ro.step == -1
    ro.push(after_reset=True)
    rng = np.random.default_rng(23)
    for _ in range(2):
        b.step(actions(rng))
        ro.push()
    before = rollout_state(ro)
    b.step(actions(rng))
    expect(ESTATE, "call mwb_rollout_after_update", lambda: ro.push())   # the cursor is at T
    assert same_state(before, rollout_state(ro))
    expect(ESTATE, "already enabled", lambda: b.rollout_enable(3, 2))
    assert same_state(before, rollout_state(ro))
    b.close()

    hwc = make("MiniWorld-Hallway-v0", layout="HWC")
    expect(EINVAL, "MWB_LAYOUT_CWH", lambda: hwc.rollout_enable(2, 4))
    assert no_rollout(hwc)
    hwc.close()

    tiny = make("MiniWorld-Hallway-v0", obs_width=3, obs_height=3)   # W*H = 9
    expect(EINVAL, "multiple of 4", lambda: tiny.rollout_enable(2, 4))
    assert no_rollout(tiny)
    tiny.close()

    g = make("MiniWorld-Hallway-v0", greyscale=True, max_episode_steps=EPISODE)
    gro = g.rollout_enable(2, 4, grey=True)
    g.reset()
    gro.push(after_reset=True)
    before = rollout_state(gro)
    expect(EINVAL, "float32", lambda: gro.obs(0, dtype=torch.uint8))   # uint8 gather from a grey ring
    assert same_state(before, rollout_state(gro))
    g.close()


# ------------------------------------------------------------------------------------- 10. nothing else changes
def test_a_rollout_changes_nothing_else():
    import torch
    a = make("MiniWorld-MazeS3-v0", seed=29, max_episode_steps=EPISODE)
    b = make("MiniWorld-MazeS3-v0", seed=29, max_episode_steps=EPISODE)
    ro = b.rollout_enable(8, 4)
    a.reset()
    b.reset()
    ro.push(after_reset=True)
    rng = np.random.default_rng(31)
    for t in range(20):
        act = actions(rng)
        a.step(act)
        b.step(act)
        if ro.full:
            ro.after_update()
        ro.push()
        assert torch.equal(a.obs, b.obs) and torch.equal(a.reward64, b.reward64) and torch.equal(a.done, b.done), t
    sa, sb = a.get_state(rng_state=True), b.get_state(rng_state=True)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    a.close()
    b.close()


# ------------------------------------------------------------------------------------- 11. VecEnv
@pytest.mark.parametrize("greyscale", [False, True])
def test_vec_env_rollout(greyscale):
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.vec_env import make_vec_envs
    T = 5
    envs = make_vec_envs("MiniWorld-Hallway-v0", seed=1, num_processes=N, device="cuda:0", rollout_steps=T, max_episode_steps=4, greyscale=greyscale)
    ro = envs.rollout
    assert ro is envs.batch.rollout and ro.num_steps == T and ro.nstack == 4 and ro.grey == greyscale
    rng = np.random.default_rng(37)
    returned = {0: envs.reset().clone()}
    assert returned[0].shape == (N, 4 if greyscale else 12, 80, 60)
    ended = 0
    for w in range(2):
        for t in range(1, T + 1):
            obs, rew, done, infos = envs.step(torch.from_numpy(rng.integers(0, 3, (N, 1))).to(envs.device))
            returned[t] = obs.clone()
            ended += int(done.sum())
            assert ro.step == t
            for k in range(t + 1):
                assert torch.equal(ro.obs(k), returned[k]), (greyscale, w, t, k)
            assert torch.equal(ro.rewards[t - 1].cpu(), rew.reshape(-1)) and torch.equal(ro.masks[t].cpu(), 1.0 - torch.from_numpy(done).float())
        if w == 0:
            # a full rollout: step() raises the library's message and nothing is stepped
            state = envs.batch.get_state()
            with pytest.raises(_lib.MwbError, match="mwb_rollout_after_update"):
                envs.step(torch.zeros((N, 1), dtype=torch.int64, device=envs.device))
            again = envs.batch.get_state()
            assert all(np.array_equal(state[k], again[k]) for k in state) and ro.step == T
            ro.after_update()
            returned = {0: returned[T]}
            assert torch.equal(ro.obs(0), returned[0])
    assert ended > 0
    envs.close()


def test_vec_env_rollout_refuses_a_captured_graph():
    from gym_miniworld_amd.vec_env import make_vec_envs
    with pytest.raises(ValueError, match="graph=True"):
        make_vec_envs("MiniWorld-Hallway-v0", seed=1, num_processes=N, device="cuda:0", rollout_steps=5, graph=True)


# ------------------------------------------------------------------------------------- 12. a ring past 4 GiB
def test_ring_past_4_gib():
    """Maze, 8192 envs, T = 36, nstack 4: 40 slots of 118 MB = 4.7 GB.  With base = 0 the slot of time 36 straddles 4 GiB (envs
    from 3350 on lie past it); in the second window times 1 .. 3 live in slots 37 .. 39."""
    import torch
    n, T, nstack = 8192, 36, 4
    if torch.cuda.mem_get_info()[1] < 64 * 2 ** 30:
        pytest.skip("needs a device of at least 64 GB")
    b = make("MiniWorld-Maze-v0", n=n, seed=41)
    ro = b.rollout_enable(num_steps=T, nstack=nstack)
    ring = (T + nstack) * n * 80 * 60 * 3
    assert ring > 2 ** 32 + 2 ** 28 and ro.nbytes > ring
    assert T * n * 14400 < 2 ** 32 < (T + 1) * n * 14400
    ref = FrameStackRef(n, nstack, (3, 80, 60), dtype=torch.uint8, device=b.device)   # 472 MB
    rng = np.random.default_rng(43)
    b.reset()
    ro.push(after_reset=True)
    ref.reset(b.obs)
    for w in range(2):
        for t in range(1, T + 1):
            b.step(actions(rng, n))
            ro.push()
            ref.step(b.obs, b.done)
            if t == T or (w == 1 and t in (1, 2, 3, 4)):
                assert ro.step == t and ro._info().base == (w * T) % (T + nstack)
                assert torch.equal(ro.obs(t, dtype=torch.uint8), ref.stacked), (w, t)
        if w == 0:
            ro.after_update()
            assert torch.equal(ro.obs(0, dtype=torch.uint8), ref.stacked)
    assert ro.rejected() == 0
    b.close()
    del ref
    torch.cuda.empty_cache()
