"""GPU: the rollout's learner half (mwb_rollout_learner_enable / Rollout(learner=True) / MiniWorldVecEnv(rollout_learner=True)).

The yardstick of the scan is tests/returns_ref.py, a NumPy float32 restatement of the specification that tests/test_returns_host.py
ties to torch's own arithmetic and to csrc/mwb_returns_scan.h on the CPU; everything here is compared bit for bit (float32 viewed
as int32).  The data of the synthetic cases is that of the host test (returns_ref.random_case): magnitudes in [2^-10, 2^10] or
exactly 0, so that no intermediate can be subnormal."""
import ctypes

import numpy as np
import pytest

import returns_ref as R

pytestmark = pytest.mark.gpu

GAMMA, TAU = 0.99, 0.95


def make(env_id, n, seed=3, **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    kw.setdefault("layout", "CWH")
    kw.setdefault("obs_width", 10)
    kw.setdefault("obs_height", 6)
    return BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)


def bit_equal(torch, got, want):
    want = torch.from_numpy(np.ascontiguousarray(want, np.float32)).to(got.device)
    return got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32))


def full_rollout(b, T, **kw):
    """a rollout with its learner half, stepped to the cursor T"""
    import torch
    ro = b.rollout_enable(num_steps=T, nstack=1, learner=True, **kw)
    b.reset()
    ro.push(after_reset=True)
    for _ in range(T):
        b.step(torch.full((b.num_envs,), 2, dtype=torch.int32))
        ro.push()
    assert ro.step == T
    return ro


def fill(torch, ro, c):
    dev = ro.batch.device
    for view, key in ((ro.rewards, "reward"), (ro.masks, "mask"), (ro.value_preds, "value"), (ro.taken, "taken"), (ro.features, "feature")):
        view.copy_(torch.from_numpy(c[key]).to(dev))


def arrays(ro):
    """every array of the rollout and its learner half, and its position"""
    info = ro._info()
    out = {"cursor": info.cursor, "base": info.base}
    for name in ("rewards", "masks", "features", "ages"):
        out[name] = getattr(ro, name).clone()
    if ro.learner:
        for name in ("actions", "action_log_probs", "value_preds", "taken", "returns", "advantages", "psi_returns"):
            out[name] = getattr(ro, name).clone()
    if info.cursor >= 0:
        out["obs"] = ro.obs(ro.step)
    return out


def same(torch, a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)


# ------------------------------------------------------------------------------------- 1. the scan, synthetic columns
@pytest.mark.parametrize("T", [1, 2, 9, 17])      # remainders of every unroll factor up to 16
@pytest.mark.parametrize("N", [1, 67, 300])       # a single lane; a partial wave; several workgroups, the last one partial
def test_scan_equals_the_restatement_bit_for_bit(N, T):
    import torch
    b = make("MiniWorld-Hallway-v0", N)
    ro = full_rollout(b, T)
    assert ro.returns.shape == (T + 1, N) and ro.advantages.shape == (T, N) and ro.psi_returns.shape == (T + 1, N, 2)
    assert ro.taken.dtype == torch.int32 and bool((ro.taken == 1).all()) and not ro.returns.any() and not ro.value_preds.any()
    c = R.random_case(T, N, seed=100 * T + N)
    assert (c["mask"][T] == 0).any() and (c["mask"][1] == 0).any() and c["taken"].max() == R.MAX_K
    assert c["taken"].min() == 0 or T * N == 1
    dev = b.device
    nv, npsi, over = (torch.from_numpy(c[k]).to(dev) for k in ("next_value", "next_psi", "reward_override"))

    fill(torch, ro, c)
    ro.compute_returns(nv, True, GAMMA, TAU)
    ret, adv, value = R.gae(c["reward"], c["value"], c["mask"], c["taken"], c["next_value"], GAMMA, TAU)
    assert bit_equal(torch, ro.returns, ret) and bit_equal(torch, ro.advantages, adv) and bit_equal(torch, ro.value_preds, value), ("gae", N, T)
    assert not ro.psi_returns.any()

    fill(torch, ro, c)
    ro.compute_returns(nv.unsqueeze(1), False, GAMMA, TAU)
    ret, adv, value = R.discounted(c["reward"], c["value"], c["mask"], c["taken"], c["next_value"], GAMMA)
    assert bit_equal(torch, ro.returns, ret) and bit_equal(torch, ro.advantages, adv) and bit_equal(torch, ro.value_preds, value), ("discounted", N, T)

    fill(torch, ro, c)
    ro.compute_returns(nv, False, GAMMA, TAU, rewards=over.unsqueeze(2))   # the sf=True branch: estimated rewards
    ret2, adv2, _ = R.discounted(c["reward_override"], c["value"], c["mask"], c["taken"], c["next_value"], GAMMA)
    assert bit_equal(torch, ro.returns, ret2) and bit_equal(torch, ro.advantages, adv2), ("override", N, T)
    assert bit_equal(torch, ro.rewards, c["reward"])   # the stored rewards are read-only to the scan
    ro.compute_returns(nv, True, GAMMA, TAU, rewards=over)
    ret3, adv3, _ = R.gae(c["reward_override"], c["value"], c["mask"], c["taken"], c["next_value"], GAMMA, TAU)
    assert bit_equal(torch, ro.returns, ret3) and bit_equal(torch, ro.advantages, adv3), ("gae override", N, T)

    before = ro.returns.clone()
    ro.compute_psi_returns(npsi, GAMMA)
    assert bit_equal(torch, ro.psi_returns, R.psi(c["feature"], c["mask"], c["taken"], c["next_psi"], GAMMA)), ("psi", N, T)
    assert torch.equal(ro.returns, before)
    assert ro.rejected() == 0
    b.close()


# ------------------------------------------------------------------------------------- 2. end to end through the VecEnv
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_vec_env_records_taken_and_actions(dtype):
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    N, T, K = 67, 8, 4
    envs = MiniWorldVecEnv("MiniWorld-Hallway-v0", N, seed=1, max_episode_steps=3, frame_skip=K, rollout_steps=T, rollout_learner=True)
    ro = envs.rollout
    assert ro.learner and ro.num_steps == T
    rng = np.random.default_rng(11)
    envs.reset()
    given, values = [], []
    for t in range(1, T + 1):
        a = torch.from_numpy(rng.integers(0, 3, (N, 1))).to(getattr(torch, dtype)).to(envs.device)
        obs, rew, done, infos = envs.step(a)
        given.append(a.reshape(-1).to(torch.int64))
        assert ro.step == t
        assert np.array_equal(ro.taken[t - 1].cpu().numpy(), np.asarray(infos.taken)), t
        assert torch.equal(ro.rewards[t - 1].cpu(), rew.reshape(-1)) and torch.equal(ro.masks[t].cpu(), 1.0 - torch.from_numpy(done).float())
        v, lp = torch.randn(N, 1, device=envs.device), torch.randn(N, device=envs.device)
        ro.insert(value=v, log_prob=lp)   # the trainer's part: the actions are the view's
        values.append((v.reshape(-1).clone(), lp.clone()))
    assert torch.equal(ro.actions, torch.stack(given))
    assert torch.equal(ro.value_preds[:T], torch.stack([v for v, _ in values])) and torch.equal(ro.action_log_probs, torch.stack([lp for _, lp in values]))
    taken, masks = ro.taken.cpu().numpy(), ro.masks.cpu().numpy()
    assert (taken < K).any() and (taken >= 1).all() and (masks == 0).any()   # the paths this test is about
    nv = torch.randn(N, device=envs.device)
    for use_gae in (True, False):
        value = ro.value_preds.cpu().numpy()
        ro.compute_returns(nv, use_gae, GAMMA, TAU)
        if use_gae:
            ret, adv, value = R.gae(ro.rewards.cpu().numpy(), value, masks, taken, nv.cpu().numpy(), GAMMA, TAU)
        else:
            ret, adv, value = R.discounted(ro.rewards.cpu().numpy(), value, masks, taken, nv.cpu().numpy(), GAMMA)
        assert bit_equal(torch, ro.returns, ret) and bit_equal(torch, ro.advantages, adv) and bit_equal(torch, ro.value_preds, value), use_gae
    # the same handle stepped with plain step(): one sub-step per transition
    ro.after_update()
    envs.batch.step(torch.zeros(N, dtype=torch.int32))
    ro.push()
    assert bool((ro.taken[0] == 1).all())
    envs.batch.step_repeat(torch.zeros(N, dtype=torch.int32), 2)
    ro.push(fresh=torch.zeros(N, dtype=torch.uint8))   # given a fresh list, the pass counts as no step
    assert bool((ro.taken[1] == 1).all())
    envs.close()


# ------------------------------------------------------------------------------------- 3. insert
def test_insert_lands_in_the_row_of_the_last_transition():
    import torch
    N, T = 67, 3
    b = make("MiniWorld-Hallway-v0", N)
    ro = b.rollout_enable(num_steps=T, nstack=1)
    ro.learner_enable()
    dev = b.device
    b.reset()
    ro.push(after_reset=True)
    act = torch.arange(N, dtype=torch.int32)
    want_a, want_l, want_v = torch.zeros(T, N, dtype=torch.int64, device=dev), torch.zeros(T, N, device=dev), torch.zeros(T + 1, N, device=dev)
    for t in range(1, T + 1):
        b.step(act % 3)
        ro.push()
        a = (torch.arange(N, device=dev) * 7 + t).to(torch.int64 if t % 2 else torch.int32)
        lp, v = torch.randn(N, device=dev), torch.randn(N, 1, device=dev)
        ro.insert(value=v, log_prob=lp, action=a)
        want_a[t - 1], want_l[t - 1], want_v[t - 1] = a.to(torch.int64), lp, v.reshape(-1)
        assert torch.equal(ro.actions, want_a) and torch.equal(ro.action_log_probs, want_l) and torch.equal(ro.value_preds, want_v), t
    # None leaves a column as it is
    lp2 = torch.randn(N, device=dev)
    ro.insert(log_prob=lp2)
    want_l[T - 1] = lp2
    assert torch.equal(ro.actions, want_a) and torch.equal(ro.action_log_probs, want_l) and torch.equal(ro.value_preds, want_v)
    ro.insert()
    ro.insert(action=torch.full((N,), 5, dtype=torch.int64, device=dev))
    want_a[T - 1] = 5
    assert torch.equal(ro.actions, want_a) and torch.equal(ro.action_log_probs, want_l) and torch.equal(ro.value_preds, want_v)
    # after after_update the next insert lands in row 0
    ro.after_update()
    b.step(act % 3)
    ro.push()
    v = torch.randn(N, device=dev)
    ro.insert(value=v)
    want_v[0] = v
    assert torch.equal(ro.actions, want_a) and torch.equal(ro.action_log_probs, want_l) and torch.equal(ro.value_preds, want_v)
    b.close()


# ------------------------------------------------------------------------------------- 4. the column gather
def test_column_gather():
    import torch
    N, T = 67, 8
    b = make("MiniWorld-Hallway-v0", N)
    ro = full_rollout(b, T)
    dev = b.device
    c = R.random_case(T, N, seed=5)
    fill(torch, ro, c)
    ro.actions.copy_(torch.from_numpy(np.random.default_rng(6).integers(0, 2 ** 40, (T, N))).to(dev))
    ro.action_log_probs.copy_(torch.from_numpy(c["reward_override"]).to(dev))
    ro.compute_returns(torch.from_numpy(c["next_value"]).to(dev), True, GAMMA, TAU)
    idx = torch.arange(T * N - 1, -1, -3, device=dev)
    idx = torch.cat([idx, idx[:11]])   # descending, with repeats
    assert idx.numel() % 64 != 0 and idx.numel() > 64
    ext = torch.randn(T, N, device=dev)
    flat = lambda x: x.reshape(-1, *x.shape[2:])   # noqa: E731
    for adv_src in (None, ext):
        obs, act, ret, mask, logp, adv, val = ro.minibatch(idx, adv_src)
        assert act.shape == (idx.numel(), 1) and act.dtype == torch.int64 and all(x.shape == (idx.numel(), 1) for x in (ret, mask, logp, adv, val))
        assert torch.equal(obs, ro.gather(idx))
        assert torch.equal(act[:, 0], flat(ro.actions)[idx]) and torch.equal(ret[:, 0], flat(ro.returns[:-1])[idx])
        assert torch.equal(mask[:, 0], flat(ro.masks[:-1])[idx]) and torch.equal(logp[:, 0], flat(ro.action_log_probs)[idx])
        assert torch.equal(val[:, 0], flat(ro.value_preds[:-1])[idx])
        assert torch.equal(adv[:, 0], flat(ro.advantages if adv_src is None else ext)[idx])
    assert ro.rejected() == 0
    # rows out of range: zeros, counted - by the column gather alone (the C ABI: Rollout.minibatch would count them in gather() too)
    bad = torch.tensor([5, -1, T * N, 2 ** 40, T * N - 1], dtype=torch.int64, device=dev)
    cols = torch.full((5, 5), 7.0, device=dev)
    act = torch.full((5,), 7, dtype=torch.int64, device=dev)
    rc = b.L.mwb_rollout_gather_cols(b.h, ctypes.c_void_p(bad.data_ptr()), 5, None, ctypes.c_void_p(cols.data_ptr()), ctypes.c_void_p(act.data_ptr()), b._stream())
    assert rc == 0
    assert not cols[:, 1:4].any() and not act[1:4].any()
    assert torch.equal(cols[0, [0, 4]], flat(ro.returns)[bad[[0, 4]]]) and torch.equal(act[[0, 4]], flat(ro.actions)[bad[[0, 4]]])
    assert ro.rejected() == 3 and ro.rejected() == 0
    # count == 0 is a no-op; a host list is checked on the host
    assert b.L.mwb_rollout_gather_cols(b.h, None, 0, None, None, None, b._stream()) == 0
    with pytest.raises(ValueError, match=r"outside \[0, %d\)" % (T * N)):
        ro.minibatch([0, T * N])
    assert ro.rejected() == 0
    b.close()


# ------------------------------------------------------------------------------------- 5. the minibatch generator
def test_feed_forward_generator():
    import torch
    N, T, M = 67, 8, 5
    b = make("MiniWorld-Hallway-v0", N)
    ro = full_rollout(b, T)
    dev = b.device
    c = R.random_case(T, N, seed=9)
    fill(torch, ro, c)
    ro.actions.copy_(torch.arange(T * N, device=dev).reshape(T, N))
    ro.action_log_probs.copy_(torch.from_numpy(c["reward_override"]).to(dev))
    ro.compute_returns(torch.from_numpy(c["next_value"]).to(dev), True, GAMMA, TAU)
    adv = (ro.advantages - ro.advantages.mean()) / (ro.advantages.std() + 1e-5)   # ppo.py:34-35 stays with the caller
    flat = lambda x: x.reshape(-1, *x.shape[2:])   # noqa: E731
    gen = lambda: torch.Generator(device=dev).manual_seed(1234)   # noqa: E731
    first = list(ro.feed_forward_generator(adv, M, generator=gen()))
    size = T * N // M
    assert [x[0].shape[0] for x in first] == [size] * M + [T * N - size * M] and T * N - size * M > 0   # the last batch is shorter
    perm = torch.randperm(T * N, device=dev, generator=gen())
    # the actions are the flat indices: they recover every batch's index list
    idx_all = torch.cat([x[2][:, 0] for x in first])
    assert torch.equal(idx_all, perm) and torch.equal(torch.sort(idx_all).values, torch.arange(T * N, device=dev))
    second = list(ro.feed_forward_generator(adv, M, generator=gen()))
    at = 0
    for one, two in zip(first, second):
        obs, hidden, act, ret, mask, logp, adv_t = one
        idx = perm[at:at + obs.shape[0]]
        at += obs.shape[0]
        assert hidden is None and len(one) == 7
        assert all(torch.equal(x, y) for x, y in zip(one, two) if x is not None)   # the same seed, the same batches
        assert torch.equal(obs, ro.gather(idx)) and torch.equal(act[:, 0], flat(ro.actions)[idx])
        assert torch.equal(ret[:, 0], flat(ro.returns[:-1])[idx]) and torch.equal(mask[:, 0], flat(ro.masks[:-1])[idx])
        assert torch.equal(logp[:, 0], flat(ro.action_log_probs)[idx]) and torch.equal(adv_t[:, 0], flat(adv)[idx])
    with pytest.raises(AssertionError, match="PPO requires"):
        next(ro.feed_forward_generator(adv, T * N + 1))
    assert ro.rejected() == 0
    b.close()


# ------------------------------------------------------------------------------------- 6. refusals leave everything unchanged
def test_refusals_change_nothing():
    import torch
    from gym_miniworld_amd import _lib
    N, T = 67, 4
    b = make("MiniWorld-Hallway-v0", N)
    L, dev = b.L, b.device
    with pytest.raises(_lib.MwbError, match="mwb_rollout_enable first"):   # before the rollout exists
        _lib.check(L.mwb_rollout_learner_enable(b.h))
    ro = b.rollout_enable(num_steps=T, nstack=1)
    for call in (lambda: ro.insert(value=torch.zeros(N, device=dev)),
                 lambda: ro.compute_returns(torch.zeros(N, device=dev), True, GAMMA, TAU)):
        with pytest.raises(_lib.MwbError, match="mwb_rollout_learner_enable first"):
            call()
    ro.learner_enable()
    with pytest.raises(_lib.MwbError, match="already enabled"):
        ro.learner_enable()
    b.reset()
    ro.push(after_reset=True)
    ro.taken.copy_(torch.from_numpy(R.random_case(T, N, 1)["taken"]).to(dev))
    ro.value_preds.copy_(torch.randn(T + 1, N, device=dev))
    v, nv, npsi = torch.randn(N, device=dev), torch.randn(N, device=dev), torch.randn(N, 2, device=dev)
    a64, a32 = torch.ones(N, dtype=torch.int64, device=dev), torch.ones(N, dtype=torch.int32, device=dev)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731

    snap = arrays(ro)
    with pytest.raises(_lib.MwbError, match="no transition has been pushed"):   # cursor 0
        ro.insert(value=v)
    with pytest.raises(_lib.MwbError, match="num_steps steps yet"):
        ro.compute_returns(nv, True, GAMMA, TAU)
    assert same(torch, snap, arrays(ro))

    b.step(torch.zeros(N, dtype=torch.int32))
    ro.push()
    snap = arrays(ro)
    with pytest.raises(_lib.MwbError, match="num_steps steps yet"):   # cursor 1 of 4
        ro.compute_psi_returns(npsi, GAMMA)
    assert L.mwb_rollout_insert(b.h, ptr(a64), ptr(a32), None, ptr(v), b._stream()) != 0 and b"at most one" in L.mwb_last_error()
    for bad in (dict(value=torch.zeros(N + 1, device=dev)), dict(log_prob=torch.zeros(N - 1, device=dev)), dict(action=torch.zeros(2 * N, dtype=torch.int64, device=dev)),
                dict(value=torch.zeros(N, dtype=torch.float64, device=dev)), dict(action=torch.zeros(N, device=dev)), dict(value=torch.zeros(N)),
                dict(log_prob=np.zeros(N, np.float32))):
        with pytest.raises(ValueError, match="rollout insert"):
            ro.insert(**bad)
    assert same(torch, snap, arrays(ro))

    for _ in range(T - 1):
        b.step(torch.zeros(N, dtype=torch.int32))
        ro.push()
    snap = arrays(ro)
    assert snap["cursor"] == T
    rc = L.mwb_rollout_returns(b.h, _lib.RETURNS_PSI, GAMMA, TAU, ptr(nv), None, None, b._stream())   # PSI without next_psi
    assert rc != 0 and b"next_psi" in L.mwb_last_error()
    assert L.mwb_rollout_returns(b.h, _lib.RETURNS_GAE, GAMMA, TAU, None, ptr(npsi), None, b._stream()) != 0
    assert L.mwb_rollout_returns(b.h, 3, GAMMA, TAU, ptr(nv), ptr(npsi), None, b._stream()) != 0 and b"unknown mode" in L.mwb_last_error()
    assert L.mwb_rollout_gather_cols(b.h, None, -1, None, None, None, b._stream()) != 0
    with pytest.raises(ValueError, match="next_value"):
        ro.compute_returns(torch.zeros(N - 1, device=dev), True, GAMMA, TAU)
    with pytest.raises(ValueError, match="rewards"):
        ro.compute_returns(nv, True, GAMMA, TAU, rewards=torch.zeros(T + 1, N, device=dev))
    with pytest.raises(ValueError, match="next_psi"):
        ro.compute_psi_returns(nv, GAMMA)
    with pytest.raises(ValueError, match="advantages"):
        ro.minibatch(torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(T + 1, N, device=dev))
    with pytest.raises(ValueError, match="empty"):
        ro.minibatch([])
    assert same(torch, snap, arrays(ro)) and ro.rejected() == 0
    b.close()


# ------------------------------------------------------------------------------------- 7. nothing else changes
def test_the_learner_half_changes_nothing_else():
    import torch
    N, T, STEPS = 16, 8, 20
    pair = [make("MiniWorld-MazeS3-v0", N, seed=5, obs_width=80, obs_height=60) for _ in range(2)]
    ros = [pair[0].rollout_enable(num_steps=T, nstack=4, learner=True), pair[1].rollout_enable(num_steps=T, nstack=4)]
    dev = pair[0].device
    rng = np.random.default_rng(21)
    idx = torch.from_numpy(rng.integers(0, T * N, 40)).to(dev)
    for b, ro in zip(pair, ros):
        b.reset()
        ro.push(after_reset=True)
    assert torch.equal(pair[0].obs, pair[1].obs)
    for i in range(STEPS):
        a = torch.from_numpy(rng.integers(0, 3, N).astype(np.int32))
        for b, ro in zip(pair, ros):
            if ro.full:
                if ro.learner:   # used: returns, a minibatch
                    ro.compute_returns(torch.randn(N, device=dev), True, GAMMA, TAU)
                    ro.compute_psi_returns(torch.randn(N, 2, device=dev), GAMMA)
                    ro.minibatch(idx)
                ro.after_update()
            b.step(a)
            ro.push()
            if ro.learner:
                ro.insert(value=torch.randn(N, device=dev), log_prob=torch.randn(N, device=dev), action=a.to(dev))
        assert torch.equal(pair[0].obs, pair[1].obs) and torch.equal(pair[0].reward64, pair[1].reward64) and torch.equal(pair[0].done, pair[1].done), i
    assert ros[0].step == ros[1].step == STEPS - 2 * T
    s0, s1 = (b.get_state(rng_state=True) for b in pair)
    assert s0.keys() == s1.keys() and all(np.array_equal(s0[k], s1[k]) for k in s0)
    for name in ("ages", "masks", "rewards", "features"):
        assert torch.equal(getattr(ros[0], name), getattr(ros[1], name)), name
    rows = torch.arange((ros[0].step + 1) * N, device=dev)
    assert torch.equal(ros[0].gather(rows), ros[1].gather(rows))
    assert ros[0].rejected() == 0 and ros[1].rejected() == 0
    for b in pair:
        b.close()
