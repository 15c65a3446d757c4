"""GPU: the episode monitor (mwb_monitor_*) against tests/monitor_ref.py, the plain-Python loop of the reference's trainer
(pytorch-a2c-ppo-acktr/main.py:167-169) with the return summed per episode.  The reference adds Python floats in step order and
the device adds float64 in the same order: every comparison of a return is bit equality, nothing here has a tolerance except the
mean of stats(), which torch sums in another order (bound stated there)."""
import math

import numpy as np
import pytest

from monitor_ref import MonitorRef, assert_equal

pytestmark = pytest.mark.gpu

W, H = 16, 12   # synthetic handles are never rendered: the smallest frames keep them cheap
REWARDS = np.array([-1.0, -0.25, 0.0, 0.0, 0.1, 0.2, 0.3, 1.0, 1e-3, 1.0 - 0.2 * (5 / 6)])   # 0.1 + 0.2 + 0.3 depends on the order


def synthetic(n, capacity, quota_max=0):
    """a handle that is never seeded, reset or rendered (the constructor archive() uses), its monitor and the reference"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld(num_envs=n, seed=None, _assets=False, obs_width=W, obs_height=H)
    return b, b.monitor_enable(capacity=capacity, quota_max=quota_max), MonitorRef(n, capacity, quota_max)


def random_pass(rng, n, p_done, p_skip=0.2):
    reward = np.where(rng.rand(n) < 0.7, REWARDS[rng.randint(0, len(REWARDS), n)], rng.standard_normal(n))
    done = (rng.rand(n) < p_done).astype(np.uint8)
    taken = rng.randint(0, 6, n).astype(np.int32)
    skip = (rng.rand(n) < p_skip).astype(np.uint8) if p_skip else None
    return reward, done, taken, skip


def both(mon, ref, reward, done, taken=None, skip=None):
    import torch
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    mon.update(skip_mask=t(skip), reward=t(reward), done=t(done), taken=t(taken))
    return ref.update(reward, done, taken, skip)


@pytest.mark.parametrize("capacity", [1, 7, 200])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 257])
def test_synthetic_passes_equal_the_loop(n, capacity):
    """12 passes at each of the done probabilities 0, 0.03, 0.5, 1 (with 1 every env that is not skipped finishes in one pass:
    c > capacity, only the last ranks are written), random skip masks, taken in 0 .. 5; everything equal after every pass"""
    b, mon, ref = synthetic(n, capacity, quota_max=3)
    rng = np.random.RandomState(1000 * n + capacity)
    most = 0
    for p_done in (0.0, 0.03, 0.5, 1.0):
        for k in range(12):
            reward, done, taken, skip = random_pass(rng, n, p_done, p_skip=0.0 if (p_done == 1.0 and k % 2) else 0.2)
            most = max(most, both(mon, ref, reward, done, taken, skip))
            assert_equal(mon, ref, (n, capacity, p_done, k))
    assert most == n and ref.total >= 6 * n
    assert n <= capacity or most > capacity   # the "last ranks only" rule was exercised wherever it can be
    b.close()


def test_synthetic_passes_70001_envs():
    """1094 waves: more waves than the scan's workgroup has lanes, more than 1024 wave counts"""
    n, capacity = 70001, 200
    b, mon, ref = synthetic(n, capacity, quota_max=1)
    rng = np.random.RandomState(7)
    for k, p_done in enumerate((0.0, 0.03, 0.5, 1.0) * 3):
        reward, done, taken, skip = random_pass(rng, n, p_done)
        both(mon, ref, reward, done, taken, skip)
        assert_equal(mon, ref, (n, k, p_done))
    assert ref.total > n
    b.close()


def test_partial_clear_drops_one_episode_and_plain_clear_restarts():
    n = 130
    b, mon, ref = synthetic(n, 7)
    rng = np.random.RandomState(3)
    for k in range(3):
        reward, done, taken, _ = random_pass(rng, n, 0.0, p_skip=0.0)
        both(mon, ref, reward, done, taken)
    mask = (rng.rand(n) < 0.3).astype(np.uint8)
    mask[[0, 64, 129]] = 1
    import torch
    mon.clear(torch.from_numpy(mask), partial=True)
    ref.clear(mask, partial=True)
    assert_equal(mon, ref, "flagged")
    assert (mon.partial.cpu().numpy() == mask).all() and float(mon.run_return[64]) == 0.0 and int(mon.run_len[64]) == 0
    ones = np.ones(n, np.uint8)
    reward = rng.standard_normal(n)
    assert both(mon, ref, reward, ones) == n - int(mask.sum())   # the flagged envs finish: dropped, not logged
    assert_equal(mon, ref, "dropped")
    assert mon.read()[1] == int(mask.sum()) and ref.dropped == int(mask.sum()) and not mon.partial.any()
    assert both(mon, ref, reward, ones) == n                     # their next episode is logged
    assert_equal(mon, ref, "next episode")
    # clear(mask): a fresh episode, nothing flagged, the others untouched
    both(mon, ref, reward, np.zeros(n, np.uint8))
    before = mon.run_return.clone()
    mon.clear(torch.from_numpy(mask))
    ref.clear(mask)
    assert_equal(mon, ref, "cleared")
    got = mon.run_return.cpu().numpy()
    assert (got[mask != 0] == 0.0).all() and np.array_equal(got[mask == 0], before.cpu().numpy()[mask == 0]) and not mon.partial.any()
    mon.clear()
    ref.clear()
    assert_equal(mon, ref, "cleared all")
    assert not mon.run_return.any() and not mon.run_len.any() and not mon.run_calls.any()
    b.close()


def test_quota_retires_at_exactly_the_second_episode():
    import torch
    n = 65
    b, mon, ref = synthetic(n, 200, quota_max=3)
    rng = np.random.RandomState(5)
    for k in range(4):   # something is running and logged before the quota is set: set_quota touches neither
        reward, done, taken, _ = random_pass(rng, n, 0.3, p_skip=0.0)
        both(mon, ref, reward, done, taken)
    run, total = mon.run_return.clone(), mon.read()[0]
    mon.set_quota(2)
    ref.set_quota(2)
    assert_equal(mon, ref, "quota set")
    assert torch.equal(mon.run_return, run) and mon.read() == (total, 0, n) and not mon.finished.any()
    assert torch.isnan(mon.tab_return).all() and (mon.tab_len == -1).all()
    for k in range(40):
        reward, done, taken, _ = random_pass(rng, n, 0.4, p_skip=0.0)
        skip = np.asarray(ref.retired, np.uint8)   # a retired env is named in the next skip mask
        was = np.asarray(ref.finished)
        both(mon, ref, reward, done, taken, skip)
        assert_equal(mon, ref, ("quota", k))
        fin, ret = mon.finished.cpu().numpy(), mon.retired.cpu().numpy() != 0
        assert fin.max() <= 2 and np.array_equal(ret, fin == 2)   # retirement at exactly the second episode, never a third
        assert np.array_equal(fin[skip != 0], was[skip != 0])
        if ref.remaining == 0:
            break
    assert ref.remaining == 0 and mon.read()[2] == 0
    assert not torch.isnan(mon.tab_return[:2]).any() and (mon.tab_len[:2] >= 0).all()
    assert torch.isnan(mon.tab_return[2]).all() and (mon.tab_len[2] == -1).all()
    # everyone is retired and skipped: a further pass changes nothing
    frozen = [t.clone() for t in (mon.run_return, mon.run_len, mon.run_calls, mon.finished, mon.tab_return, mon.tab_len)]
    both(mon, ref, np.ones(n), np.ones(n, np.uint8), None, np.ones(n, np.uint8))
    assert_equal(mon, ref, "frozen")
    for a, t in zip(frozen, (mon.run_return, mon.run_len, mon.run_calls, mon.finished, mon.tab_return, mon.tab_len)):
        assert torch.equal(a.view(torch.uint8), t.view(torch.uint8))
    b.close()


def test_refusals():
    import ctypes
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld(num_envs=5, seed=None, _assets=False, obs_width=W, obs_height=H)
    L = b.L
    assert L.mwb_monitor_update(b.h, None, None, None, None, None) == -4 and b"mwb_monitor_enable first" in L.mwb_last_error()   # MWB_ESTATE
    assert L.mwb_monitor_clear(b.h, None, 0, None) == -4 and L.mwb_monitor_quota(b.h, 0, None) == -4
    assert L.mwb_monitor_info(b.h, ctypes.byref(_lib.MwbMonitorInfo())) == -4 and L.mwb_monitor_read(b.h, ctypes.byref(_lib.MwbMonitorCounts())) == -4
    for capacity, quota_max in ((0, 0), (-1, 0), (65537, 0), (10, -1), (10, 65)):
        with pytest.raises(_lib.MwbError, match="must lie in"):
            b.monitor_enable(capacity=capacity, quota_max=quota_max)
    assert b.monitor is None
    mon = b.monitor_enable(capacity=65536, quota_max=2)
    with pytest.raises(_lib.MwbError, match="already enabled"):
        b.monitor_enable(capacity=10)
    assert b.monitor is mon
    assert L.mwb_monitor_quota(b.h, 3, None) == -1 and b"quota_max" in L.mwb_last_error()   # MWB_EINVAL
    for bad in (3, -1, True, 1.0):
        with pytest.raises(ValueError, match="quota"):
            mon.set_quota(bad)
    mon.set_quota(2)
    with pytest.raises(ValueError, match="entries for 5 envs"):
        mon.update(reward=np.zeros(4))
    assert mon.read() == (0, 0, 5) and mon.stats() == dict(n=0, mean=None, median=None, min=None, max=None, success_rate=None, mean_len=None)
    b.close()
    c = BatchedMiniWorld(num_envs=5, seed=None, _assets=False, obs_width=W, obs_height=H, auto_reset=False)
    with pytest.raises(_lib.MwbError, match="no_auto_reset"):
        c.monitor_enable()
    c.close()


# ------------------------------------------------------------------------------------------ real envs
def drive(env_id, mode, seed):
    """130 envs, max_episode_steps = 6, 40 steps of seeded random actions; the reference is fed with the step's own reward64 /
    done / taken read back.  Returns (most episodes one pass finished, some return differed from its episode's last reward)."""
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n, capacity = 130, 50
    b = BatchedMiniWorld(env_id, num_envs=n, seed=seed, max_episode_steps=6, obs_width=W, obs_height=H)
    mon, ref = b.monitor_enable(capacity=capacity), MonitorRef(n, capacity)
    b.reset()
    g = torch.Generator().manual_seed(seed)
    most, summed = 0, False
    for t in range(40):
        acts = torch.randint(0, b.n_actions, (n,), generator=g, dtype=torch.int32)
        skip = (torch.rand(n, generator=g) < 0.3).to(torch.uint8) if (mode == "skip" and t % 3 == 2) else None
        if mode == "repeat":
            b.step_repeat(acts, 3, skip_mask=skip)
        else:
            b.step(acts, skip_mask=skip)
        mon.update(skip_mask=skip)   # the NULL form: the handle's own buffers
        reward, done = b.reward64.cpu().numpy(), b.done.cpu().numpy()
        taken = b.taken.cpu().numpy() if mode == "repeat" else None
        most = max(most, ref.update(reward, done, taken, None if skip is None else skip.numpy()))
        assert_equal(mon, ref, (env_id, mode, t))
        summed = summed or any(ref.logged[e] and ref.last_return[e] != reward[e] for e in range(n))
        if skip is not None:
            assert (reward[skip.numpy() != 0] == -99.0).all()   # ... and no return has seen it
    assert all(abs(r) < 50 for r, _, _, _ in ref.log) and ref.total >= 5 * n
    if mode == "repeat":
        assert max(w[1] for w in ref.log) > max(w[2] for w in ref.log)   # lengths count sub-steps, calls count calls
    b.close()
    return most, summed


@pytest.mark.parametrize("mode", ["step", "repeat", "skip"])
def test_real_envs_wiring(mode):
    results = [drive(env_id, mode, seed) for env_id, seed in (("MiniWorld-Hallway-v0", 11), ("MiniWorld-PickupObjs-v0", 12))]
    print("monitor wiring", mode, results)
    assert max(m for m, _ in results) > 50      # a pass finished more episodes than the ring holds
    assert any(s for _, s in results)           # a return that is not its episode's last reward: what the old loop gets wrong


def test_reset_mask_and_copy_envs():
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n = 130
    b = BatchedMiniWorld("MiniWorld-Hallway-v0", num_envs=n, seed=21, max_episode_steps=50, obs_width=W, obs_height=H)
    mon = b.monitor_enable(capacity=50)
    b.reset()
    g = torch.Generator().manual_seed(21)
    for t in range(3):
        b.step(torch.randint(0, b.n_actions, (n,), generator=g, dtype=torch.int32))
        mon.update()
    assert (mon.run_calls == 3).all()
    mask = torch.rand(n, generator=g) < 0.4
    mask[0], mask[1] = True, False
    b.reset(mask.to(b.device))
    m = mask.numpy()
    calls, lens, part = mon.run_calls.cpu().numpy(), mon.run_len.cpu().numpy(), mon.partial.cpu().numpy()
    assert (calls[m] == 0).all() and (lens[m] == 0).all() and (mon.run_return.cpu().numpy()[m] == 0.0).all() and not part.any()
    assert (calls[~m] == 3).all() and (lens[~m] == 3).all()
    # copy_envs: the destinations are in the middle of an episode whose start was not seen
    dst, src = [5, 64, 129], [1, 1, 2]
    b.copy_envs(dst, src)
    part = mon.partial.cpu().numpy()
    assert part[dst].all() and part.sum() == 3 and (mon.run_calls.cpu().numpy()[dst] == 0).all()
    b.copy_envs(torch.tensor([7], device=b.device), torch.tensor([1], device=b.device))   # index lists on the device
    assert mon.partial.cpu().numpy().sum() == 4 and int(mon.partial[7]) == 1
    b.reset()
    assert not mon.partial.any() and not mon.run_calls.any()
    b.close()


def test_vecenv_infos_and_stats():
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    n, K = 65, 20
    envs = MiniWorldVecEnv("MiniWorld-TMaze-v0", n, monitor=K, frame_skip=2, max_episode_steps=5)
    assert envs.monitor is envs.batch.monitor and envs.monitor.capacity == K
    ref = MonitorRef(n, K)
    envs.reset()
    g = torch.Generator().manual_seed(31)
    seen = 0
    for t in range(12):
        _, _, dones, infos = envs.step(torch.randint(0, 3, (n, 1), generator=g))
        ref.update(envs.batch.reward64.cpu().numpy(), dones, infos.taken)
        for i in range(n):
            assert ("episode" in infos[i]) == bool(dones[i]), (t, i)
            if dones[i]:
                ep = infos[i]["episode"]
                assert ep["r"] == ref.last_return[i] and ep["l"] == ref.last_len[i] and ep["t"] >= 0.0, (t, i)
                assert isinstance(ep["r"], float) and isinstance(ep["l"], int)
                seen += 1
        assert np.array_equal(infos.episode_logged, dones)
        assert_equal(envs.monitor, ref, t)
    assert seen == ref.total >= 3 * n and max(ref.last_len) == 5 and max(w[2] for w in ref.log) == 3   # 5 env steps are 3 calls of 2
    st = envs.monitor.stats()
    r = np.array([w[0] for w in ref.log])
    assert st["n"] == len(r) == K and st["min"] == r.min() and st["max"] == r.max() and st["median"] == float(np.median(r))
    assert st["success_rate"] == np.count_nonzero(np.greater(r, 0)) / len(r)   # main.py:214
    # torch sums in another order than math.fsum: the bound of a float64 sum of n terms
    assert abs(st["mean"] - math.fsum(r) / len(r)) <= len(r) * 2.0 ** -52 * np.abs(r).max()
    assert st["mean_len"] == sum(w[1] for w in ref.log) / K
    envs.close()


def seeded_policy(n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return lambda obs: torch.randint(0, 3, (n, 1), generator=g)


def test_evaluate_is_per_env_not_first_k():
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv, evaluate
    n, q, seed = 65, 2, 41
    envs = MiniWorldVecEnv("MiniWorld-MazeS3-v0", n, seed=seed, monitor=200)
    ref = MonitorRef(n, 200, envs.monitor.quota_max)
    ref.set_quota(q)
    policy = seeded_policy(n, seed)
    calls = [0]

    def feed():   # the step that has just been made, with the mask evaluate() must have given it
        skip = np.asarray(ref.retired, np.uint8)
        ref.update(envs.batch.reward64.cpu().numpy(), envs.batch.done.cpu().numpy(), None, skip)

    def act(obs):
        if calls[0]:
            feed()
        calls[0] += 1
        return policy(obs)
    ret, ln = evaluate(envs, act, episodes_per_env=q)   # the loop ends
    feed()
    assert ret.shape == (q, n) and ln.shape == (q, n) and ret.dtype == torch.float64 and ln.dtype == torch.int32
    assert ref.remaining == 0 and envs.monitor_remaining == 0 and envs.monitor.read() == (q * n, 0, 0)
    assert_equal(envs.monitor, ref, "evaluate")
    assert not torch.isnan(ret).any() and (ln > 0).all() and (envs.monitor.finished == q).all()   # exactly two entries per env
    assert np.array_equal(ret.cpu().numpy(), np.array(ref.tab_return[:q])) and np.array_equal(ln.cpu().numpy(), np.array(ref.tab_len[:q]))
    table = sorted(zip(ret.cpu().numpy().reshape(-1).tolist(), ln.cpu().numpy().reshape(-1).tolist()))
    envs.close()
    # the point of it: the same envs under the same policy without retirement - the first 2 * 65 episodes to finish
    envs = MiniWorldVecEnv("MiniWorld-MazeS3-v0", n, seed=seed, monitor=200)
    policy = seeded_policy(n, seed)
    obs = envs.reset()
    while envs.monitor.read()[0] < q * n:   # (at most 129 + 65 episodes: the ring of 200 still holds the first 130)
        obs = envs.step(policy(obs))[0]
    r, l, _, _ = envs.monitor.log()
    first = sorted(zip(r.cpu().numpy().tolist()[:q * n], l.cpu().numpy().tolist()[:q * n]))
    print("evaluate: mean return per env %.4f, first-K %.4f; success %d vs %d of %d" % (
        sum(x for x, _ in table) / len(table), sum(x for x, _ in first) / len(first), sum(x > 0 for x, _ in table), sum(x > 0 for x, _ in first), q * n))
    assert len(first) == q * n and first != table
    envs.close()


def test_vecenv_graph_replay_equals_eager_steps_with_a_monitor():
    """MiniWorldVecEnv(graph=True, monitor=K): the update is part of the captured step; log and per-env arrays equal the eager path's"""
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    n = 64
    a = MiniWorldVecEnv("MiniWorld-FourRooms-v0", n, seed=9, to_float=False, graph=True, monitor=20, max_episode_steps=3)
    b = MiniWorldVecEnv("MiniWorld-FourRooms-v0", n, seed=9, to_float=False, graph=False, monitor=20, max_episode_steps=3)
    assert torch.equal(a.reset(), b.reset())
    g = torch.Generator().manual_seed(1)
    for t in range(8):
        act = torch.randint(0, 3, (n, 1), generator=g)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, ib = b.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and np.array_equal(da, db), t
        assert np.array_equal(ia.episode_logged, ib.episode_logged) and np.array_equal(ia.episode_r, ib.episode_r), t
        ma, mb = a.monitor, b.monitor
        assert ma.read() == mb.read(), t
        for name in ("run_return", "run_len", "run_calls", "last_return", "last_len", "last_calls", "finished", "retired", "partial", "logged"):
            assert torch.equal(getattr(ma, name), getattr(mb, name)), (t, name)
        for x, y in zip(ma.log(), mb.log()):
            assert torch.equal(x, y), t
    assert a._graph is not None and b._graph is None and a.monitor.read()[0] >= 2 * n
    a.close(); b.close()
