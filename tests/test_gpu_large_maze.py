"""GPU: mazes of more than 256 segments.  step_kernel's cull loop makes one trip per 32 segment groups, and the registered
8 x 8 Maze - 256 segments, 32 groups - is exactly one trip: in a larger maze the loop reloads its boxes (`c0 > 0`), passes its
second barrier and deals out groups of index 32 and more; reset_kernel<Maze> runs its depth-first search, cdf and seg_off in
LDS regions sized for up to 511 rooms; copy_seg_box_kernel moves more than 32 boxes; the serial wall tests and mwb_intersect
walk long lists; the render kernels hold a room table of 15 - 49 KB in LDS.

Sizes: 9 x 9 (324 segments, 41 groups: a second, partial trip), 16 x 16 (1024 segments, 128 groups: four full trips; the
oracle's largest, MWO_MAX_ROOMS 512) and 2 x 40 (320 segments, not square).  Everything against the oracle, whose own large
mazes tests/golden/state_MazeR9C9.npz and stepedge_MazeR*.npz pin to the reference."""
import numpy as np
import pytest

from test_gpu_parity import assert_state_equal, obs_diff, oracle_states
from test_gpu_seg_cull import forward_heavy, make_pair, run_pair

pytestmark = pytest.mark.gpu
ENV_ID = "MiniWorld-Maze-v0"
SIZES = [[9, 9, 3], [16, 16, 3], [2, 40, 3]]
IDS = ["9x9", "16x16", "2x40"]


def oracle_batch(O, args, n, seed, dr=False, mes=0):
    envs = [O.OracleEnv("Maze", seed=seed + i, domain_rand=dr, task_args=args, max_episode_steps=mes) for i in range(n)]
    for e in envs:
        e.reset(render=False)
    return envs


def n_segs_of(args):
    return 4 * args[0] * args[1]


@pytest.mark.parametrize("args", SIZES, ids=IDS)
def test_reset_state_geometry_and_rng_bit_exact(oracle_mod, args):
    """65 envs: a second, nearly empty block of the step launch; every env's world, placement and generator position after a
    first and after a second reset"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n = 65
    b = BatchedMiniWorld(ENV_ID, num_envs=n, seed=5100, task_args=args)
    b.reset()
    envs = oracle_batch(oracle_mod, args, n, 5100)
    for rnd in ("reset", "2nd reset"):
        st = b.get_state()
        assert_state_equal(st, oracle_states(envs), tag=(args, rnd))
        assert (st["n_segs"] == n_segs_of(args)).all() and (st["n_rooms"] == 2 * args[0] * args[1] - 1).all()
        for i in (0, 31, 63, 64):
            rooms, segs = b.get_geometry(i, max_segs=n_segs_of(args))
            g = envs[i].geometry()
            assert np.array_equal(segs, g["wall_segs"]), (args, rnd, i, "segs")
            o = g["outline"]
            rect = np.stack([o[:, :, 0].min(1), o[:, :, 0].max(1), o[:, :, 1].min(1), o[:, :, 1].max(1)], axis=1)
            assert np.array_equal(rooms[:, 0:4], rect.astype(np.float32)), (args, rnd, i, "rects")
        b.reset()
        for e in envs:
            e.reset(render=False)
    b.close()


@pytest.mark.parametrize("args,dr", [(SIZES[0], True), (SIZES[1], False), (SIZES[2], False)], ids=["9x9dr", "16x16", "2x40"])
def test_rollout_against_the_oracle(oracle_mod, args, dr):
    """150 forward-heavy steps of 16 envs, episodes of 40 steps so that every env regenerates its maze three times: pose, reward,
    done and ep_steps exact at every step, the whole state every 25"""
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n, mes = 16, 40
    b = BatchedMiniWorld(ENV_ID, num_envs=n, seed=5200, task_args=args, domain_rand=dr, max_episode_steps=mes)
    b.reset()
    envs = oracle_batch(oracle_mod, args, n, 5200, dr=dr, mes=mes)
    rng = np.random.default_rng(21)
    n_done = blocked = 0
    for t in range(150):
        a = forward_heavy(rng, n)
        before = b.get_state()["agent_pos"]
        b.step(torch.from_numpy(a))
        st = b.get_state()
        rew, done, eps = b.reward64.cpu().numpy(), b.done.cpu().numpy(), b.ep_steps.cpu().numpy()
        for i, e in enumerate(envs):
            _, r, d, _ = e.step(int(a[i]))
            s = e.state()
            assert r == rew[i] and d == bool(done[i]) and s.step_count == eps[i], (args, t, i)
            if d:
                e.reset(render=False)
                n_done += 1
                s = e.state()
            elif a[i] == 2:
                blocked += bool((st["agent_pos"][i] == before[i]).all())
            assert list(st["agent_pos"][i]) == list(s.agent_pos) and st["agent_dir"][i] == s.agent_dir, (args, t, i, "pose")
        if t % 25 == 24:
            assert_state_equal(st, oracle_states(envs), tag=(args, t))
    assert n_done >= 3 * n and blocked > n, (n_done, blocked)
    b.close()


@pytest.mark.parametrize("args", SIZES, ids=IDS)
def test_cull_on_equals_cull_off(args):
    n = 65
    a, b = make_pair(ENV_ID, n, seed=5300, task_args=args)
    a.reset(); b.reset()
    rng = np.random.default_rng(22)
    seen = dict(moved=0, blocked=0, carrying=0, done=0)
    run_pair(a, b, 200, lambda st: forward_heavy(rng, n), args, seen)
    assert seen["moved"] > 10 * n and seen["blocked"] > n, seen
    a.close(); b.close()


@pytest.mark.parametrize("args", SIZES[:2], ids=IDS[:2])
def test_boxes_follow_the_segments_through_partial_resets_and_copies(args):
    """as tests/test_gpu_seg_cull.py's test of the name, with 41 and 128 boxes an env: a masked reset, a snapshot, a clone inside
    the handle and the restore - after each, 50 steps agree with the twin on which every group passes"""
    import torch
    n = 65
    a, b = make_pair(ENV_ID, n, seed=5400, task_args=args, max_episode_steps=25)
    a.reset(); b.reset()
    rng = np.random.default_rng(23)
    policy = lambda st: forward_heavy(rng, n)   # noqa: E731
    seen = dict(moved=0, blocked=0, carrying=0, done=0)
    S = n_segs_of(args)
    geo = lambda h, i: h.get_geometry(i, max_segs=S)[1].copy()   # noqa: E731
    run_pair(a, b, 10, policy, "start", seen)
    segs0 = [geo(a, i) for i in range(n)]
    mask = torch.from_numpy((np.arange(n) % 3 == 0).astype(np.uint8))
    a.reset(mask); b.reset(mask)
    new = [not np.array_equal(geo(a, i), segs0[i]) for i in range(n)]
    assert sum(new[0::3]) > 15 and not any(new[1::3]) and not any(new[2::3]), new
    run_pair(a, b, 13, policy, "after the masked reset", seen)
    arch = [h.archive(n) for h in (a, b)]
    idx = np.arange(n, dtype=np.int32)
    for h, ar in zip((a, b), arch):
        h.save(ar, idx, idx)
    snap = [geo(a, i) for i in range(n)]
    run_pair(a, b, 50, policy, "after the snapshot", seen)
    assert 0 < seen["done"] and seen["blocked"] > n, seen
    for h in (a, b):   # clone: the upper half over the lower
        h.copy_envs(np.arange(0, 32, dtype=np.int32), np.arange(33, 65, dtype=np.int32))
    assert np.array_equal(geo(a, 5), geo(a, 38))
    run_pair(a, b, 50, policy, "after the clone", seen)
    assert sum(not np.array_equal(geo(a, i), snap[i]) for i in range(n)) > n // 2
    for h, ar in zip((a, b), arch):
        h.restore(ar, idx, idx)
    assert all(np.array_equal(geo(a, i), snap[i]) for i in range(n))
    run_pair(a, b, 50, policy, "after the restore", seen)
    for h in (a, b) + tuple(arch):
        h.close()


@pytest.mark.parametrize("args", SIZES, ids=IDS)
def test_frames_match_the_oracle(oracle_mod, args):
    """the first observation and ten step frames of four envs, within the suite's +-1 of the oracle's render_obs"""
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n = 4
    b = BatchedMiniWorld(ENV_ID, num_envs=n, seed=5500, task_args=args)
    obs = b.reset().cpu().numpy()
    envs = oracle_batch(oracle_mod, args, n, 5500)
    rng = np.random.default_rng(24)
    for t in range(11):
        for i, e in enumerate(envs):
            d = obs_diff(obs[i], e.render_obs())
            assert d.max() <= 1, (args, t, i, int(d.max()), int((d > 1).sum()))
        assert len(np.unique(obs.reshape(-1, 3), axis=0)) > 8
        a = forward_heavy(rng, n)
        obs = b.step(torch.from_numpy(a))[0].cpu().numpy()
        for i, e in enumerate(envs):
            if e.step(int(a[i]))[2]:
                e.reset(render=False)
    b.close()


def test_top_view_and_visible_ents_of_a_9x9_maze(oracle_mod):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n, args = 6, SIZES[0]
    b = BatchedMiniWorld(ENV_ID, num_envs=n, seed=5600, task_args=args)
    b.reset()
    envs = oracle_batch(oracle_mod, args, n, 5600)
    st = b.get_state()
    # turn every agent towards its box, step up to it where a wall does not hide it: some masks are then non-zero
    pos, bp = st["agent_pos"], st["boxes_pos"][:, 0]
    ang = np.arctan2(-(bp[:, 2] - pos[:, 2]), bp[:, 0] - pos[:, 0])
    b.set_state(0, agent_dir=ang)
    for i, e in enumerate(envs):
        e.set_agent(pos[i, 0], pos[i, 2], ang[i])
    got = b.visible_ents().cpu().numpy().astype(np.int64)
    assert np.array_equal(got, np.array([e.visible_ents() for e in envs], dtype=np.int64)), got
    top = b.render_top_view(160, 120).cpu().numpy()
    for i, e in enumerate(envs):
        d = obs_diff(top[i], e.render_top(160, 120))
        assert d.max() <= 1, (i, int(d.max()), int((d > 1).sum()))
    b.close()


@pytest.mark.parametrize("args", SIZES[:2], ids=IDS[:2])
def test_intersect_walks_the_whole_list(oracle_mod, args):
    """mwb_intersect (walls_hit_serial over every group) against the oracle at points beside the maze's LAST segments"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld(ENV_ID, num_envs=2, seed=5700, task_args=args)
    b.reset()
    e = oracle_batch(oracle_mod, args, 2, 5700)[1]
    segs = b.get_geometry(1, max_segs=n_segs_of(args))[1]
    hits = 0
    for j in list(range(len(segs) - 24, len(segs))) + [0, 255, 256, 257]:
        mid = 0.5 * (segs[j, :2] + segs[j, 2:])
        for off in ((0.39, 0.0), (0.0, 0.41), (-0.2, 0.3)):
            x, z = float(mid[0] + off[0]), float(mid[1] + off[1])
            got = b.intersect(1, x, z)
            assert got == e.intersect_agent(x, z), (args, j, off)
            hits += got == 1
    assert hits > 20
    b.close()
