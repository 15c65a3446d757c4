"""GPU: crowded worlds and task arguments off the class defaults against the oracle (rows, seeds and step scripts:
tests/crowded_rows.py; that the rows are crowded: tests/test_oracle_crowded.py).  WorldGen::place_entity_ex over several twists of
the wave-shared generator with up to 20 entities in LDS, the CollectHealth respawn of the step kernel through tens of attempts, the
attempt cap and what every kernel does with an env whose generation failed.

Rows the reference does not finish and that are NOT run here (15 s - 20 s time-outs of the oracle on the CPU; only observed, not
proved, unless noted): Hallway [2.2] [2.5] (same argument as Hallway [2] below: every length under 2.8), OneRoom [2], PutNext [3.6],
PickupObjs [7, 20] [6, 20] [5, 20] [4, 12], RoomObjs [6] [5] [4.5]; OneRoom [2.1] beyond the seeds and scripts used here (proved for a
box at the centre, crowded_rows.py)."""
import ctypes

import numpy as np
import pytest

import crowded_rows as CR
from test_gpu_episode_boundaries import assert_frames, assert_full_state, assert_step_outputs
from test_gpu_levels import Follower
from test_gpu_putnext import assert_putnext_state_equal

pytestmark = pytest.mark.gpu

FRAME_ENVS_ENTS = (0, 5, 10, 15)   # last frames of the rollouts: the oracle renders a frame with 20 meshes in 0.2 s, so four of the 16


def make_batch(name, dr=0, mes=None, n=CR.N, seed="row", **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    env_id, _, args = CR.row(name)
    return BatchedMiniWorld(env_id, num_envs=n, seed=CR.seed_of(name) if seed == "row" else seed, domain_rand=dr, want_depth=True,
                            task_args=args, max_episode_steps=mes, **kw)


def reset_oracles(envs):
    for e in envs:
        e.reset(render=False)


def assert_state(b, envs, tag):
    assert_full_state(b, envs, tag)
    if b.task == "PutNext":
        assert_putnext_state_equal(b.get_state(), envs, tag)
    assert b.L.mwb_check(b.h) == 0, tag   # no cap where the reference finishes


def frame_envs(b):
    return [i for i in FRAME_ENVS_ENTS if i < b.num_envs] if b.ent_task else range(b.num_envs)


def assert_rooms(b, rooms, g, tag):
    """the rectangle room table of a box row against the oracle's rooms: rectangles, wall heights, texture ids"""
    o = g["outline"]
    rect = np.stack([o[:, :, 0].min(1), o[:, :, 0].max(1), o[:, :, 1].min(1), o[:, :, 1].max(1)], axis=1)
    assert rooms.shape[0] == len(rect) and np.array_equal(rooms[:, 0:4], rect.astype(np.float32)), (tag, "rects")
    assert np.array_equal(np.abs(rooms[:, 4]), g["wall_height"].astype(np.float32)), (tag, "heights")   # (negative: no ceiling)
    tex = rooms[:, 5].view(np.int32)
    assert np.array_equal(np.stack([tex & 255, (tex >> 8) & 255, (tex >> 16) & 255], axis=1), g["tex_ids"]), (tag, "tex ids")


# Sign forces domain randomisation off (sign.py:62-71): no dr 1 case
RESET_CASES = [(name, dr) for name in list(CR.CROWDED) + list(CR.PLAIN) for dr in (0, 1) if not (dr and "Sign" in name)]


@pytest.mark.parametrize("name,dr", RESET_CASES)
def test_reset_parity_and_first_frame(oracle_mod, name, dr):
    """three resets: the whole state bit for bit (poses, entity table and list order, generator position and key sum), rooms and
    segments of three envs; the first frame and depth at the project's bars (+-1 per channel, 1e-4 m)"""
    b = make_batch(name, dr)
    envs = CR.make_oracles(oracle_mod, name, dr=b.domain_rand)
    for k in range(CR.RESETS):
        b.reset()
        reset_oracles(envs)
        assert_state(b, envs, "%s dr%d reset %d" % (name, dr, k + 1))
        for i in (0, 7, CR.N - 1):
            rooms, segs = b.get_geometry(i)
            g = envs[i].geometry()
            assert np.array_equal(segs, g["wall_segs"]), (name, k, i, "segs")
            if not b.ent_task:   # the box rows: OneRoom, PutNext and the off-default Maze shapes
                assert_rooms(b, rooms, g, (name, dr, k, i))
            assert b.get_state()["n_rooms"][i] == envs[i].state().n_rooms
        if k == 0:
            assert_frames(b, envs, range(CR.N), None, "%s dr%d first frame" % (name, dr))
    b.close()


def run_rollout(name, b, envs, policy, steps, repeat=0, state_every=25):
    import torch
    b.reset()
    reset_oracles(envs)
    n_done = 0
    for t, a in CR.script(envs, policy, steps, b.n_actions):
        if repeat:
            b.step_repeat(torch.from_numpy(a), repeat)
            rew, done, sc, taken = CR.oracle_repeat_step(envs, a, repeat)
            assert np.array_equal(b.taken.cpu().numpy(), taken), (name, t, "taken")
        else:
            b.step(torch.from_numpy(a))
            rew, done, sc = np.zeros(len(envs)), np.zeros(len(envs), bool), np.zeros(len(envs), np.int32)
            for i, e in enumerate(envs):
                _, rew[i], done[i], _ = e.step(int(a[i]))
                sc[i] = e.state().step_count
                if done[i]:
                    e.reset(render=False)
        assert_step_outputs(b, rew, done, sc, "%s t=%d" % (name, t))
        n_done += int(done.sum())
        if t % state_every == state_every - 1 or t == steps - 1:
            assert_state(b, envs, "%s t=%d" % (name, t))
    assert_frames(b, envs, frame_envs(b), done, "%s last frame" % name)
    return n_done


@pytest.mark.parametrize("name", list(CR.ROLLOUTS))
def test_rollouts_with_auto_reset(oracle_mod, name):
    """short episodes: every env regenerates its crowded world several times; reward, done and step count at every step, the full
    state every 25 steps and at the end, the last frame"""
    policy, mes, steps, n = CR.ROLLOUTS[name]
    b = make_batch(name, 0, mes, n=n)
    envs = CR.make_oracles(oracle_mod, name, mes=mes, n=n)
    assert run_rollout(name, b, envs, policy, steps) >= 4 * n
    b.close()


@pytest.mark.parametrize("name", CR.ROUTE_ROWS)
def test_partial_reset(oracle_mod, name):
    import torch
    b = make_batch(name)
    envs = CR.make_oracles(oracle_mod, name)
    b.reset()
    reset_oracles(envs)
    mask = np.zeros(CR.N, bool)
    mask[[0, 3, 4, 9, 15]] = True
    before = b.get_state(rng_state=True)
    b.reset(torch.from_numpy(mask))
    reset_oracles([e for i, e in enumerate(envs) if mask[i]])
    assert_state(b, envs, name + " reset(mask)")
    after = b.get_state(rng_state=True)
    for k in before:
        assert np.array_equal(before[k][~mask], after[k][~mask]), k
    assert_frames(b, envs, [0, 1, 15], None, name + " reset(mask)")
    b.close()


@pytest.mark.parametrize("name", CR.ROUTE_ROWS)
def test_step_repeat(oracle_mod, name):
    repeat, mes, calls = CR.REPEAT_ROUTE
    b = make_batch(name, 0, mes)
    envs = CR.make_oracles(oracle_mod, name, mes=mes)
    assert run_rollout(name, b, envs, CR.ROLLOUTS[name][0], calls, repeat=repeat, state_every=5) >= 4 * CR.N
    b.close()


@pytest.mark.parametrize("name", CR.ROUTE_ROWS)
def test_regeneration_on_the_callers_stream(oracle_mod, name, monkeypatch):
    """MWB_NO_OVERLAP=1 (read at creation): the regenerated envs' chain runs on the caller's stream"""
    policy, mes, _, _ = CR.ROLLOUTS[name]
    monkeypatch.setenv("MWB_NO_OVERLAP", "1")
    b = make_batch(name, 0, mes)
    monkeypatch.delenv("MWB_NO_OVERLAP")
    envs = CR.make_oracles(oracle_mod, name, mes=mes)
    assert run_rollout(name, b, envs, policy, CR.NO_OVERLAP_STEPS) >= 2 * CR.N
    b.close()


@pytest.mark.parametrize("name", CR.ROUTE_ROWS)
def test_level_sets(oracle_mod, name):
    """three sequential levels (seeds: crowded_rows.LEVEL_ROUTE): every episode is the first episode of an oracle re-seeded with its
    level's seed (the Follower of test_gpu_levels.py)"""
    import torch
    start, levels, mes, steps = CR.LEVEL_ROUTE[name]
    b = make_batch(name, 0, mes, seed=None)
    lv = b.levels_enable(levels, start_level=start, mode="sequential")
    envs = CR.make_oracles(oracle_mod, name, mes=mes)
    f = Follower(lv, envs, CR.N)
    b.reset()
    f.reset()
    assert_state(b, envs, name + " levels reset")
    for t, a in CR.script(envs, CR.ROLLOUTS[name][0], steps, b.n_actions):
        b.step(torch.from_numpy(a))
        rew, done, sc = f.step(a)
        assert_step_outputs(b, rew, done, sc, "%s levels t=%d" % (name, t))
        f.finish(rew, done, sc)
        f.assert_views("%s levels t=%d" % (name, t))
        if done.any():
            assert_state(b, envs, "%s levels t=%d" % (name, t))
    assert (f.epno >= 3).all()
    b.close()


def device_n_rooms(b):
    """n_rooms through mwb_get_state (BatchedMiniWorld.get_state raises on a handle whose generation failed)"""
    from gym_miniworld_amd import _lib
    out = np.zeros(b.num_envs, np.int32)
    st = _lib.MwbState()
    st.n_rooms = out.ctypes.data_as(ctypes.c_void_p)
    assert b.L.mwb_get_state(b.h, 0, b.num_envs, ctypes.byref(st)) == 0
    return out


def test_generation_that_cannot_succeed_is_reported_not_looped(oracle_mod):
    """Hallway [2]: the room is [-1, 1] x [-2, 2] (hallway.py:27-30); the box fits (x in [-1 + r, 1 - r], r = 0.8 / sqrt(2)), but
    the agent is placed with max_x = room.max_x - 2 = -1 (hallway.py:39-42): x = low + (high - low) u with low = -1 + 0.4,
    high = -1 - 0.4 (miniworld.py:881-888, numpy's uniform), i.e. x = -0.6 - 0.8 u.  For every u in (0, 1) the point is less than the
    agent's radius 0.4 from the wall at x = -1 (or beyond it): intersect() or point_inside() rejects it.  Only u = 0 - two
    consecutive generator words below 32 and 64 - puts the agent exactly 0.4 from the wall, which `dist < radius` lets pass; the
    test checks on the host that no word below 64 occurs in the 700 000 words (100 000 attempts of three doubles and the draws
    before them) that the capped loop can read from the four seeds it uses.  The reference loops for ever; the device gives up after
    100 000 attempts and reports the env."""
    import time
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n, seed = 4, 9000
    for i in range(n):   # the proof's last step, for these seeds
        words = np.frombuffer(np.random.RandomState(np.array(oracle_mod.seed_to_mt_key(seed + i), np.uint32)).bytes(4 * 700000), np.uint32)
        assert words.min() >= 64, (seed + i, int(words.min()))
    b = BatchedMiniWorld("MiniWorld-Hallway-v0", num_envs=n, seed=seed, task_args=[2])
    t0 = time.perf_counter()
    b.reset()
    torch.cuda.synchronize()
    print("capped reset of %d envs: %.3f s" % (n, time.perf_counter() - t0))

    def assert_reported():
        rc = b.L.mwb_check(b.h)   # MWB_ESTATE = -4
        assert rc == -4 and b"world generation failed for env" in b.L.mwb_last_error(), rc
        with pytest.raises(_lib.MwbError, match="world generation failed"):
            b.check()
    assert_reported()
    assert (device_n_rooms(b) == -1).all()
    b.step(torch.full((n,), 2, dtype=torch.int32))
    b.render()
    torch.cuda.synchronize()
    assert_reported()
    b.close()
    # nothing leaked into the process: a good row on a fresh handle
    g = make_batch("OneRoom-2.2")
    envs = CR.make_oracles(oracle_mod, "OneRoom-2.2")
    g.reset()
    reset_oracles(envs)
    assert_state(g, envs, "after the failure")
    g.close()
