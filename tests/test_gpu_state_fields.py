"""GPU: mwb_get_state / mwb_set_state through the state-field table, and the one allocation list behind every feature.

tests/golden/hostapi_state_7580f56_<task>.npz hold get_state(rng_state=True) of three batches of N = 5 envs (seed 11, no domain
randomisation) after the 12 steps of ACTIONS, written by record() below on commit 7580f56 - the last one whose mwb_get_state
spelled every field out by hand.  The library must return the same arrays bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, SEED = 5, 11
ENV_IDS = {"PutNext": "MiniWorld-PutNext-v0", "TMazeTwoBox": "MiniWorld-TMazeTwoBoxDynamic-v0", "CollectHealth": "MiniWorld-CollectHealth-v0"}
# turn_left 0, turn_right 1, move_forward 2, move_back 3, pickup 4, drop 5; env e takes the sequence rotated by e
ACTIONS = [2, 2, 4, 0, 2, 5, 1, 2, 4, 2, 3, 5]


def golden_path(task):
    return os.path.join(HERE, "golden", "hostapi_state_7580f56_%s.npz" % task)


def make(task):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld(ENV_IDS[task], num_envs=N, seed=SEED)
    b.reset()
    return b


def run12(b):
    """the 12 steps; returns whether any env ended an episode on the way"""
    import torch
    ended = False
    for t in range(12):
        b.step(torch.tensor([ACTIONS[(t + e) % 12] for e in range(N)], dtype=torch.int32))
        ended = ended or bool(b.done.any())
    return ended


def record(task):
    """what the golden files hold (run on the commit named above)"""
    b = make(task)
    run12(b)
    st = b.get_state(rng_state=True)
    b.close()
    return st


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("task", sorted(ENV_IDS))
def test_states_are_the_recorded_ones_and_a_snapshot_restores_them(task):
    import torch
    from gym_miniworld_amd import _lib
    b = make(task)
    assert not run12(b)
    snap = b.get_state(rng_state=True)
    want = np.load(golden_path(task))
    assert set(want.files) == set(snap)
    for k in want.files:
        assert same_bits(snap[k], want[k]), (task, k)
    # a sub-range is the rows of the whole
    part = b.get_state(1, 3, rng_state=True)
    assert set(part) == set(snap)
    for k in snap:
        assert same_bits(part[k], snap[k][1:4]), (task, k)
    # snapshot, 12 steps, the snapshot put back, the same 12 steps: the same states and observations
    assert not run12(b)
    after, obs_after = b.get_state(rng_state=True), b.obs.clone()
    keys = [("boxes_" + n[4:] if n.startswith("box_") else n) for n, _, _, writable, ent in _lib.STATE_FIELDS if writable and (b.ent_task or not ent)]
    if b.ent_task:
        assert {"task_f", "ent_order", "ent_meta", "rng_state"} <= set(keys)
    b.set_state(0, **{k: snap[k] for k in keys})
    again = b.get_state(rng_state=True)
    for k in snap:
        assert same_bits(again[k], snap[k]), (task, k)
    assert not run12(b)
    redo = b.get_state(rng_state=True)
    for k in after:
        assert same_bits(redo[k], after[k]), (task, k)
    assert torch.equal(b.obs, obs_after)
    # a sub-range put back touches its envs only
    b.set_state(1, **{k: snap[k][1:4] for k in keys})
    mixed = b.get_state(rng_state=True)
    for k in snap:
        assert same_bits(mixed[k][1:4], snap[k][1:4]) and same_bits(mixed[k][:1], after[k][:1]) and same_bits(mixed[k][4:], after[k][4:]), (task, k)
    b.close()


def test_every_feature_on_one_handle_and_no_second_enable():
    """each feature once, in the order the header prescribes, on one small handle: fused stack, terminal, rollout with learner,
    monitor, levels; three steps, every counter read; a second enable of each is refused with its message and changes nothing"""
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld("MiniWorld-Hallway-v0", num_envs=N, seed=SEED, layout="CWH", greyscale=True)
    L, h = b.L, b.h
    b.stack_enable(2, fused=True)
    term = b.terminal_enable()
    ro = b.rollout_enable(4, nstack=2, learner=True)
    mon = b.monitor_enable(capacity=8, quota_max=2)
    lev = b.levels_enable(7, mode="sequential")

    def refused(rc, text):   # MWB_ESTATE
        assert rc == -4 and text in L.mwb_last_error().decode(), (rc, L.mwb_last_error())
    for _ in range(2):   # (the second round: a refused enable left the flags as they were)
        refused(L.mwb_grey_enable(h), "mwb_grey_enable: already enabled")
        refused(L.mwb_stack_enable(h, 2, 1 | _lib.STACK_FUSED), "mwb_stack_enable: already enabled")
        refused(L.mwb_terminal_enable(h, N, 0), "mwb_terminal_enable: already enabled")
        refused(L.mwb_rollout_enable(h, 4, 2, 0), "mwb_rollout_enable: already enabled")
        refused(L.mwb_rollout_learner_enable(h), "mwb_rollout_learner_enable: already enabled")
        refused(L.mwb_monitor_enable(h, 8, 2), "mwb_monitor_enable: already enabled")
        refused(L.mwb_levels_enable(h, 7, 0, None, 0, 0, 0, N, 0), "mwb_levels_enable: already enabled")
    b.reset()
    ro.push(after_reset=True)
    for t in range(3):
        b.step(torch.full((N,), 2, dtype=torch.int32))
        ro.push()
        mon.update()
    assert ro.step == 3 and ro.taken[:3].eq(1).all()
    assert ro.rejected() == 0 and term.dropped() == 0 and lev.rejected() == 0 and b.copy_rejected() == 0
    reused, rendered = b.frame_reuse_stats()
    assert reused + rendered == 3 * N and b.frame_reuse_stats() == (0, 0)   # read and cleared
    assert mon.read() == (0, 0, N)                                          # nobody ended an episode, nobody retired
    assert int(term.count[0]) == 0 and lev.index.tolist() == list(range(N))   # sequential: env e starts on level e
    b.close()
