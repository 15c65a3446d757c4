"""CPU: how mwb_step_repeat folds its sub-steps into one transition per env.  The device applies the rule of
gym_miniworld_amd/csrc/mwb_repeat_fold.h after every sub-step (repeat_fold_kernel); here the same header is built into a small
host program that plays a whole call - output slots kept as the step kernels keep them, frozen envs untouched - and is compared
with the frame-skip wrapper's loop restated in Python.  Also: what step_repeat refuses before anything reaches a GPU, and the
two new symbols of the ABI."""
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def wrapper_loop(steps, n):
    """for _ in range(n): obs, r, done, info = env.step(a); total += r; if done: break  -  `steps`: the (reward, done) env.step returns"""
    total, taken, done = 0.0, 0, False
    for r, done in steps[:n]:
        total += r
        taken += 1
        if done:
            break
    return total, taken, bool(done)


@pytest.fixture(scope="module")
def fold_host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "repeat_fold_host")
    srcs = [os.path.join(HERE, "repeat_fold_host.cpp"), os.path.join(ROOT, "gym_miniworld_amd", "csrc", "mwb_repeat_fold.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.dirname(srcs[1]), "-o", exe, srcs[0]])

    def run(repeat, auto_reset, envs):
        """envs: [(masked, count, skip_same, [(reward, done, frame_same)] * repeat)] -> [(sum, reward f32, taken, frame_same, done, last sub-step)]"""
        lines = ["%d %d %d" % (repeat, len(envs), auto_reset)]
        for masked, count, skip_same, seq in envs:
            assert len(seq) == repeat
            lines.append("%d %d %d " % (masked, count, skip_same) +
                         " ".join("%x %d %d" % (struct.unpack("<Q", struct.pack("<d", r))[0], d, fs) for r, d, fs in seq))
        res = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
        outs = []
        for ln in res[:len(envs)]:
            sb, fb, taken, same, done, applied = ln.split()
            outs.append((struct.unpack("<d", struct.pack("<Q", int(sb, 16)))[0], struct.unpack("<f", struct.pack("<I", int(fb, 16)))[0],
                         int(taken), int(same), int(done), int(applied)))
        return outs
    return run


def bits(x):
    return struct.pack("<d", x)


def reward_pool(rng, max_steps=280):
    """what the step kernels hand out: 0, 1 - 0.2 * (sc / max) at a goal, its negative at the T-maze's penalty box, PickupObjs' 1,
    CollectHealth's 2 and -100, and arbitrary doubles (sums whose value depends on the order)"""
    sc = int(rng.integers(1, max_steps + 1))
    rw = 1.0 - 0.2 * (sc / max_steps)
    return [0.0, rw, -1 * rw, rw + -1 * rw, 1.0, 2.0, -100.0, float(rng.normal()) * 10.0 ** int(rng.integers(-8, 8)), 0.1, 1e16][int(rng.integers(0, 10))]


def test_fold_equals_the_wrapper_loop(fold_host):
    rng = np.random.default_rng(12)
    seen = {"done_first": 0, "done_mid": 0, "done_last": 0, "count_cut": 0, "masked": 0, "negative": 0, "same_kept": 0, "same_lost_early": 0}
    for trial in range(60):
        repeat = int(rng.integers(1, 9)) if trial else 64
        auto_reset = int(rng.integers(0, 2))
        envs = []
        for e in range(70):
            done_at = int(rng.integers(0, 2 * repeat))   # >= repeat: never
            seq = [(reward_pool(rng), int(j == done_at or rng.random() < 0.05), int(rng.random() < 0.7)) for j in range(repeat)]
            if e % 7 == 0:   # nothing changes the frame in any sub-step
                seq = [(r, d, 1) for r, d, _ in seq]
            if e % 7 == 1:   # a move in the first sub-step, blocked afterwards
                seq = [(r, d, int(j > 0)) for j, (r, d, _) in enumerate(seq)]
            envs.append((int(rng.random() < 0.15), int(rng.integers(-2, repeat + 6)), int(rng.integers(0, 2)), seq))
        got = fold_host(repeat, auto_reset, envs)
        for e, ((masked, count, skip_same, seq), (total, rew, taken, same, done, applied)) in enumerate(zip(envs, got)):
            tag = (trial, e, repeat, masked, count, seq)
            if masked:   # the fork's 'dummy' command, once: never summed k times
                assert bits(total) == bits(-99.0) and rew == -99.0 and taken == 0 and done == 0 and same == skip_same and applied == -1, tag
                seen["masked"] += 1
                continue
            n = min(max(count, 1), repeat)
            want_total, want_taken, want_done = wrapper_loop([(r, d) for r, d, _ in seq], n)
            assert bits(total) == bits(want_total), tag   # bit for bit, in sub-step order from 0.0
            assert bits(float(rew)) == bits(float(np.float32(want_total))), tag
            assert taken == want_taken and bool(done) == want_done and applied == want_taken - 1, tag   # outputs: the last sub-step taken
            want_same = all(fs for _, _, fs in seq[:want_taken]) and not (want_done and auto_reset)
            assert bool(same) == want_same, tag
            seen["done_first"] += want_done and want_taken == 1 and repeat > 1
            seen["done_mid"] += want_done and 1 < want_taken < n
            seen["done_last"] += want_done and want_taken == n and n > 1
            seen["count_cut"] += (not want_done) and want_taken < repeat
            seen["negative"] += want_total < 0
            seen["same_kept"] += want_same and want_taken > 1
            seen["same_lost_early"] += (not seq[0][2]) and all(fs for _, _, fs in seq[1:want_taken]) and want_taken > 1
    assert all(v > 0 for v in seen.values()), seen


def test_order_of_the_sum_is_the_sub_step_order(fold_host):
    """1e16 + 1 + 1 + ... differs from 1 + 1 + ... + 1e16 in float64: the fold must add in sub-step order, starting from 0.0"""
    seq = [(1e16, 0, 1)] + [(1.0, 0, 1)] * 7
    (a, _, ta, _, _, _), (b, _, tb, _, _, _) = fold_host(8, 1, [(0, 8, 0, seq), (0, 8, 0, seq[::-1])])
    assert a == wrapper_loop([(r, d) for r, d, _ in seq], 8)[0] and b == wrapper_loop([(r, d) for r, d, _ in seq[::-1]], 8)[0]
    assert a != b and ta == tb == 8


def test_counts_are_clamped(fold_host):
    seq = [(2.0, 0, 1)] * 4
    got = fold_host(4, 1, [(0, c, 0, seq) for c in (-5, 0, 1, 2, 4, 5, 9, 2 ** 31 - 1, -2 ** 31)])
    assert [g[2] for g in got] == [1, 1, 1, 2, 4, 4, 4, 4, 1]
    assert [g[0] for g in got] == [2.0, 2.0, 2.0, 4.0, 8.0, 8.0, 8.0, 8.0, 2.0]


def test_step_repeat_refuses_bad_arguments_before_any_launch():
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.batch import BatchedMiniWorld, check_repeat_args
    assert _lib.MAX_REPEAT == 64
    assert check_repeat_args(1, 70, 70) == 1 and check_repeat_args(np.int64(64), 70, 70, 70, 70) == 64
    for bad in (0, -1, _lib.MAX_REPEAT + 1, 2.0, "4", None, True):
        with pytest.raises(ValueError):
            check_repeat_args(bad, 70, 70)
    for kw in (dict(n_actions=69), dict(n_actions=70, n_skip=71), dict(n_actions=70, n_counts=1)):
        with pytest.raises(ValueError):
            check_repeat_args(4, 70, **kw)
    # the method itself, on an object that has no handle: it must raise before it touches the library
    b = object.__new__(BatchedMiniWorld)
    b.torch, b.num_envs, b.device, b.h = torch, 70, torch.device("cpu"), None
    acts = torch.zeros(70, dtype=torch.int32)
    for rep in (0, _lib.MAX_REPEAT + 1):
        with pytest.raises(ValueError):
            b.step_repeat(acts, rep)
    with pytest.raises(ValueError):
        b.step_repeat(acts[:69], 4)
    with pytest.raises(ValueError):
        b.step_repeat(acts, 4, skip_mask=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        b.step_repeat(acts, 4, counts=torch.ones(71, dtype=torch.int32))


def test_new_symbols_are_exported_and_the_header_states_the_limit():
    from gym_miniworld_amd import _lib, build
    build.build()
    assert "mwb_step_repeat" in _lib.EXPORTS and "mwb_repeat_taken" in _lib.EXPORTS
    L = _lib.load()
    assert L.mwb_step_repeat is not None and L.mwb_repeat_taken is not None
    hdr = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    assert "#define MWB_MAX_REPEAT %d" % _lib.MAX_REPEAT in hdr
    # refused without a handle, with a message
    assert L.mwb_step_repeat(None, None, None, None, 4, None, None) == -1
    assert L.mwb_repeat_taken(None, None) == -1
