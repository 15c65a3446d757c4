"""CPU: the rollout storage's ring arithmetic, host-side index check and ABI.

gym_miniworld_amd/csrc/mwb_rollout_map.h - the functions mwb_rollout_push / _gather / _after_update and their kernels share - is
built into a host program (rollout_map_host.cpp) that plays pushes and after_updates and prints, for every (t, env, frame group)
of the window, the ring slot the gather would read or "zeros".  The yardstick is a restatement of VecPyTorchFrameStack
(tests/stack_ref.py::FrameStackRef) over frame IDS instead of pixels: per env the list of the last nstack frame ids, shifted every
step, cleared when the env was done.  A slot must hold exactly the frame id the restated stack holds at that place - at every
moment, so a push that overwrote a frame still needed shows up as a wrong id."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gym_miniworld_amd", "csrc")
ROLLOUT_SYMBOLS = ["mwb_rollout_enable", "mwb_rollout_push", "mwb_rollout_gather", "mwb_rollout_after_update", "mwb_rollout_info",
                   "mwb_rollout_rejected"]


@pytest.fixture(scope="module")
def map_host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "rollout_map_host")
    srcs = [os.path.join(HERE, "rollout_map_host.cpp"), os.path.join(CSRC, "mwb_rollout_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, srcs[0]]
        # with AddressSanitizer + UBSan where their runtimes link (a stand-alone program: nothing is preloaded), plain otherwise
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)

    def run(T, nstack, fresh):
        """fresh: [W][T][E] flags -> the program's output lines, split"""
        W, E = len(fresh), len(fresh[0][0])
        text = "%d %d %d %d\n" % (T, nstack, E, W) + "\n".join(" ".join(str(int(f)) for f in row) for win in fresh for row in win) + "\n"
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        return [ln.split() for ln in res.stdout.split("\n") if ln]
    return run


def fresh_flags(T, nstack, rng):
    """[W][T][E]: env a < nstack - 1 is done exactly once, a steps before the last after_update, env nstack - 1 never (so that
    every age 0 .. nstack - 1 stands at t = 0 of the last window); then an env done at t = 1 of every window, one done at t = T of
    every window and two with random episode ends"""
    W = max(4, -(-(nstack - 1) // T) + 1)
    E = nstack + 4
    last_update = (W - 1) * T   # global step count at the last after_update
    fresh = np.zeros((W, T, E), np.int64)
    for a in range(nstack - 1):
        g = last_update - a   # global step 1 .. W*T
        fresh[(g - 1) // T, (g - 1) % T, a] = 1
    fresh[:, 0, nstack] = 1
    fresh[:, T - 1, nstack + 1] = 1
    fresh[:, :, nstack + 2:] = rng.random((W, T, 2)) < 0.3
    return fresh


@pytest.mark.parametrize("T,nstack", list(itertools.product((1, 2, 3, 8), (1, 2, 4, 16))))
def test_map_header_against_the_frame_stack(map_host, T, nstack):
    rng = np.random.default_rng(100 * T + nstack)
    fresh = fresh_flags(T, nstack, rng)
    W, _, E = fresh.shape
    assert W >= 4   # three or more after_updates
    lines = map_host(T, nstack, fresh.tolist())

    next_id = 0
    content = {}                          # ring slot -> id of the frame it holds now
    stack = [[None] * nstack for _ in range(E)]   # FrameStackRef over frame ids, per env
    snap = {}                             # t -> [per env tuple of nstack ids] of the current window
    needed, dump_key = set(), None        # slots the valid (t, e, k) of the latest dump map to
    seen = {"done_t1": 0, "done_tT": 0, "prev_window": 0, "zeros": 0, "frames": 0}
    ages_after_update = set()
    n_pushes = 0
    for ln in lines:
        if ln[0] == "P":
            w, t, slot = map(int, ln[1:])
            assert 0 <= slot < T + nstack
            assert slot not in needed, ("push onto a slot the window still maps to", w, t, slot)
            needed, dump_key = set(), None
            content[slot] = next_id
            if t == 0:   # FrameStackRef.reset
                assert w == 0 and n_pushes == 0
                for e in range(E):
                    stack[e] = [None] * (nstack - 1) + [next_id]
            else:        # FrameStackRef.step
                for e in range(E):
                    f = fresh[w, t - 1, e]
                    stack[e] = ([None] * (nstack - 1) if f else stack[e][1:]) + [next_id]
                    seen["done_t1"] += bool(f and t == 1)
                    seen["done_tT"] += bool(f and t == T)
            snap[t] = [tuple(s) for s in stack]
            next_id += 1
            n_pushes += 1
        elif ln[0] == "G":
            w, t, e, age = map(int, ln[1:])
            if t == 0 and w > 0:   # after_update: time T of the window before is time 0 now
                if e == 0:
                    snap = {0: snap[T]}
                ages_after_update.add(age)
            assert age == sum(x is not None for x in snap[t][e]) - 1, (w, t, e, age, snap[t][e])
        else:
            assert ln[0] == "M"
            w, c, t, e, k, slot = map(int, ln[1:])
            if dump_key != (w, c):
                needed, dump_key = set(), (w, c)
            want = snap[t][e][k]
            if want is None:
                assert slot == -1, (w, c, t, e, k, slot)
                seen["zeros"] += 1
            else:
                assert slot >= 0 and content[slot] == want, (w, c, t, e, k, slot, content.get(slot), want)
                needed.add(slot)
                seen["frames"] += 1
                seen["prev_window"] += t - (nstack - 1 - k) < 0
    assert n_pushes == 1 + W * T
    assert seen["done_t1"] and seen["done_tT"] and seen["frames"], seen
    assert ages_after_update == set(range(nstack)), ages_after_update   # every age at t = 0 after an update
    if nstack > 1:
        assert seen["prev_window"] and seen["zeros"], seen   # history read from the window before; zeroed groups


def test_the_restatement_is_the_frame_stack():
    """the id lists above against FrameStackRef itself: frames whose every pixel is their id + 1"""
    import torch
    from stack_ref import FrameStackRef
    nstack, E = 4, 3
    ref = FrameStackRef(E, nstack, (1, 2, 2))
    stack = [[None] * (nstack - 1) + [0] for _ in range(E)]
    ref.reset(torch.full((E, 1, 2, 2), 1.0))
    rng = np.random.default_rng(5)
    for i in range(1, 12):
        news = rng.random(E) < 0.3
        ref.step(torch.full((E, 1, 2, 2), float(i + 1)), torch.as_tensor(news))
        for e in range(E):
            stack[e] = ([None] * (nstack - 1) if news[e] else stack[e][1:]) + [i]
            assert ref.stacked[e, :, 0, 0].tolist() == [0.0 if x is None else x + 1.0 for x in stack[e]]


def test_host_index_check():
    from gym_miniworld_amd.batch import check_rollout_indices
    N, cursor = 16, 2
    ok = check_rollout_indices([0, 5, 17, 47, 5], cursor, N)
    assert ok.dtype == np.int64 and ok.tolist() == [0, 5, 17, 47, 5]
    assert check_rollout_indices(np.array([[1, 2], [3, 4]], np.int32), cursor, N).tolist() == [1, 2, 3, 4]
    with pytest.raises(ValueError, match="negative index -1"):
        check_rollout_indices([3, -1], cursor, N)
    with pytest.raises(ValueError, match=r"index 48 outside \[0, 48\)"):
        check_rollout_indices([47, 48], cursor, N)
    with pytest.raises(ValueError, match=r"index 16 outside \[0, 16\)"):   # t = 1 has not been pushed
        check_rollout_indices([16], 0, N)
    with pytest.raises(ValueError, match=r"outside \[0, 0\)"):   # nothing pushed at all
        check_rollout_indices([0], -1, N)
    with pytest.raises(ValueError, match="must be integers"):
        check_rollout_indices([0.0, 1.0], cursor, N)
    with pytest.raises(ValueError, match="must be integers"):
        check_rollout_indices([True, False], cursor, N)
    with pytest.raises(ValueError, match="must be integers"):
        check_rollout_indices(["3"], cursor, N)
    with pytest.raises(ValueError, match="empty"):
        check_rollout_indices([], cursor, N)
    with pytest.raises(ValueError, match="empty"):
        check_rollout_indices(np.zeros((0,), np.int64), cursor, N)


def test_rollout_symbols_are_exported_and_the_abi_version_stands():
    from gym_miniworld_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in ROLLOUT_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert getattr(L, name) is not None
    assert "#define MWB_ABI_VERSION 5" in hdr and _lib.ABI_VERSION == 5 and L.mwb_abi_version() == 5
    assert "#define MWB_ROLLOUT_GREY %d" % _lib.ROLLOUT_GREY in hdr
    # refused without a handle, with a message
    assert L.mwb_rollout_enable(None, 4, 4, 0) == -1 and b"mwb_rollout_enable" in L.mwb_last_error()
    assert L.mwb_rollout_push(None, 1, None, None) == -1
    assert L.mwb_rollout_gather(None, None, 0, None, 1, None) == -1
    assert L.mwb_rollout_after_update(None, None) == -1
    assert L.mwb_rollout_info(None, None) == -1
    assert L.mwb_rollout_rejected(None, None) == -1
    # struct mwb_rollout_info: 5 pointers, 5 sizes, 6 int32
    assert __import__("ctypes").sizeof(_lib.MwbRolloutInfo) == 10 * 8 + 6 * 4


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_rollout_kernels_use_no_scratch():
    """every rollout_* kernel of csrc/mwb_rollout.hip reports 0 bytes of scratch (and no LDS): compile-time, hipcc's resource remarks"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    table = {n: r for n, r in kernel_resources(src=os.path.join(CSRC, "mwb_rollout.hip")).items() if "rollout_" in n}
    gathers = [n for n in table if "rollout_gather_kernel" in n]
    assert len(gathers) == 5 and any("rollout_push_kernel" in n for n in table) and any("rollout_after_update_kernel" in n for n in table), sorted(table)
    for n, r in table.items():
        assert r["scratch"] == 0 and r["lds"] == 0, (n, r)
