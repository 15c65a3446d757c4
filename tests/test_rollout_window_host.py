"""CPU: the windowed gather's rule, draws, limits, ABI and kernel resources.

gym_miniworld_amd/csrc/mwb_rollout_window_map.h - the functions mwb_rollout_window_offsets / mwb_rollout_gather_window, their kernels
and this test share - is built into a host program (rollout_window_host.cpp).  Its draws are compared with an independent
restatement in Python integers and with Augment.offsets_of; its per-pixel source rule with a numpy restatement of the rule as
include/miniworld_batch.h states it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gym_miniworld_amd", "csrc")
WINDOW_SYMBOLS = ["mwb_rollout_window_offsets", "mwb_rollout_gather_window"]
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "rollout_window_host")
    srcs = [os.path.join(HERE, "rollout_window_host.cpp"), os.path.join(CSRC, "mwb_rollout_window_map.h"), os.path.join(CSRC, "mwb_levels_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, srcs[0]]
        # with AddressSanitizer + UBSan where their runtimes link (a stand-alone program: nothing is preloaded), plain otherwise
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        return [ln for ln in res.stdout.split("\n") if ln]
    return run


# ------------------------------------------------------------------------------------- the restatements
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key_of(seed, call):
    return mix((seed + GOLD * (call + 1)) & M64)


def draw_of(key, index, dx_lo, dx_hi, dy_lo, dy_hi):
    h = mix((key + GOLD * ((index & M64) + 1)) & M64)
    return (dx_lo + (((h >> 32) * (dx_hi - dx_lo + 1)) >> 32), dy_lo + (((h & 0xffffffff) * (dy_hi - dy_lo + 1)) >> 32))


def window_of(W, H, win, dx, dy):
    """the rule of include/miniworld_batch.h over every output pixel -> (sx, sy, shown) as [out_w, out_h] arrays"""
    out_w, out_h, border, dx_lo, dx_hi, dy_lo, dy_hi = win
    dx, dy = min(max(dx, dx_lo), dx_hi), min(max(dy, dy_lo), dy_hi)
    x, y = np.meshgrid(np.arange(out_w), np.arange(out_h), indexing="ij")
    sx, sy = x + dx, y + dy
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    return (dx, dy), np.clip(sx, 0, W - 1), np.clip(sy, 0, H - 1), inside | (border == 0)


def draws(host, seed, call, rng4, indices):
    lines = host(["D %d %d %d %d %d %d %d" % ((seed, call) + tuple(rng4) + (i,)) for i in indices])
    return [tuple(int(v) for v in ln.split()) for ln in lines]


# ------------------------------------------------------------------------------------- draws
def test_known_answers(host):
    from gym_miniworld_amd.batch import Augment
    assert host(["K 0 0", "K 7 3"]) == ["e220a8397b1dcdaf", "953aeb70673e29cb"]
    assert key_of(0, 0) == 0xe220a8397b1dcdaf and key_of(7, 3) == 0x953aeb70673e29cb
    want = [(1, -2), (2, 4), (-1, 4), (1, 0), (3, -1), (-3, 1), (3, 0), (-2, -1)]
    assert draws(host, 0, 0, (-4, 4, -4, 4), range(8)) == want
    aug = Augment.shift(4)
    aug.bind(80, 60)
    assert [tuple(r) for r in aug.offsets_of(np.arange(8)).tolist()] == want
    idx = [0, 1, 47, 2 ** 31, 2 ** 40]
    want = [(11, 1), (3, 2), (16, 9), (12, 1), (3, 8)]
    assert draws(host, 7, 3, (0, 16, 0, 12), idx) == want
    crop = Augment.crop(64, 48, seed=7)
    crop.bind(80, 60)   # ranges 0 .. 16 x 0 .. 12
    assert crop.window == (64, 48, 0, 0, 16, 0, 12)
    assert [tuple(r) for r in crop.offsets_of(idx, call=3).tolist()] == want


@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
@pytest.mark.parametrize("call", [0, 1, 2 ** 40])
def test_header_draws_equal_the_restatement_and_offsets_of(host, seed, call):
    from gym_miniworld_amd.batch import Augment
    N, T = 16, 3
    idx = [0, 1, N * T - 1, 2 ** 31, 2 ** 40, 2 ** 63 - 1]
    for aug, W, H in ((Augment.shift(4, seed=seed), 80, 60), (Augment.crop(64, 48, seed=seed), 80, 60),
                      (Augment.translate(96, 72, seed=seed), 80, 60), (Augment.center_crop(6, 4), 10, 6), (Augment.shift(61, seed=seed), 80, 60)):
        win = aug.bind(W, H)
        got = draws(host, aug.seed, call, win[3:], idx)
        key = key_of(aug.seed, call)
        assert got == [draw_of(key, i, *win[3:]) for i in idx], (aug.kind, seed, call)
        assert got == [tuple(r) for r in aug.offsets_of(idx, call=call).tolist()], (aug.kind, seed, call)
        assert all(win[3] <= dx <= win[4] and win[5] <= dy <= win[6] for dx, dy in got)
    assert Augment.shift(4, seed=seed).seed == seed


@pytest.mark.parametrize("widths", [(1, 1), (2, 1), (9, 9), (17, 13), (61, 1), (1, 61)])
def test_every_pair_of_the_range_occurs(host, widths):
    for seed, call in ((0, 0), (0, 1), (7, 3), (2 ** 64 - 1, 2 ** 40)):
        rng4 = (-(widths[0] // 2), widths[0] - 1 - widths[0] // 2, -3, widths[1] - 4)
        got = draws(host, seed, call, rng4, range(4096))
        assert all(rng4[0] <= dx <= rng4[1] and rng4[2] <= dy <= rng4[3] for dx, dy in got), (widths, seed, call)
        assert len(set(got)) == widths[0] * widths[1], (widths, seed, call, len(set(got)))
        key = key_of(seed, call)
        assert got[:64] == [draw_of(key, i, *rng4) for i in range(64)]


def test_calls_draw_separately(host):
    a = draws(host, 0, 0, (-4, 4, -4, 4), range(4096))
    b = draws(host, 0, 1, (-4, 4, -4, 4), range(4096))
    same = sum(x == y for x, y in zip(a, b))
    assert same < 0.05 * 4096, same   # chance is 1 in 81


# ------------------------------------------------------------------------------------- the window rule
WINDOWS = {   # (W, H) -> windows (out_w, out_h, border, dx_lo, dx_hi, dy_lo, dy_hi): smaller than, equal to and larger than the frame
    (10, 6): [(10, 6, 0, -2, 2, -2, 2), (10, 6, 1, -2, 2, -2, 2), (6, 4, 0, 0, 4, 0, 2), (4, 3, 1, 0, 6, 0, 3), (14, 10, 1, -4, 0, -4, 0),
              (14, 10, 0, -4, 0, -4, 0), (1, 4, 0, 0, 9, 0, 2), (10, 6, 0, -11, 11, -7, 7), (10, 6, 1, -32767, 32767, -32767, 32767)],
    (80, 60): [(80, 60, 0, -4, 4, -4, 4), (80, 60, 1, -4, 4, -4, 4), (80, 60, 0, -61, 61, -61, 61), (64, 48, 0, 0, 16, 0, 12),
               (76, 57, 1, 0, 4, 0, 3), (96, 72, 1, -16, 0, -12, 0), (96, 72, 0, -16, 0, -12, 0), (80, 60, 0, 0, 0, 0, 0)],
}


@pytest.mark.parametrize("size", sorted(WINDOWS))
def test_header_window_rule_equals_the_restatement(host, size):
    W, H = size
    zeros = replicated = 0
    for win in WINDOWS[size]:
        _, _, border, dx_lo, dx_hi, dy_lo, dy_hi = win
        pairs = [(dx_lo, dy_lo), (dx_lo, dy_hi), (dx_hi, dy_lo), (dx_hi, dy_hi), ((dx_lo + dx_hi) // 2, (dy_lo + dy_hi) // 2),
                 (dx_lo - 1, dy_hi + 1), (dx_hi + 1000, dy_lo - 1000), (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (I32_MIN, I32_MIN), (I32_MAX, I32_MAX)]
        for dx, dy in pairs:
            lines = host(["W %d %d %s %d %d" % (W, H, " ".join(map(str, win)), dx, dy)])
            (cdx, cdy), sx, sy, shown = window_of(W, H, win, dx, dy)
            assert lines[0] == "O %d %d" % (cdx, cdy), (win, dx, dy, lines[0])
            assert dx_lo <= cdx <= dx_hi and dy_lo <= cdy <= dy_hi
            want = ["%d %d" % (a, b) if s else "zero" for a, b, s in zip(sx.reshape(-1), sy.reshape(-1), shown.reshape(-1))]
            assert lines[1:] == want, (win, dx, dy)
            zeros += int((~shown).sum())
            replicated += int((shown & ((sx != np.arange(win[0])[:, None] + cdx) | (sy != np.arange(win[1])[None, :] + cdy))).sum())
    assert zeros and replicated, (zeros, replicated)   # both borders were exercised


def test_division_by_multiplication_is_exact(host):
    ds = [1, 2, 3, 4, 6, 48, 57, 60, 72, 240, 1023, 1024]
    assert host(["M %d" % d for d in ds]) == ["0"] * len(ds)


# ------------------------------------------------------------------------------------- limits
BAD_WINDOWS = [   # (window, the limit it breaks)
    ((0, 4, 0, 0, 0, 0, 0), 1), ((4, 0, 0, 0, 0, 0, 0), 1), ((1025, 4, 0, 0, 0, 0, 0), 1), ((4, 1025, 0, 0, 0, 0, 0), 1), ((-4, 4, 0, 0, 0, 0, 0), 1),
    ((3, 3, 0, 0, 0, 0, 0), 2), ((2, 3, 0, 0, 0, 0, 0), 2), ((1023, 1022, 0, 0, 0, 0, 0), 2),
    ((4, 4, 0, 1, 0, 0, 0), 3), ((4, 4, 0, 0, 0, 1, 0), 3),
    ((4, 4, 0, -32768, 0, 0, 0), 4), ((4, 4, 0, 0, 32768, 0, 0), 4), ((4, 4, 0, 0, 0, -32768, 0), 4), ((4, 4, 0, 0, 0, 0, 32768), 4),
    ((4, 4, 0, I32_MIN, I32_MAX, 0, 0), 4),
    ((4, 4, 2, 0, 0, 0, 0), 5), ((4, 4, -1, 0, 0, 0, 0), 5),
]
GOOD_WINDOWS = [(1, 4, 0, 0, 0, 0, 0), (1024, 1024, 1, -32767, 32767, -32767, 32767), (80, 60, 0, -4, 4, -4, 4), (2, 2, 1, 5, 5, -7, -7)]


def test_every_limit_is_refused(host):
    lines = host(["C " + " ".join(map(str, w)) for w, _ in BAD_WINDOWS] + ["C " + " ".join(map(str, w)) for w in GOOD_WINDOWS])
    codes = [int(ln.split()[0]) for ln in lines]
    assert codes == [c for _, c in BAD_WINDOWS] + [0] * len(GOOD_WINDOWS)
    assert all(len(ln.split()) > 1 for ln in lines[:len(BAD_WINDOWS)])   # every refusal has a text


def test_augment_refuses_before_anything_runs():
    from gym_miniworld_amd.batch import Augment, check_window_offsets
    with pytest.raises(ValueError, match="does not fit"):
        Augment.crop(81, 60).bind(80, 60)
    with pytest.raises(ValueError, match="does not fit"):
        Augment.crop(80, 61).bind(80, 60)
    with pytest.raises(ValueError, match="does not fit"):
        Augment.center_crop(0, 4).bind(80, 60)
    with pytest.raises(ValueError, match="smaller than"):
        Augment.translate(79, 60).bind(80, 60)
    with pytest.raises(ValueError, match="smaller than"):
        Augment.translate(80, 56).bind(80, 60)
    with pytest.raises(ValueError, match="pad -1"):
        Augment.shift(-1)
    with pytest.raises(ValueError, match="pad 32768"):
        Augment.shift(32768)
    with pytest.raises(ValueError, match="multiple of 4"):
        Augment.crop(77, 57).bind(80, 60)
    with pytest.raises(ValueError, match="multiple of 4"):
        Augment.translate(81, 61).bind(80, 60)
    with pytest.raises(ValueError, match="outside 1 .. 1024"):
        Augment.translate(1028, 60).bind(80, 60)
    with pytest.raises(ValueError, match="integer"):
        Augment.shift(1.5)
    with pytest.raises(ValueError, match="not bound"):
        Augment.crop(64, 48).offsets_of([0])
    aug = Augment.crop(64, 48, seed=5)
    assert aug.calls == 0 and aug.seed == 5 and aug.bind(80, 60) == (64, 48, 0, 0, 16, 0, 12) and aug.bind(80, 60) == aug.window
    with pytest.raises(ValueError, match="bound to 80 x 60"):
        aug.bind(10, 6)
    assert Augment.shift(4).bind(10, 6) == (10, 6, 0, -4, 4, -4, 4)
    assert Augment.center_crop(64, 48).bind(80, 60) == (64, 48, 0, 8, 8, 6, 6)
    assert Augment.center_crop(75, 56).bind(80, 60) == (75, 56, 0, 2, 2, 2, 2)
    assert Augment.translate(96, 72).bind(80, 60) == (96, 72, 1, -16, 0, -12, 0)
    # offsets that live on the host
    assert check_window_offsets([[1, -2], [3, 4]], 2).dtype == np.int32
    for bad, n in (([[1.0, 2.0]], 1), ([[True, False]], 1), ([1, 2], 1), ([[1, 2]], 2), ([[1, 2, 3]], 1), ([[2 ** 31, 0]], 1)):
        with pytest.raises(ValueError):
            check_window_offsets(bad, n)
    import gym_miniworld_amd
    assert gym_miniworld_amd.Augment is Augment and "Augment" in gym_miniworld_amd.__all__


# ------------------------------------------------------------------------------------- ABI
def test_window_symbols_are_exported_and_the_abi_version_stands():
    from gym_miniworld_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in WINDOW_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert getattr(L, name) is not None
    assert "#define MWB_ABI_VERSION 5" in hdr and _lib.ABI_VERSION == 5 and L.mwb_abi_version() == 5
    assert ctypes.sizeof(_lib.MwbRolloutWindow) == 32
    assert re.search(r"struct\s+mwb_rollout_window\s*\{\s*int32_t\s+out_w,\s*out_h,\s*border,\s*dx_lo,\s*dx_hi,\s*dy_lo,\s*dy_hi,\s*pad;\s*\}", code)
    win = _lib.MwbRolloutWindow(80, 60, 0, -4, 4, -4, 4, 0)
    # refused without a handle or without a window, with the function's name in the message
    assert L.mwb_rollout_window_offsets(None, ctypes.byref(win), 0, 0, None, 0, None, None) == -1
    assert b"mwb_rollout_window_offsets" in L.mwb_last_error()
    assert L.mwb_rollout_gather_window(None, None, 0, ctypes.byref(win), None, None, 1, None) == -1
    assert b"mwb_rollout_gather_window" in L.mwb_last_error()
    assert L.mwb_rollout_window_offsets(None, None, 0, 0, None, 0, None, None) == -1 and b"mwb_rollout_window_offsets" in L.mwb_last_error()
    assert L.mwb_rollout_gather_window(None, None, 0, None, None, None, 1, None) == -1 and b"mwb_rollout_gather_window" in L.mwb_last_error()
    assert _lib.WINDOW_MAX_OUT == 1024 and _lib.WINDOW_MAX_OFFSET == 32767
    src = open(os.path.join(CSRC, "mwb_rollout_window_map.h")).read()
    assert "#define MWB_WINDOW_MAX_OUT 1024" in src and "#define MWB_WINDOW_MAX_OFFSET 32767" in src


# ------------------------------------------------------------------------------------- resources
@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_window_kernels_use_no_scratch_and_little_lds():
    """every rollout_window kernel reports 0 bytes of scratch and at most 32 KB of LDS (five workgroups per CU); the plain gather
    still has its five instantiations"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources, remarks_of_the_build
    from gym_miniworld_amd import build
    build.build()
    if remarks_of_the_build() is not None:
        table = kernel_resources()
    else:
        table = dict(kernel_resources(src=os.path.join(CSRC, "mwb_rollout_window.hip")), **kernel_resources(src=os.path.join(CSRC, "mwb_rollout.hip")))
    window = {n: r for n, r in table.items() if "rollout_window" in n}
    # (float32 | uint8 | grey) x (edge replication | zero border)
    assert sum("rollout_window_kernel" in n for n in window) == 6 and sum("rollout_window_offsets_kernel" in n for n in window) == 1, sorted(window)
    for n, r in window.items():
        assert r["scratch"] == 0 and r["lds"] <= 32768, (n, r)
    assert sum("rollout_gather_kernel" in n for n in table) == 5, sorted(n for n in table if "rollout_gather" in n)
    banned = ["rollout_gather_kernel", "rollout_gather_cols_kernel", "rollout_returns_kernel", "rollout_insert_kernel", "rollout_taken_kernel",
              "render_kernel", "reset_kernel", "monitor"]
    assert not any(b in n for n in window for b in banned)
