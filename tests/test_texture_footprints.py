"""The bilinear footprint tables the render kernels fetch from (gym_miniworld_amd/csrc/mwb_texture_host.h), built for the
host: for every level of a pyramid, entry (I, J) of its (w+1) x (h+1) table must hold the four texels
L[j0 % h][i0 % w], L[j0 % h][(i0+1) % w], L[(j0+1) % h][i0 % w], L[(j0+1) % h][(i0+1) % w] with (i0, j0) = (I-1, J-1) -
exactly what a wrapped 2x2 fetch at (i0, j0) reads, 1-texel-wide levels included - and the levels' tables must follow one
another without gaps."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U32P = ctypes.POINTER(ctypes.c_uint32)
SIZES = [(1, 1), (1, 7), (2, 1), (3, 5), (16, 4), (768, 768), (1024, 510)]   # (w, h)


@pytest.fixture(scope="module")
def host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libtexture_footprints_host.so")
    srcs = [os.path.join(HERE, "texture_footprints_host.cpp"), os.path.join(ROOT, "gym_miniworld_amd", "csrc", "mwb_texture_host.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, srcs[0]])
    L = ctypes.CDLL(so)
    for f in ("fp_level_texels", "fp_level_off", "fp_total_words", "fp_pyramid_entries", "fp_entries"):
        getattr(L, f).restype = ctypes.c_long
    return L


def level_dims(w, h):
    dims = [(w, h)]
    while w > 1 or h > 1:
        w, h = max(1, w // 2), max(1, h // 2)
        dims.append((w, h))
    return dims


@pytest.mark.parametrize("w,h", SIZES)
def test_every_entry_is_the_wrapped_2x2_block(host, w, h):
    rng = np.random.default_rng(1000 * w + h)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    base = 5
    n_levels = host.fp_build(rgb.ctypes.data_as(ctypes.c_void_p), w, h, base)
    dims = level_dims(w, h)
    assert n_levels == len(dims)
    words = host.fp_total_words()
    table = np.zeros(words, np.uint32)
    host.fp_table_copy(table.ctypes.data_as(U32P))
    table = table.reshape(-1, 4)
    assert (table[:base] == 0xDEADBEEF).all()                      # what was in the buffer before is left alone
    expect_off = base
    for l, (lw, lh) in enumerate(dims):
        assert host.fp_level_texels(l) == lw * lh
        lvl = np.zeros(lw * lh, np.uint32)
        host.fp_level_copy(l, lvl.ctypes.data_as(U32P))
        lvl = lvl.reshape(lh, lw)
        if l == 0:   # the level the table is built from is the image itself, bottom row first, alpha 255
            img = np.flipud(rgb).astype(np.uint32)
            assert (lvl == (img[..., 0] | (img[..., 1] << 8) | (img[..., 2] << 16) | 0xFF000000)).all()
        assert host.fp_level_off(l) == expect_off, (l, "level_off must be contiguous, in 16-byte entries")
        n = (lw + 1) * (lh + 1)
        assert host.fp_entries(lw, lh) == n
        t = table[expect_off:expect_off + n].reshape(lh + 1, lw + 1, 4)
        j0 = (np.arange(lh + 1) - 1) % lh
        j1 = np.arange(lh + 1) % lh
        i0 = (np.arange(lw + 1) - 1) % lw
        i1 = np.arange(lw + 1) % lw
        want = np.stack([lvl[np.ix_(j0, i0)], lvl[np.ix_(j0, i1)], lvl[np.ix_(j1, i0)], lvl[np.ix_(j1, i1)]], axis=-1)
        assert (t == want).all(), (w, h, l)
        expect_off += n
    assert expect_off - base == host.fp_pyramid_entries(w, h) == sum((a + 1) * (b + 1) for a, b in dims)
    assert words == 4 * expect_off
