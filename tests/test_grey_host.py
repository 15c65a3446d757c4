"""CPU: the greyscale entry points of the C ABI (include/miniworld_batch.h) as the binding sees them, their refusals that need no
device, and the NumPy restatement of GreyscaleWrapper that the GPU tests (test_gpu_grey.py) compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

from grey_ref import grey_of_channels, grey_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREY_FUNCTIONS = {"mwb_grey_enable": 1, "mwb_grey_output": 3, "mwb_grey_convert": 8}   # name -> parameters


@pytest.fixture(scope="module")
def built():
    from gym_miniworld_amd import build
    build.build()
    from gym_miniworld_amd import _lib
    return _lib


def header_text():
    src = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_constants_and_prototypes_agree_with_the_header(built):
    src = header_text()
    defines = dict(re.findall(r"#define\s+(MWB_\w+)\s+(\d+)\s", src))
    assert int(defines["MWB_STACK_GREY"]) == built.STACK_GREY == 64
    assert int(defines["MWB_STACK_SLIDING"]) == built.STACK_SLIDING and int(defines["MWB_STACK_FUSED"]) == built.STACK_FUSED
    assert int(defines["MWB_STACK_SLACK_FRAMES"]) == built.STACK_SLACK_FRAMES
    assert int(defines["MWB_ABI_VERSION"]) == built.ABI_VERSION == 5   # the greyscale entry points are additive
    flags = [built.STACK_SLIDING, built.STACK_FUSED, built.STACK_GREY]
    assert all(f > 1 and f & (f - 1) == 0 for f in flags) and len(set(flags)) == 3   # distinct bits above the dtype bit
    L = built.load()
    for name, n_params in GREY_FUNCTIONS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == n_params, (name, m.group(1))
        assert name in built.EXPORTS
        assert len(getattr(L, name).argtypes) == n_params, name


def test_null_handles_are_refused_with_a_message(built):
    L = built.load()
    assert L.mwb_grey_enable(None) == -1   # MWB_EINVAL
    assert b"mwb_grey_enable" in L.mwb_last_error()
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.mwb_grey_output(None, ctypes.byref(p), ctypes.byref(n)) == -1
    assert b"mwb_grey_output" in L.mwb_last_error()
    assert L.mwb_grey_convert(None, None, None, 1, 4, 4, 0, None) == -1
    assert b"mwb_grey_convert" in L.mwb_last_error()


def test_numpy_restatement_spot_values():
    u8 = lambda *v: np.array(v, np.uint8)   # noqa: E731
    g = grey_of_channels(u8(255, 0), u8(255, 0), u8(255, 0))
    assert g.dtype == np.float32 and g[0] == 255.0 and g[1] == 0.0   # white, black
    # by hand: 0.30 * 255 = 76.5 (exact in binary); 30 + 88.5 + 22 = 140.5 (exact); 0.59 * 255 = 150.45 and 0.11 * 255 = 28.05 are
    # not: the float32 nearest to each
    assert grey_of_channels(u8(255), u8(0), u8(0))[0] == np.float32(76.5)
    assert grey_of_channels(u8(100), u8(150), u8(200))[0] == np.float32(140.5)
    assert grey_of_channels(u8(0), u8(255), u8(0))[0] == np.float32(150.45)
    assert grey_of_channels(u8(0), u8(0), u8(255))[0] == np.float32(28.05)
    assert grey_of_channels(u8(1), u8(1), u8(1))[0] == np.float32(1.0)


def test_numpy_restatement_layouts():
    rng = np.random.default_rng(0)
    hwc = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)       # [N,H,W,3]
    cwh = np.ascontiguousarray(hwc.transpose(0, 3, 2, 1))          # TransposeImage: [N,3,W,H]
    a, b = grey_ref(hwc, "HWC"), grey_ref(cwh, "CWH")
    assert a.shape == (2, 5, 7, 1) and b.shape == (2, 1, 7, 5) and a.dtype == b.dtype == np.float32
    assert np.array_equal(a.transpose(0, 3, 2, 1), b)
    # float32 arithmetic alone is NOT the contract: it rounds differently for many colours
    r, g, bl = (hwc[..., k].astype(np.float32) for k in range(3))
    f32 = (np.float32(0.30) * r + np.float32(0.59) * g) + np.float32(0.11) * bl
    assert (f32 != a[..., 0]).any()
