"""Host build of gym_miniworld_amd/csrc/mwb_lds_layout.h (tests/lds_layout_host.cpp) for the tests that size things with the
kernels' own layout arithmetic: test_lds_layout.py (the layouts themselves) and test_gpu_frame_sizes.py (the frame sizes at which
mwb_create switches a handle to tiles)."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LDS_LIMIT = 160 * 1024   # mwb_create: a frame whose whole-frame launch asks for more is rendered in tiles

_host = None


def build_lds_host():
    """compiles (when stale) and loads tests/_build/liblds_layout_host.so"""
    global _host
    if _host is not None:
        return _host
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "liblds_layout_host.so")
    srcs = [os.path.join(HERE, "lds_layout_host.cpp"), os.path.join(ROOT, "gym_miniworld_amd", "csrc", "mwb_lds_layout.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", so, srcs[0]])
    L = ctypes.CDLL(so)
    L.lds_launch_bytes.restype = ctypes.c_long
    _host = L
    return L


def frame_words(n_boxes):   # MWB_FRAME_WORDS_FOR
    return (36 + 34 * n_boxes + 3) & ~3
