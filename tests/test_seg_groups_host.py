"""CPU: the float32 bounding boxes of an env's collision segments, eight to a group (gym_miniworld_amd/csrc/mwb_seg_groups.h:
reset_kernel writes them, every circle-vs-walls loop of the step kernels reads them before the segments).  The same header is
built into a small host program - with the host's address and undefined-behaviour sanitizers where the compiler has them -
which checks 1.2 million random groups and the directed cases: every bound of a box lies outside or on the float64 bound of
every member segment, one float32 step at the most, and the group test never turns down a point that a member's own
bounding-box test (step_kernel's) accepts."""
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "seg_groups_host")
    srcs = [os.path.join(HERE, "seg_groups_host.cpp"), os.path.join(ROOT, "gym_miniworld_amd", "csrc", "mwb_seg_groups.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(srcs[1]), "-o", exe, srcs[0]]
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        r = subprocess.run(base + san, capture_output=True, text=True)
        if r.returncode != 0:
            # without sanitizers only where their runtimes are not installed (the linker cannot find them); any other failure is one
            assert any(w in r.stderr for w in ("libasan", "libubsan", "-lasan", "-lubsan")), r.stderr
            subprocess.check_call(base)
            print("seg_groups_host: built WITHOUT sanitizers (runtimes not installed)")
        else:
            print("seg_groups_host: built with -fsanitize=address,undefined")
    return exe


def test_random_and_directed_groups(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    assert f[0] == "checked" and int(f[1]) >= 1000000 and int(f[2]) >= 6 * int(f[1]), r.stdout


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def box(exe, segs):
    args = [float(v).hex() for s in segs for v in s]
    out = subprocess.run([exe, "box", str(len(segs))] + args, check=True, capture_output=True, text=True).stdout
    return [float.fromhex(v) for v in out.split()]


def test_boxes_restated_in_python(exe):
    """Bounds worked out here without the header: the float32 neighbours of 0.1 and 1/3, exact values, a partial group."""
    lo, hi = box(exe, [(0.1, 1.0 / 3.0, 0.1, 1.0 / 3.0)])[0::2]
    assert lo < 0.1 < hi and f32(lo) == lo and f32(hi) == hi and hi - lo == 2.0 ** -27   # consecutive float32 around 0.1
    lo, hi = box(exe, [(0.1, 1.0 / 3.0, 0.1, 1.0 / 3.0)])[1::2]
    assert lo < 1.0 / 3.0 < hi and hi - lo == 2.0 ** -25
    assert box(exe, [(3.0, -1.0, 7.5, -1.0), (7.5, -1.0, 7.5, 4.25)]) == [3.0, -1.0, 7.5, 4.25]
    assert box(exe, [(2.0, 2.0, 1.0, 1.0)] + [(0.0, 0.0, 0.0, 0.0)] * 0) == [1.0, 1.0, 2.0, 2.0]
    assert box(exe, [(1.0, 2.0, 3.0, 4.0), (float("nan"), 0.0, 0.0, 0.0)]) == [float("-inf"), float("-inf"), float("inf"), float("inf")]
    assert box(exe, [(1.0, 2.0, float("-inf"), 4.0)]) == [float("-inf"), float("-inf"), float("inf"), float("inf")]
