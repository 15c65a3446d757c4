"""CPU: the ring arithmetic of the episode monitor's log, its Python restatement, ABI and kernel resources.

gym_miniworld_amd/csrc/mwb_monitor_map.h - where rank r of a pass goes, whether it is written at all, and where the oldest live
record sits - is built into a host program (monitor_map_host.cpp) and compared with collections.deque(maxlen=capacity), the
container the reference's trainer keeps (pytorch-a2c-ppo-acktr/main.py:141), over every (total, capacity, c) of the grid below."""
import ctypes
import os
import re
import subprocess
from collections import deque

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gym_miniworld_amd", "csrc")
MONITOR_SYMBOLS = ["mwb_monitor_enable", "mwb_monitor_update", "mwb_monitor_clear", "mwb_monitor_quota", "mwb_monitor_info", "mwb_monitor_read"]
CAPACITIES = [1, 2, 7, 64]


@pytest.fixture(scope="module")
def map_host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "monitor_map_host")
    srcs = [os.path.join(HERE, "monitor_map_host.cpp"), os.path.join(CSRC, "mwb_monitor_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        cmd = ["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, srcs[0]]
        # with AddressSanitizer + UBSan where their runtimes link (a stand-alone program: nothing is preloaded), plain otherwise
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)

    def run(cases):
        text = "".join("%d %d %d\n" % c for c in cases)
        res = subprocess.run([exe], input=text.encode(), capture_output=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        lines = res.stdout.decode().split("\n")
        assert len(lines) == 2 * len(cases) + 1
        out = []
        for i in range(len(cases)):
            w, r = lines[2 * i].split(), lines[2 * i + 1].split()
            assert w[0] == "W" and r[0] == "R"
            out.append(([tuple(int(x) for x in p.split(":")) for p in w[1:]], [int(x) for x in r[1:]]))
        return out
    return run


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_header_equals_the_deque(map_host, capacity):
    cases = [(total, capacity, c) for total in range(3 * capacity + 1) for c in range(3 * capacity + 2)]
    got = map_host(cases)
    for (total, _, c), (written, readout) in zip(cases, got):
        d = deque(range(total), maxlen=capacity)
        for r in range(c):   # the loop of main.py:167-169: one append per finished env, in env order
            d.append(total + r)
        # the ranks a deque(maxlen) still holds after the pass are the last `capacity` of it
        assert [r for r, _ in written] == [r for r in range(c) if r >= c - capacity], (total, capacity, c)
        assert all(slot == (total + r) % capacity for r, slot in written), (total, capacity, c)
        assert readout == list(d), (total, capacity, c)


@pytest.mark.parametrize("capacity", CAPACITIES + [100, 65536])
def test_python_restatement_of_the_read_out(capacity):
    """Monitor.log()'s slot list (batch.monitor_log_slots) against a ring filled the way the header says"""
    from gym_miniworld_amd.batch import monitor_log_slots
    for total in list(range(3 * min(capacity, 70) + 2)) + [capacity - 1, capacity, capacity + 1, 3 * capacity + 5, 2 ** 40 + 3]:
        if total < 0:
            continue
        first = max(0, total - capacity)
        ring = {i % capacity: i for i in range(first, total)}
        assert [ring[s] for s in monitor_log_slots(total, capacity)] == list(range(first, total)), (total, capacity)


def test_reference_restatement_is_the_loop_with_summed_returns():
    """tests/monitor_ref.py on a case small enough to write down"""
    from monitor_ref import MonitorRef
    m = MonitorRef(3, capacity=2, quota_max=2)
    m.update([0.1, 1.0, 0.0], [0, 1, 0])
    m.update([0.2, 0.5, -1.0], [1, 0, 1], taken=[2, 3, 0])
    assert list(m.log) == [(0.1 + 0.2, 3, 2, 0), (0.0 + 0.0 + -1.0, 1, 2, 2)] and m.total == 3   # env 1's (1.0, 1, 1, 1) fell out
    assert m.last_return == [0.1 + 0.2, 1.0, -1.0] and m.run_return == [0.0, 0.5, 0.0] and m.run_len == [0, 3, 0]
    m.clear([0, 1, 0], partial=True)
    m.set_quota(1)
    n = m.update([9.0, 9.0, 9.0], [1, 1, 1], skip=[1, 0, 0])
    assert n == 1 and m.dropped == 1 and m.total == 4 and m.retired == [False, False, True] and m.remaining == 2
    assert m.tab_return[0][2] == 9.0 and m.tab_len[0][:2] == [-1, -1] and m.run_return[0] == 0.0 and m.partial == [False] * 3


def test_monitor_symbols_are_exported_and_the_abi_stands():
    from gym_miniworld_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in MONITOR_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert getattr(L, name) is not None
    assert "#define MWB_ABI_VERSION 5" in hdr and L.mwb_abi_version() == 5
    maph = open(os.path.join(CSRC, "mwb_monitor_map.h")).read()
    assert "#define MWB_MONITOR_MAX_CAPACITY %d" % _lib.MONITOR_MAX_CAPACITY in maph
    assert "#define MWB_MONITOR_MAX_QUOTA %d" % _lib.MONITOR_MAX_QUOTA in maph
    # refused without a handle, with a message (the argument refusals of mwb_monitor_enable need a handle, hence a GPU:
    # tests/test_gpu_monitor.py)
    assert L.mwb_monitor_enable(None, 100, 0) == -1 and b"mwb_monitor_enable" in L.mwb_last_error()
    assert L.mwb_monitor_update(None, None, None, None, None, None) == -1
    assert L.mwb_monitor_clear(None, None, 0, None) == -1
    assert L.mwb_monitor_quota(None, 0, None) == -1
    assert L.mwb_monitor_info(None, None) == -1
    assert L.mwb_monitor_read(None, None) == -1
    # struct mwb_monitor_info: 18 pointers, one size, four int32; struct mwb_monitor_counts: what the kernels write
    assert ctypes.sizeof(_lib.MwbMonitorInfo) == 18 * 8 + 8 + 4 * 4
    assert ctypes.sizeof(_lib.MwbMonitorCounts) == 32 and _lib.MwbMonitorCounts.remaining.offset == 16


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_monitor_kernels_use_no_scratch():
    """the build's resource remarks (libmwbatch.resources.txt, as tests/test_kernel_budget.py reads them): the five new kernels
    report 0 bytes of scratch, and only the scan allocates LDS - the wave totals of its sums, a few dozen bytes"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources, remarks_of_the_build
    # (a tree whose library is older than its sources has no remarks to read: the one file is compiled instead, two seconds)
    table = kernel_resources() if remarks_of_the_build() is not None else kernel_resources(src=os.path.join(CSRC, "mwb_monitor.hip"))
    for kernel in ("monitor_accumulate_kernel", "monitor_scan_kernel", "monitor_log_kernel", "monitor_clear_kernel", "monitor_quota_kernel"):
        rows = {n: r for n, r in table.items() if kernel in n}
        assert len(rows) == 1, (kernel, sorted(rows))
        for n, r in rows.items():
            assert r["scratch"] == 0 and r.get("vgpr_spill", 0) == 0, (n, r)
            assert r["lds"] == (48 if kernel == "monitor_scan_kernel" else 0), (n, r)
