"""CPU: which block of a step's bulk render launch renders or copies which list entry.  The device decides with
mwb_dispatch_map (gym_miniworld_amd/csrc/mwb_dispatch_map.h, called by render_body's MODE 2); here the same header is built into
a small host program - with the host's address and undefined-behaviour sanitizers where the compiler has them - which checks
every launch of up to 12 envs, and whose printed maps are compared with a restatement of the rule in Python."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXIT, RENDER, COPY = 0, 1, 2


@pytest.fixture(scope="module")
def exe():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "dispatch_map_host")
    srcs = [os.path.join(HERE, "dispatch_map_host.cpp"), os.path.join(ROOT, "gym_miniworld_amd", "csrc", "mwb_dispatch_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(srcs[1]), "-o", exe, srcs[0]]
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        r = subprocess.run(base + san, capture_output=True, text=True)
        if r.returncode != 0:
            # without sanitizers only where their runtimes are not installed (the linker cannot find them); any other failure is one
            assert any(w in r.stderr for w in ("libasan", "libubsan", "-lasan", "-lubsan")), r.stderr
            subprocess.check_call(base)
            print("dispatch_map_host: built WITHOUT sanitizers (runtimes not installed)")
        else:
            print("dispatch_map_host: built with -fsanitize=address,undefined")
    return exe


def test_every_launch_of_up_to_12_envs_covers_both_lists_exactly_once(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checked ") and int(r.stdout.split()[1]) > 4000, r.stdout


def restated(n, split, r, c):
    """The rule as the header's comment states it, block by block."""
    grid, s = n + split, min(split, r)
    rows = []
    for b in range(grid):
        if b < r - s:
            rows.append((RENDER, b, -1))
        elif b < r + s:
            rows.append((RENDER, r - s + (b - (r - s)) // 2, (b - (r - s)) % 2))
        elif b - (r + s) < c:
            rows.append((COPY, b - (r + s), -1))
        else:
            rows.append((EXIT, 0, -1))
    return rows


@pytest.mark.parametrize("n,split,r,c", [(8192, 768, 6700, 1440), (8192, 768, 8192, 0), (8192, 768, 0, 8192), (8192, 768, 500, 7000),
                                         (8192, 0, 6000, 2000), (65537, 768, 43691, 21846), (5, 8, 3, 1), (1, 1, 1, 0), (1, 0, 0, 1)])
def test_printed_map_equals_the_rule(exe, n, split, r, c):
    out = subprocess.run([exe, str(n), str(split), str(r), str(c)], check=True, capture_output=True, text=True).stdout
    got = [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    want = restated(n, split, r, c)
    assert len(got) == n + split
    assert [(g[0], g[1] if g[0] != EXIT else 0, g[2] if g[0] == RENDER else -1) for g in got] == want
