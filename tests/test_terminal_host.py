"""CPU: terminal observations - the row arithmetic, the host-side argument checks, the info dicts and the kernel's resources.

gym_miniworld_amd/csrc/mwb_terminal_map.h - the functions terminal_rank_kernel, terminal_stack_kernel and the API share - is built
into a host program (terminal_map_host.cpp) that ranks the ended envs of one step and walks the fused stack's window over a run of
passes.  The yardsticks are restatements in Python: the rows are the ended envs in ascending index, cut at the capacity; the
window is a list of frame ids per plane, moved as mwb_api.hip's stack_advance and stack_slide_kernel (mode 3) move it, in which
the planes the program names must hold the frames before the terminal one."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gym_miniworld_amd", "csrc")
TERMINAL_SYMBOLS = ["mwb_terminal_enable", "mwb_terminal_info", "mwb_terminal_dropped", "mwb_rollout_bootstrap"]
SIZES = (1, 5, 255, 256, 257, 1030, 65537)


@pytest.fixture(scope="module")
def map_host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "terminal_map_host")
    srcs = [os.path.join(HERE, "terminal_map_host.cpp"), os.path.join(CSRC, "mwb_terminal_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, srcs[0]]
        # with AddressSanitizer + UBSan where their runtimes link (a stand-alone program: nothing is preloaded), plain otherwise
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)

    def run(flags, capacity, nstack=4, cpf=3, K=36, passes=1):
        text = "%d %d\n%s\n%d %d %d %d\n" % (len(flags), capacity, " ".join(str(int(f)) for f in flags), nstack, cpf, K, passes)
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        return [ln.split() for ln in res.stdout.split("\n") if ln]
    return run


def patterns(N, rng):
    """reset_set patterns of N envs: nobody, everybody (a mass time-out), the first / the last env alone, random at three densities"""
    yield np.zeros(N, bool)
    yield np.ones(N, bool)
    for e in (0, N - 1):
        one = np.zeros(N, bool)
        one[e] = True
        yield one
    for p in (0.01, 0.3, 0.9):
        yield rng.random(N) < p


@pytest.mark.parametrize("N", SIZES)
def test_rows_against_the_restatement(map_host, N):
    rng = np.random.default_rng(N)
    for flags in patterns(N, rng):
        for capacity in sorted({1, min(3, N), N}):
            lines = map_host(flags, capacity)
            ended = np.flatnonzero(flags)                     # ascending env index
            want_rows = ended[:capacity]
            head = [ln for ln in lines if ln[0] == "C"]
            assert head == [["C", str(len(ended)), str(max(0, len(ended) - capacity))]], (N, capacity, head)
            row_of = np.full(N, -1, np.int64)                 # (the program itself fails if an env without a flag has a row)
            for ln in lines:
                if ln[0] == "R":
                    row_of[int(ln[1])] = int(ln[2])
            want_of = np.full(N, -1, np.int64)
            want_of[want_rows] = np.arange(len(want_rows))
            assert (row_of == want_of).all(), (N, capacity)
            row_env = np.array([int(ln[2]) for ln in lines if ln[0] == "E"])
            assert len(row_env) == capacity
            assert (row_env[:len(want_rows)] == want_rows).all() and (row_env[len(want_rows):] == -1).all(), (N, capacity)


def test_the_vec_env_derives_the_same_rows_from_the_causes(map_host):
    from gym_miniworld_amd.vec_env import terminal_infos
    rng = np.random.default_rng(7)
    for N, capacity in ((5, 3), (257, 100), (1030, 1030)):
        cause = rng.integers(0, 4, N).astype(np.uint8) * (rng.random(N) < 0.5)
        trunc, term, row = terminal_infos(cause, capacity)
        lines = map_host(cause != 0, capacity)
        want = np.full(N, -1, np.int64)
        for ln in lines:
            if ln[0] == "R":
                want[int(ln[1])] = int(ln[2])
        assert (row == want).all()
        assert (trunc == (cause == 1)).all() and (term == ((cause == 2) | (cause == 3))).all()


@pytest.mark.parametrize("nstack,cpf,slack", [(4, 3, 8), (4, 1, 8), (2, 3, 8), (1, 3, 8), (16, 1, 8), (3, 3, 1)])
def test_history_planes_over_the_window_slide(map_host, nstack, cpf, slack):
    """every window position of a run that slides back to plane 0 several times: the planes named for history group g of the
    terminal observation of pass p hold frame p - (nstack - 1) + g (nothing before the run's first frame)"""
    C, K = nstack * cpf, nstack * cpf + cpf * slack
    passes = 3 * (slack + 1) + 2
    lines = map_host([1], 1, nstack, cpf, K, passes)
    pos_of = {int(ln[1]): int(ln[2]) for ln in lines if ln[0] == "W"}
    hist = {(int(ln[1]), int(ln[2])): int(ln[3]) for ln in lines if ln[0] == "H"}
    assert len(pos_of) == passes and len(hist) == passes * (nstack - 1)
    planes = [None] * K           # frame id held by every plane of one env
    pos, slides, seen = 0, 0, set()
    for p in range(passes):
        if p:                     # stack_advance for a step
            new = pos + cpf
            if new + C > K:       # stack_slide_kernel mode 3: the history back to the front
                planes[0:C - cpf] = planes[pos + cpf:pos + C]
                new, slides = 0, slides + 1
            pos = new
        assert pos_of[p] == pos, (p, pos_of[p], pos)
        seen.add(pos)
        for g in range(nstack - 1):   # what the terminal pass reads BEFORE the render writes the newest frame
            first = hist[(p, g)]
            want = p - (nstack - 1) + g
            assert pos <= first and first + cpf <= pos + C - cpf
            assert planes[first:first + cpf] == [want if want >= 0 else None] * cpf, (p, g, first, planes)
        planes[pos + C - cpf:pos + C] = [p] * cpf   # the pass's own frame
    assert slides >= 2 and seen == set(range(0, K - C + 1, cpf)), (slides, sorted(seen))


def test_python_argument_checks():
    from gym_miniworld_amd.batch import check_terminal_args
    fused = dict(nstack=4, dtype="float32", sliding=True, fused=True, grey=False)
    assert check_terminal_args(None, 7) == (7, False)
    assert check_terminal_args(3, 7, dtype="float32") == (3, True)
    assert check_terminal_args(np.int64(7), 7, True, fused) == (7, True)
    assert check_terminal_args(1, 7, True, dict(fused, dtype="uint8")) == (1, False)
    with pytest.raises(ValueError, match="auto_reset=False"):
        check_terminal_args(3, 7, auto_reset=False)
    for bad in (0, 8, -1):
        with pytest.raises(ValueError, match=r"outside 1 \.\. num_envs = 7"):
            check_terminal_args(bad, 7)
    for bad in (True, 2.0, "3"):
        with pytest.raises(ValueError, match="must be an integer"):
            check_terminal_args(bad, 7)
    with pytest.raises(ValueError, match="not the fused one"):
        check_terminal_args(3, 7, True, dict(fused, fused=False))
    with pytest.raises(ValueError, match="take the stack's"):
        check_terminal_args(3, 7, True, fused, dtype="uint8")
    with pytest.raises(ValueError, match="dtype must be"):
        check_terminal_args(3, 7, dtype="float16")


def test_lazy_infos_keys_from_plain_arrays():
    from gym_miniworld_amd.vec_env import LazyInfos, terminal_infos
    cause = np.array([0, 1, 2, 3, 1, 0], np.uint8)
    trunc, term, row = terminal_infos(cause, 3)
    assert trunc.tolist() == [False, True, False, False, True, False]
    assert term.tolist() == [False, False, True, True, False, False]
    assert row.tolist() == [-1, 0, 1, 2, -1, -1]          # the fourth ended env is past the capacity
    rows = np.arange(3 * 2).reshape(3, 2) + 100
    skipped = np.array([False] * 5 + [True])
    infos = LazyInfos(6, skipped=skipped, truncated=trunc, terminated=term, terminal_row=row, terminal_obs=rows)
    assert len(infos) == 6 and (infos.truncated == trunc).all() and (infos.terminal_row == row).all()
    assert "TimeLimit.truncated" not in infos[0] and "terminal_observation" not in infos[0]
    assert infos[1]["TimeLimit.truncated"] is True and infos[1]["terminal_observation"].tolist() == [100, 101]
    assert infos[2]["TimeLimit.truncated"] is False and infos[2]["terminal_observation"].tolist() == [102, 103]
    assert infos[3]["TimeLimit.truncated"] is False and infos[3]["terminal_observation"].tolist() == [104, 105]   # clock AND rule: terminal
    assert infos[4]["TimeLimit.truncated"] is True and "terminal_observation" not in infos[4]                      # dropped row
    assert "TimeLimit.truncated" not in infos[5] and infos[5]["feature"].tolist() == [0, 0]                        # the dummy info
    # observations indexed by env (greyscale without a stack)
    by_env = LazyInfos(6, truncated=trunc, terminated=term, terminal_row=row, terminal_obs=np.arange(6) * 10,
                       terminal_index=np.where(cause != 0, np.arange(6), -1))
    assert by_env[4]["terminal_observation"] == 40 and by_env[3]["terminal_observation"] == 30
    # without the feature nothing changes
    assert LazyInfos(2)[0] == {} and LazyInfos(2, taken=np.array([1, 2]))[1] == {"taken": 2}


def test_terminal_symbols_are_exported():
    from gym_miniworld_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in TERMINAL_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert getattr(L, name) is not None
    assert "#define MWB_END_CLOCK %d" % _lib.END_CLOCK in hdr and "#define MWB_END_TASK %d" % _lib.END_TASK in hdr
    assert "#define MWB_TERMINAL_FLOAT %d" % _lib.TERMINAL_FLOAT in hdr
    assert L.mwb_terminal_enable(None, 1, 0) == -1 and b"mwb_terminal_enable" in L.mwb_last_error()
    assert L.mwb_terminal_info(None, None) == -1
    assert L.mwb_terminal_dropped(None, None) == -1
    assert L.mwb_rollout_bootstrap(None, None, 0.99, None) == -1
    assert ctypes.sizeof(_lib.MwbTerminalInfo) == 7 * 8 + 3 * 8 + 4 * 4   # struct mwb_terminal_info
    for cite in ("subproc_vec_env.py:10-13", "miniworld.py:708-711"):
        assert cite in hdr
        assert cite in open(os.path.join(CSRC, "mwb_terminal.hip")).read() and cite in open(os.path.join(CSRC, "mwb_terminal_map.h")).read()


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_terminal_stack_kernel_uses_no_scratch_and_no_lds():
    """every terminal_stack_kernel instantiation of csrc/mwb_terminal.hip reports 0 bytes of scratch and of LDS, and none of the
    file's kernels has scratch: compile-time, hipcc's resource remarks"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    table = {n: r for n, r in kernel_resources(src=os.path.join(CSRC, "mwb_terminal.hip")).items() if "terminal_" in n}
    stacks = [n for n in table if "terminal_stack_kernel" in n]
    assert len(stacks) == 8, sorted(table)   # grey x {16, 4}, float RGB x {16, 4, 1}, uint8 x {16, 4, 1}
    for name in ("terminal_rank_kernel", "terminal_clear_kernel", "terminal_bootstrap_kernel"):
        assert any(name in n for n in table), sorted(table)
    for n, r in table.items():
        assert r["scratch"] == 0, (n, r)
        if "terminal_stack_kernel" in n:
            assert r["lds"] == 0, (n, r)
