"""CPU: level sets - the seed arithmetic, the level rules, the host-side argument checks, the info dicts and the kernels' resources.

gym_miniworld_amd/csrc/mwb_levels_map.h - the functions levels_assign_kernel runs per lane and mwb_seed runs per env - is built into
a host program (levels_host.cpp) that answers one request per line.  The yardsticks: hashlib for SHA-512, the oracle's
seed_to_mt_key for the key, NumPy's own RandomState.seed(list) for init_by_array, and batch.level_of - Python integers - for the
rules."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gym_miniworld_amd", "csrc")
LEVELS_SYMBOLS = ["mwb_levels_enable", "mwb_levels_restart", "mwb_levels_info", "mwb_levels_rejected"]
EDGE_SEEDS = [0, 1, 9, 10, 99, 2 ** 32 - 1, 2 ** 32, 10 ** 19, 2 ** 64 - 1]
SEEDS = EDGE_SEEDS + [int(x) for x in np.random.default_rng(512).integers(0, 2 ** 64, 1000, dtype=np.uint64)]


@pytest.fixture(scope="module")
def host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "levels_host")
    srcs = [os.path.join(HERE, "levels_host.cpp"), os.path.join(CSRC, "mwb_levels_map.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, srcs[0]]
        # with AddressSanitizer + UBSan where their runtimes link (a stand-alone program: nothing is preloaded), plain otherwise
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        out_lines = [ln.split() for ln in res.stdout.split("\n") if ln]
        assert len(out_lines) == len(lines)
        return out_lines
    return run


@pytest.fixture(scope="module")
def digests(host):
    return host(["D %d" % s for s in SEEDS])


def numpy_row(key):
    rs = np.random.RandomState()
    rs.seed(list(key))
    st = rs.get_state()
    return [int(x) for x in st[1]] + [int(st[2])]


def test_sha512_against_hashlib(digests):
    for s, ln in zip(SEEDS, digests):
        assert ln[0] == hashlib.sha512(str(s).encode()).hexdigest(), s


def test_key_against_the_oracle(digests, oracle_mod):
    for s, ln in zip(SEEDS, digests):
        key = oracle_mod.seed_to_mt_key(s)
        assert int(ln[3]) == len(key) and [int(ln[1]), int(ln[2])][:len(key)] == [int(k) for k in key], s


def test_init_by_array_against_numpy(host, digests):
    keys = [(int(ln[1]), int(ln[2])) for ln in digests[:40]]
    assert all(k[1] != 0 for k in keys)   # (a zero high limb has probability 2^-32: the length-1 path is forced below)
    rows = host(["R %d %d 2" % k for k in keys] + ["R %d 7 1" % k[0] for k in keys] + ["R 0 0 1", "R 4294967295 4294967295 2"])
    want = [numpy_row(k) for k in keys] + [numpy_row(k[:1]) for k in keys] + [numpy_row([0]), numpy_row([2 ** 32 - 1] * 2)]
    for got, w in zip(rows, want):
        assert len(got) == 625 and [int(x) for x in got] == w
        assert w[624] == 624 and w[0] == 0x80000000


def test_rows_against_what_mwb_seed_writes(host):
    """mwb_seed's own path: the library's mwb_seed_key (the key mwb_seed hashes an env's seed to), then init_by_array - NumPy's"""
    from gym_miniworld_amd import _lib, build
    build.build()
    L = _lib.load()
    L.mwb_seed_key.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    seeds = EDGE_SEEDS + SEEDS[9:29]
    rows = host(["Q %d" % s for s in seeds])
    for s, got in zip(seeds, rows):
        key = (ctypes.c_uint32 * 2)()
        n = L.mwb_seed_key(s, key)
        assert n in (1, 2)
        assert [int(x) for x in got] == numpy_row(list(key)[:n]), s


GRID_L = [1, 2, 7, 70, 1000, 2 ** 22, 2 ** 31 - 1]
GRID_G = [0, 1, 69, 8191, 2 ** 31, 2 ** 40 - 1, 2 ** 40 + 12345]
GRID_N = [0, 1, 2, 15, 2 ** 32 - 1, 2 ** 40, 2 ** 40 + 77]
GRID_STRIDE = [1, 7, 70, 8192, 2 ** 31, 2 ** 40 + 3]   # also stride > L
GRID_SEED = [0, 1, 12345, 2 ** 63 + 5]


def test_rules_against_level_of(host):
    from gym_miniworld_amd.batch import level_of
    cases = []
    for L in GRID_L:
        for g in GRID_G:
            for n in GRID_N:
                for stride in GRID_STRIDE:
                    cases.append((0, g, n, L, stride, 0, -1))
                for seed in GRID_SEED:
                    cases.append((1, g, n, L, 1, seed, -1))
                    for req in (-1, 0, L - 1, L, -5, 2 ** 31 - 1, -2 ** 31):
                        cases.append((2, g, n, L, 1, seed, req))
    got = host(["C %d %d %d %d %d %d %d" % c for c in cases])
    for c, ln in zip(cases, got):
        mode, g, n, L, stride, seed, req = c
        assert int(ln[0]) == level_of(mode, g, n, L, stride, seed, req), c
        assert int(ln[1]) == int(mode == 2 and req != -1 and not 0 <= req < L), c
    # the branch-free modulo on its own, and the seed of a level: uint64 arithmetic
    xs = [0, 1, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62 - 1, 2 ** 64 - 1] + [int(x) for x in np.random.default_rng(3).integers(0, 2 ** 64, 50, dtype=np.uint64)]
    mods = [(x, L) for x in xs for L in GRID_L + [3, 2 ** 31 - 2]]
    for (x, L), ln in zip(mods, host(["M %d %d" % m for m in mods])):
        assert int(ln[0]) == x % L, (x, L)
    assert [int(ln[0]) for ln in host(["S 0 0", "S 5 100", "S 2147483646 18446744073709551615"])] == [0, 105, 2 ** 31 - 3]


@pytest.mark.parametrize("q,stride", [(1, 70), (3, 70), (5, 7), (2, 8192)])
def test_sequential_visits_every_level_once(host, q, stride):
    L = q * stride
    got = host(["C 0 %d %d %d %d 0 -1" % (g, n, L, stride) for n in range(q) for g in range(stride)])
    assert sorted(int(ln[0]) for ln in got) == list(range(L))


@pytest.mark.parametrize("seed", GRID_SEED)
def test_uniform_counts_within_six_sigma(host, seed):
    """the three samples of 65 536 draws (a 4096 x 16 grid of (g, n), one env's stream, one episode number across envs): every
    level's count within 6 standard deviations of its binomial expectation"""
    Ls = [1, 2, 7, 16, 1000]
    got = host(["U %d %d %d" % (seed, L, kind) for L in Ls for kind in range(3)])
    k = 0
    for L in Ls:
        for kind in range(3):
            counts = np.array([int(x) for x in got[k]], dtype=np.float64)
            k += 1
            assert len(counts) == L and counts.sum() == 65536
            p = 1.0 / L
            mean, sd = 65536 * p, np.sqrt(65536 * p * (1 - p))
            worst = np.abs(counts - mean).max()
            print("seed %d L %d sample %d: worst deviation %.2f sd" % (seed, L, kind, worst / sd if sd else 0.0))
            assert worst <= 6 * sd, (seed, L, kind, worst, sd)


def test_python_argument_checks():
    from gym_miniworld_amd.batch import check_levels_args, level_of
    assert check_levels_args(7, num_envs=70)[0::3] == (7, 1, 70)                 # uniform, stride = num_envs
    L, start, table, mode, sseed, tally, stride = check_levels_args(3, 2 ** 64 - 1, [5, 2 ** 64 - 1, 0], "sequential", 9, False, 4)
    assert (L, start, mode, sseed, tally, stride) == (3, 2 ** 64 - 1, 0, 9, False, 4)
    assert table.dtype == np.uint64 and table.tolist() == [5, 2 ** 64 - 1, 0]
    assert check_levels_args(np.int64(2 ** 31 - 1), tally=False)[0] == 2 ** 31 - 1
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match=r"outside 1 \.\. 2\^31 - 1"):
            check_levels_args(bad, tally=False)
    for bad in (True, 2.0, "3", None):
        with pytest.raises(ValueError, match="must be an integer"):
            check_levels_args(bad)
    with pytest.raises(ValueError, match="4 seeds for num_levels = 3"):
        check_levels_args(3, seeds=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="outside uint64"):
        check_levels_args(2, seeds=[1, 2 ** 64])
    with pytest.raises(ValueError, match="outside uint64"):
        check_levels_args(2, seeds=[1, -1])
    with pytest.raises(ValueError, match="outside uint64"):
        check_levels_args(2, start_level=-1)
    with pytest.raises(ValueError, match="mode must be one of"):
        check_levels_args(2, mode="random")
    with pytest.raises(ValueError, match="mode must be one of"):
        check_levels_args(2, mode=3)
    with pytest.raises(ValueError, match="env_stride 0 < 1"):
        check_levels_args(2, env_stride=0)
    with pytest.raises(ValueError, match="at most 2\\^22 levels"):
        check_levels_args(2 ** 22 + 1)
    assert check_levels_args(2 ** 22)[0] == 2 ** 22
    # the VecEnv refuses before anything is created (no GPU is touched: these raise on a machine without one)
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    with pytest.raises(ValueError, match="graph=True"):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, num_levels=7, graph=True)
    with pytest.raises(ValueError, match="outside 1"):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, num_levels=-3)
    with pytest.raises(ValueError, match="mode must be one of"):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, num_levels=7, level_mode="shuffle")
    assert level_of("table", 0, 0, 7, request=3) == 3 and level_of("table", 0, 0, 7, request=7) == level_of("uniform", 0, 0, 7)
    assert level_of("sequential", 69, 2, 7, stride=70) == (69 + 140) % 7


def test_lazy_infos_keys_from_plain_arrays():
    from gym_miniworld_amd.vec_env import LazyInfos, level_infos
    pair = np.array([[2, 0, -1, 1], [1, -1, -1, 2]], np.int32)
    dones = np.array([True, True, False, False])
    kw = level_infos(pair, dones, start_level=100)
    assert kw["level"].tolist() == [2, 0, -1, 1] and kw["prev_level"].tolist() == [1, -1, -1, 2]
    infos = LazyInfos(4, **kw)
    assert infos.level_seed.tolist() == [102, 100, 0, 101] and infos.level_seed.dtype == np.uint64
    assert infos.prev_level_seed.tolist() == [101, 0, 0, 102]
    assert (infos.level == pair[0]).all() and (infos.prev_level == pair[1]).all()
    assert infos[0] == {"level_seed": 102, "prev_level_seed": 101}
    assert infos[1] == {"level_seed": 100, "prev_level_seed": None}     # ended, but its level was not known
    assert infos[2] == {"level_seed": None} and infos[3] == {"level_seed": 101}
    assert type(infos[0]["level_seed"]) is int
    # a table, with seeds beyond int64; start_level wraps mod 2^64
    kw = level_infos(pair, dones, seeds=[7, 2 ** 64 - 1, 2 ** 63])
    assert LazyInfos(4, **kw)[0] == {"level_seed": 2 ** 63, "prev_level_seed": 2 ** 64 - 1}
    assert LazyInfos(4, **level_infos(pair, dones, start_level=2 ** 64 - 1)).level_seed.tolist() == [1, 2 ** 64 - 1, 0, 0]
    assert LazyInfos(2).level_seed is None
    # a skipped env keeps the dummy info; without level sets nothing changes
    assert LazyInfos(4, skipped=np.array([True, False, False, False]), **kw)[0]["feature"].tolist() == [0, 0]
    assert LazyInfos(2)[0] == {}


def test_levels_symbols_are_exported():
    from gym_miniworld_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in LEVELS_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert getattr(L, name) is not None
    assert "#define MWB_ABI_VERSION 5" in hdr and _lib.ABI_VERSION == 5 and L.mwb_abi_version() == 5
    for name, val in (("SEQUENTIAL", _lib.LEVELS_SEQUENTIAL), ("UNIFORM", _lib.LEVELS_UNIFORM), ("TABLE", _lib.LEVELS_TABLE)):
        assert re.search(r"#define MWB_LEVELS_%s\s+%d\b" % (name, val), hdr), name
    assert re.search(r"#define MWB_LEVELS_TALLY\s+%du" % _lib.LEVELS_TALLY, hdr)
    assert L.mwb_levels_enable(None, 7, 0, None, 1, 0, 0, 1, 0) == -1 and b"mwb_levels_enable" in L.mwb_last_error()
    assert L.mwb_levels_restart(None, 1, 0, 0, None) == -1
    assert L.mwb_levels_info(None, None) == -1
    assert L.mwb_levels_rejected(None, None) == -1
    assert ctypes.sizeof(_lib.MwbLevelsInfo) == 6 * 8 + 5 * 8 + 2 * 4   # struct mwb_levels_info
    maph = open(os.path.join(CSRC, "mwb_levels_map.h")).read()
    for cite in ("num_levels", "start_level", "env.seed("):
        assert cite in hdr and cite in maph and cite in open(os.path.join(CSRC, "mwb_levels.hip")).read()
    # mwb_api.hip keeps no second copy of the seed arithmetic
    api = open(os.path.join(CSRC, "mwb_api.hip")).read()
    assert "0x428a2f98d728ae22" not in api and "1812433253" not in api and "mwb_levels_seed_key" in api


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_levels_kernels_use_no_scratch_and_spill_no_sgprs():
    """every kernel of csrc/mwb_levels.hip reports 0 bytes of scratch and 0 SGPR spills, the assign kernel no LDS either:
    compile-time, hipcc's resource remarks under the build's own flags"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources
    table = {n: r for n, r in kernel_resources(src=os.path.join(CSRC, "mwb_levels.hip"), extra_flags=["-fno-slp-vectorize"]).items() if "levels_" in n}
    for name in ("levels_assign_kernel", "levels_restart_kernel", "levels_copy_kernel"):
        assert sum(name in n for n in table) == 1, sorted(table)
    for n, r in table.items():
        assert r["scratch"] == 0 and r["sgpr_spill"] == 0 and r["vgpr_spill"] == 0, (n, r)
        if "levels_assign_kernel" in n:
            assert r["lds"] == 0, (n, r)
