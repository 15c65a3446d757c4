"""CPU: which (destination, source) pairs mwb_copy_envs carries out.  The device decides with the functions of
gym_miniworld_amd/csrc/mwb_copy_check.h (copy_validate_kernel is the only code that reads an unchecked index); here the same
header is built into a small host program that runs the kernel's three passes, and BatchedMiniWorld's host-side check
(batch.check_copy_indices) must agree with it: it raises exactly where the device would reject a pair.  Out-of-range indices
(-1, N, INT32_MAX) are covered here and never sent to a GPU."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INT32_MAX = 2 ** 31 - 1
COPY, IDENT, REJ = 0, 1, 2

# (n_dst, n_src, same_handle, [(dst, src) ...], expected verdict per pair)
CASES = [
    # valid
    ("clone upper half from lower", 8, 8, 1, [(4, 0), (5, 1), (6, 2), (7, 3)], [COPY] * 4),
    ("one pair", 8, 8, 1, [(7, 0)], [COPY]),
    ("fan out: one source, many destinations", 8, 8, 1, [(1, 0), (2, 0), (3, 0)], [COPY] * 3),
    ("identity pairs are valid and copy nothing", 8, 8, 1, [(2, 2), (5, 5)], [IDENT, IDENT]),
    ("an identity pair's env may be another pair's source", 8, 8, 1, [(3, 3), (7, 3)], [IDENT, COPY]),
    ("two handles: destination and source index spaces are separate", 4, 10, 0, [(0, 9), (1, 0), (3, 1), (2, 3)], [COPY] * 4),
    ("two handles: equal indices are a copy, not an identity", 4, 4, 0, [(0, 0), (1, 1), (2, 3), (3, 2)], [COPY] * 4),
    ("two handles: a permutation of everything", 4, 4, 0, [(2, 0), (0, 1), (3, 2), (1, 3)], [COPY] * 4),
    ("first and last env", 96, 96, 1, [(95, 0)], [COPY]),
    # range
    ("destination -1", 8, 8, 1, [(-1, 0), (4, 1)], [REJ, COPY]),
    ("destination N", 8, 8, 1, [(8, 0), (4, 1)], [REJ, COPY]),
    ("destination INT32_MAX", 8, 8, 1, [(INT32_MAX, 0), (4, 1)], [REJ, COPY]),
    ("source -1 / N / INT32_MAX", 8, 8, 1, [(4, -1), (5, 8), (6, INT32_MAX), (7, 0)], [REJ, REJ, REJ, COPY]),
    ("source beyond the smaller source handle", 8, 4, 0, [(0, 4), (1, 3)], [REJ, COPY]),
    ("destination beyond the smaller destination handle", 4, 8, 0, [(4, 0), (3, 7)], [REJ, COPY]),
    ("INT32_MIN", 8, 8, 0, [(-2 ** 31, 0), (0, -2 ** 31)], [REJ, REJ]),
    # duplicates
    ("a destination named twice: both pairs", 8, 8, 1, [(4, 0), (4, 1), (5, 2)], [REJ, REJ, COPY]),
    ("named three times", 8, 8, 0, [(1, 0), (1, 0), (1, 5), (2, 5)], [REJ, REJ, REJ, COPY]),
    ("an identity pair and a copy into the same env", 8, 8, 1, [(3, 3), (3, 0)], [REJ, REJ]),
    ("a pair rejected for its source still counts at its destination", 8, 8, 1, [(4, -1), (4, 0)], [REJ, REJ]),
    # overlap on one handle
    ("a destination that is another pair's source", 8, 8, 1, [(1, 0), (2, 1)], [REJ, COPY]),
    ("a swap", 8, 8, 1, [(0, 1), (1, 0)], [REJ, REJ]),
    ("a chain", 8, 8, 1, [(1, 0), (2, 1), (3, 2)], [REJ, REJ, COPY]),
    ("the same lists on two handles overlap nothing", 8, 8, 0, [(1, 0), (2, 1), (0, 1)], [COPY] * 3),
    ("a pair rejected for its destination still marks its source", 8, 8, 1, [(8, 3), (3, 0)], [REJ, REJ]),
]


@pytest.fixture(scope="module")
def host_check():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "copy_check_host")
    srcs = [os.path.join(HERE, "copy_check_host.cpp"), os.path.join(ROOT, "gym_miniworld_amd", "csrc", "mwb_copy_check.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(srcs[1]), "-o", exe, srcs[0]])

    def run(n_dst, n_src, same, pairs):
        args = [exe, str(n_dst), str(n_src), str(same)] + [str(v) for p in pairs for v in p]
        vals = [int(v) for v in subprocess.run(args, check=True, capture_output=True, text=True).stdout.split()]
        return vals[:-1], vals[-1]
    return run


def test_the_device_predicate_on_the_host(host_check):
    for name, n_dst, n_src, same, pairs, want in CASES:
        got, clean = host_check(n_dst, n_src, same, pairs)
        assert got == want, (name, got, want)
        assert clean == 1, (name, "the scratch arrays were not put back to zero")
    # the verdicts do not depend on the order of the pairs
    rng = np.random.default_rng(5)
    for name, n_dst, n_src, same, pairs, want in CASES:
        perm = rng.permutation(len(pairs))
        got, _ = host_check(n_dst, n_src, same, [pairs[i] for i in perm])
        assert got == [want[i] for i in perm], (name, "permuted")
    # random lists against a restatement of the rules from their text
    for trial in range(200):
        n_dst, n_src = (int(rng.integers(1, 12)),) * 2 if trial % 2 else (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
        same = trial % 2
        pairs = [(int(rng.integers(-2, n_dst + 2)), int(rng.integers(-2, n_src + 2))) for _ in range(int(rng.integers(1, 10)))]
        want = []
        for d, s in pairs:
            ok = 0 <= d < n_dst and 0 <= s < n_src and sum(1 for d2, _ in pairs if d2 == d) == 1
            if ok and same and d == s:
                want.append(IDENT)
                continue
            if ok and same and any(s2 == d and d2 != s2 and 0 <= s2 < n_src for d2, s2 in pairs):
                ok = False
            want.append(COPY if ok else REJ)
        got, clean = host_check(n_dst, n_src, same, pairs)
        assert got == want and clean == 1, (pairs, n_dst, n_src, same, got, want)


def test_check_copy_indices_raises_where_the_device_rejects(host_check):
    from gym_miniworld_amd.batch import check_copy_indices
    for name, n_dst, n_src, same, pairs, want in CASES:
        dst, src = [p[0] for p in pairs], [p[1] for p in pairs]
        for conv in (list, lambda v: np.asarray(v, np.int64), lambda v: np.asarray(v, np.int32)):
            if REJ in want:
                with pytest.raises(ValueError):
                    check_copy_indices(conv(dst), conv(src), n_dst, n_src, bool(same))
            else:
                d, s = check_copy_indices(conv(dst), conv(src), n_dst, n_src, bool(same))
                assert d.dtype == np.int32 and s.dtype == np.int32 and d.tolist() == dst and s.tolist() == src, name
    d, s = check_copy_indices([], [], 8, 8, True)   # nothing to copy is valid
    assert d.size == 0 and s.size == 0
    d, s = check_copy_indices(range(48, 96), range(48), 96, 96, True)
    assert d.tolist() == list(range(48, 96)) and s.tolist() == list(range(48))
    for bad in (([1, 2], [0]), ([[1]], [[0]]), ([1.5], [0])):   # lengths, shapes, non-integers
        with pytest.raises(ValueError):
            check_copy_indices(bad[0], bad[1], 8, 8, True)
    with pytest.raises(ValueError):   # beyond int32 altogether
        check_copy_indices([2 ** 40], [0], 8, 8, False)
