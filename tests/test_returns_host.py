"""CPU: the arithmetic of the rollout's returns scan, its host-side index check, ABI and kernel resources.

gym_miniworld_amd/csrc/mwb_returns_scan.h - the discount tables and per-step recurrences mwb_rollout_returns and its kernel share -
is built into a host program (returns_scan_host.cpp) that runs the three scans over columns given on stdin.  Three links:
  (a) the header == tests/returns_ref.py (a NumPy float32 restatement of the specification), bit for bit, with taken in 0 .. 64;
  (b) returns_ref.py with taken == 1 == the reference's loops written with torch CPU float32 tensors and Python-float gamma / tau
      in the expression order of pytorch-a2c-ppo-acktr/storage.py:82-105, bit for bit: this pins the rounding of the scalars
      (G[1] = float32(gamma), L[1] = float32(gamma * tau)) to torch itself on the machine the test runs on;
  (c) the tables' rule.
Magnitudes of all test data lie in [2^-10, 2^10] or are exactly 0 (returns_ref.magnitudes says why no intermediate can then be
subnormal): flush-to-zero settings cannot matter."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import returns_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gym_miniworld_amd", "csrc")
MODES = {"discounted": 0, "gae": 1, "psi": 2}
LEARNER_SYMBOLS = ["mwb_rollout_learner_enable", "mwb_rollout_learner_info", "mwb_rollout_insert", "mwb_rollout_returns", "mwb_rollout_gather_cols"]
GAMMAS = [(0.99, 0.95), (0.9, 1.0), (0.997, 0.5)]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def scan_host():
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "returns_scan_host")
    srcs = [os.path.join(HERE, "returns_scan_host.cpp"), os.path.join(CSRC, "mwb_returns_scan.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        cmd = ["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", exe, srcs[0]]
        # with AddressSanitizer + UBSan where their runtimes link (a stand-alone program: nothing is preloaded), plain otherwise
        if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
            subprocess.check_call(cmd)

    def run(mode, c, gamma, tau):
        T, N = c["reward"].shape
        nxt = np.zeros((N, 2), np.float32)
        if mode == "psi":
            nxt[:] = c["next_psi"]
        else:
            nxt.reshape(-1)[:N] = c["next_value"]
        blob = struct.pack("=iiidd", MODES[mode], T, N, gamma, tau) + b"".join(
            np.ascontiguousarray(c[k]).tobytes() for k in ("reward", "value", "mask", "taken", "feature")) + nxt.tobytes()
        res = subprocess.run([exe], input=blob, capture_output=True)
        assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
        got = np.frombuffer(res.stdout, np.float32)
        sizes = [("ret", (T + 1, N)), ("adv", (T, N)), ("value", (T + 1, N)), ("psi", (T + 1, N, 2)), ("G", (R.MAX_K + 1,)), ("L", (R.MAX_K + 1,))]
        assert got.size == sum(int(np.prod(s)) for _, s in sizes)
        out, at = {}, 0
        for name, shape in sizes:
            n = int(np.prod(shape))
            out[name] = got[at:at + n].reshape(shape)
            at += n
        return out
    return run


@pytest.mark.parametrize("T", [1, 2, 9, 17])
def test_header_equals_the_restatement_bit_for_bit(scan_host, T):
    """(a)"""
    N = 64
    for i, (gamma, tau) in enumerate(GAMMAS):
        c = R.random_case(T, N, seed=1000 * T + i)
        assert c["taken"].min() == 0 and c["taken"].max() == R.MAX_K and set(np.unique(c["mask"])) == {0.0, 1.0}
        ret, adv, value = R.gae(c["reward"], c["value"], c["mask"], c["taken"], c["next_value"], gamma, tau)
        got = scan_host("gae", c, gamma, tau)
        assert (bits(got["ret"]) == bits(ret)).all() and (bits(got["adv"]) == bits(adv)).all() and (bits(got["value"]) == bits(value)).all()
        ret, adv, value = R.discounted(c["reward"], c["value"], c["mask"], c["taken"], c["next_value"], gamma)
        got = scan_host("discounted", c, gamma, tau)
        assert (bits(got["ret"]) == bits(ret)).all() and (bits(got["adv"]) == bits(adv)).all() and (bits(got["value"]) == bits(value)).all()
        want = R.psi(c["feature"], c["mask"], c["taken"], c["next_psi"], gamma)
        got = scan_host("psi", c, gamma, tau)
        assert (bits(got["psi"]) == bits(want)).all()
        # the scan discounted: a different taken gives different returns
        other = R.discounted(c["reward"], c["value"], c["mask"], np.ones_like(c["taken"]), c["next_value"], gamma)[0]
        assert T * N < 3 or (bits(other) != bits(ret)).any()


@pytest.mark.parametrize("T", [1, 2, 9, 17])
def test_restatement_with_taken_one_equals_torch(T):
    """(b): the loops of storage.py:82-105 on torch CPU float32 tensors, Python floats for gamma and tau"""
    import torch
    N = 64
    for i, (gamma, tau) in enumerate(GAMMAS):
        c = R.random_case(T, N, seed=2000 * T + i)
        ones = np.ones_like(c["taken"])
        rewards, masks, features = torch.from_numpy(c["reward"]), torch.from_numpy(c["mask"]), torch.from_numpy(c["feature"])
        next_value, next_psi = torch.from_numpy(c["next_value"]), torch.from_numpy(c["next_psi"])
        # use_gae
        value_preds = torch.from_numpy(c["value"].copy())
        returns = torch.zeros(T + 1, N)
        value_preds[-1] = next_value
        gae = 0
        for step in reversed(range(T)):
            delta = rewards[step] + gamma * value_preds[step + 1] * masks[step + 1] - value_preds[step]
            gae = delta + gamma * tau * masks[step + 1] * gae
            returns[step] = gae + value_preds[step]
        ret, adv, value = R.gae(c["reward"], c["value"], c["mask"], ones, c["next_value"], gamma, tau)
        assert (bits(ret[:-1]) == bits(returns[:-1].numpy())).all() and (bits(value) == bits(value_preds.numpy())).all()
        assert (bits(adv) == bits((returns[:-1] - value_preds[:-1]).numpy())).all()
        # plain discounted returns
        returns = torch.zeros(T + 1, N)
        returns[-1] = next_value
        for step in reversed(range(T)):
            returns[step] = returns[step + 1] * gamma * masks[step + 1] + rewards[step]
        ret, adv, _ = R.discounted(c["reward"], c["value"], c["mask"], ones, c["next_value"], gamma)
        assert (bits(ret) == bits(returns.numpy())).all()
        # successor-feature returns
        psi_returns = torch.zeros(T + 1, N, 2)
        psi_returns[-1] = next_psi
        for step in reversed(range(T)):
            psi_returns[step] = psi_returns[step + 1] * gamma * masks[step + 1].unsqueeze(1).repeat(1, 2) + features[step]
        assert (bits(R.psi(c["feature"], c["mask"], ones, c["next_psi"], gamma)) == bits(psi_returns.numpy())).all()


def test_tables(scan_host):
    """(c)"""
    c = R.random_case(1, 1, seed=3)
    for gamma, tau in GAMMAS + [(1.0, 1.0), (0.5, 0.25)]:
        G, L = R.tables(gamma, tau)
        assert G[0] == 1.0 and L[0] == 1.0
        assert G[1] == np.float32(gamma) and L[1] == np.float32(gamma * tau)
        gd, ld = 1.0, 1.0
        for k in range(R.MAX_K + 1):
            assert G[k] == np.float32(gd) and L[k] == np.float32(ld), k
            gd, ld = gd * gamma, ld * (gamma * tau)
        got = scan_host("gae", c, gamma, tau)
        assert (bits(got["G"]) == bits(G)).all() and (bits(got["L"]) == bits(L)).all()


def test_host_column_index_check():
    from gym_miniworld_amd.batch import check_rollout_column_indices
    T, N = 3, 16
    ok = check_rollout_column_indices([0, 5, 17, 47, 5], T, N)
    assert ok.dtype == np.int64 and ok.tolist() == [0, 5, 17, 47, 5]
    assert check_rollout_column_indices(np.array([[1, 2], [3, 4]], np.int32), T, N).tolist() == [1, 2, 3, 4]
    with pytest.raises(ValueError, match="negative index -1"):
        check_rollout_column_indices([3, -1], T, N)
    with pytest.raises(ValueError, match=r"index 48 outside \[0, 48\)"):   # row T is no transition
        check_rollout_column_indices([47, 48], T, N)
    with pytest.raises(ValueError, match=r"outside \[0, 48\)"):
        check_rollout_column_indices([2 ** 40], T, N)
    for bad in ([0.0, 1.0], [True, False], ["3"], np.zeros(2, np.float32)):
        with pytest.raises(ValueError, match="must be integers"):
            check_rollout_column_indices(bad, T, N)
    for empty in ([], np.zeros((0,), np.int64)):
        with pytest.raises(ValueError, match="empty"):
            check_rollout_column_indices(empty, T, N)


def test_learner_symbols_are_exported_and_the_abi_stands():
    from gym_miniworld_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "miniworld_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = _lib.load()
    for name in LEARNER_SYMBOLS:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert getattr(L, name) is not None
    assert "#define MWB_ABI_VERSION 5" in hdr and L.mwb_abi_version() == 5
    for name in ("DISCOUNTED", "GAE", "PSI"):
        assert "#define MWB_RETURNS_%s %d" % (name, getattr(_lib, "RETURNS_" + name)) in hdr
    assert "#define MWB_RETURNS_MAX_K %d" % _lib.MAX_REPEAT in open(os.path.join(CSRC, "mwb_returns_scan.h")).read()
    # refused without a handle, with a message
    assert L.mwb_rollout_learner_enable(None) == -1 and b"mwb_rollout_learner_enable" in L.mwb_last_error()
    assert L.mwb_rollout_learner_info(None, None) == -1
    assert L.mwb_rollout_insert(None, None, None, None, None, None) == -1
    assert L.mwb_rollout_returns(None, 1, 0.99, 0.95, None, None, None, None) == -1
    assert L.mwb_rollout_gather_cols(None, None, 0, None, None, None, None) == -1
    # struct mwb_rollout_learner_info: 7 pointers, 7 sizes; struct mwb_rollout_info keeps its layout
    assert ctypes.sizeof(_lib.MwbRolloutLearnerInfo) == 14 * 8
    assert ctypes.sizeof(_lib.MwbRolloutInfo) == 10 * 8 + 6 * 4


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="hipcc not available")
def test_learner_kernels_use_no_scratch_and_no_lds():
    """the build's resource remarks (libmwbatch.resources.txt, as tests/test_kernel_budget.py reads them): the four new kernels -
    the scan in its three modes - report 0 bytes of scratch and 0 bytes of LDS"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources, remarks_of_the_build
    # (a tree whose library is older than its sources has no remarks to read: the one file is compiled instead, two seconds)
    table = kernel_resources() if remarks_of_the_build() is not None else kernel_resources(src=os.path.join(CSRC, "mwb_rollout_learner.hip"))
    for kernel, count in (("rollout_returns_kernel", 3), ("rollout_gather_cols_kernel", 1), ("rollout_insert_kernel", 1), ("rollout_taken_kernel", 1)):
        rows = {n: r for n, r in table.items() if kernel in n}
        assert len(rows) == count, (kernel, sorted(rows))
        for n, r in rows.items():
            assert r["scratch"] == 0 and r["lds"] == 0, (n, r)
