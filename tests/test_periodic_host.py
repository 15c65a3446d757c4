"""CPU: tests/periodic.py can fail.  A small periodic buffer passes; each of four planted faults - the kinds of damage a wrong env
index or a truncated byte offset does to a large buffer - makes assert_periodic raise, also when the buffer is compared in
several chunks and when it is a strided view."""
import numpy as np
import pytest
import torch

import periodic
from periodic import assert_periodic, periodic_actions, periodic_seeds

P = 13
N, FRAME = 13 * 7 + 5, 36     # 96 envs of 36 bytes: not a whole number of periods
WRAP = 1000                   # the stand-in for 2^32: FRAME does not divide it (as 14 400 does not divide 2^32)


def clean():
    """[N, FRAME] uint8, env i = the frame of env i % P; no frame is zero, no two classes share a frame"""
    cls = torch.arange(P, dtype=torch.int64).reshape(P, 1)
    frames = ((cls * 17 + torch.arange(FRAME, dtype=torch.int64).reshape(1, FRAME) * 3) % 250 + 1).to(torch.uint8)
    assert len({bytes(f.tolist()) for f in frames}) == P and int(frames.min()) > 0
    return frames[torch.arange(N) % P].contiguous()


def unwritten_tail(x):          # (a) the last envs were never written
    x[N - 9:] = 0


def wrapped_offset(x):          # (b) one env's frame went to its byte offset modulo WRAP; its own place keeps what was there before
    env = 61
    assert env * FRAME > WRAP and (env * FRAME) % WRAP % FRAME != 0
    flat = x.reshape(-1)
    frame = flat[env * FRAME:(env + 1) * FRAME].clone()
    flat[env * FRAME:(env + 1) * FRAME] = 0
    at = (env * FRAME) % WRAP
    flat[at:at + FRAME] = frame


def wrong_byte_last_env(x):     # (c)
    x[N - 1, FRAME - 1] ^= 1


def wrong_byte_first_compared(x):   # (d) env P is the first one compared
    x[P, 0] ^= 1


FAULTS = {"unwritten_tail": (unwritten_tail, N - 9), "wrapped_offset": (wrapped_offset, None), "wrong_byte_last_env": (wrong_byte_last_env, N - 1),
          "wrong_byte_env_P": (wrong_byte_first_compared, P)}


@pytest.mark.parametrize("chunk", [periodic.CHUNK_ELEMS, 5 * FRAME, 1])
def test_clean_buffer_passes(chunk, monkeypatch):
    monkeypatch.setattr(periodic, "CHUNK_ELEMS", chunk)
    assert_periodic(clean(), P, "clean")
    assert_periodic(clean().reshape(N, 3, 4, 3), P, "clean 4-d")
    assert_periodic(clean().to(torch.float32), P, "clean float")


@pytest.mark.parametrize("chunk", [periodic.CHUNK_ELEMS, 5 * FRAME, 1])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_found(fault, chunk, monkeypatch):
    monkeypatch.setattr(periodic, "CHUNK_ELEMS", chunk)
    plant, first_env = FAULTS[fault]
    x = clean()
    plant(x)
    assert not torch.equal(x, clean())
    with pytest.raises(AssertionError, match="differs from env") as err:
        assert_periodic(x, P, fault)
    if first_env is not None:   # the report names the first offending env and its byte offset
        assert "env %d differs" % first_env in str(err.value), str(err.value)
    if fault == "wrong_byte_last_env":
        assert "byte offset %d " % (N * FRAME - 1) in str(err.value), str(err.value)
    if fault == "wrong_byte_env_P":
        assert "byte offset %d " % (P * FRAME) in str(err.value), str(err.value)


def test_fault_in_a_strided_view_is_found():
    """the sliding stack's window is a slice of a longer run of planes per env"""
    base = torch.zeros((N, 3 * FRAME), dtype=torch.uint8)
    view = base[:, FRAME:2 * FRAME]
    view.copy_(clean())
    assert not view.is_contiguous()
    assert_periodic(view, P, "view")
    base[N - 1, 0] = 9              # outside the window: not the view's business
    assert_periodic(view, P, "view")
    base[N - 1, 2 * FRAME - 1] ^= 1
    with pytest.raises(AssertionError, match="env %d differs" % (N - 1)):
        assert_periodic(view, P, "view")


def test_a_single_period_is_refused():
    with pytest.raises(AssertionError):
        assert_periodic(clean()[:P], P, "one period")


def test_seeds_and_actions():
    s = periodic_seeds(30, P, base=1000)
    assert s.dtype == np.uint64 and s.shape == (30,)
    assert s[:P].tolist() == list(range(1000, 1000 + P)) and s[P:2 * P].tolist() == s[:P].tolist() and s[26:].tolist() == s[:4].tolist()
    a = np.arange(P, dtype=np.int32) % 3
    full = periodic_actions(a, 30)
    assert full.dtype == np.int32 and full.shape == (30,) and all(full[i] == a[i % P] for i in range(30))
    t = periodic_actions(torch.from_numpy(a).to(torch.int64), 30)
    assert t.dtype == torch.int64 and t.tolist() == full.tolist()
