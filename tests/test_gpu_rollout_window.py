"""GPU: the windowed gather (mwb_rollout_window_offsets / mwb_rollout_gather_window / Rollout.gather(augment=...)).

The yardstick is tests/stack_ref.py::FrameStackRef, fed with the cloned batch.obs (or batch.grey) and batch.done of every step as
tests/test_gpu_rollout.py's Driver does, and indexed with numpy by the window rule of include/miniworld_batch.h - never the
rollout's own plain gather (the identity test cross-checks against it and says so).  Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

from test_gpu_rollout import EPISODE, N, Driver, actions, make

pytestmark = pytest.mark.gpu

T = 3
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
EINVAL, ESTATE = -1, -4


def augment(kind, *p, **kw):
    from gym_miniworld_amd.batch import Augment
    return getattr(Augment, kind)(*p, **kw)


def windowed(F, win, offs):
    """F: numpy [B, P, W, H], the plain stacked rows -> [B, P, out_w, out_h] by the rule: the offsets are clamped first, a pixel
    outside the frame is the clamped pixel (border 0) or zero (border 1)"""
    out_w, out_h, border, dx_lo, dx_hi, dy_lo, dy_hi = win
    B, P, W, H = F.shape
    out = np.zeros((B, P, out_w, out_h), F.dtype)
    for b in range(B):
        dx, dy = min(max(int(offs[b][0]), dx_lo), dx_hi), min(max(int(offs[b][1]), dy_lo), dy_hi)
        sx, sy = np.arange(out_w) + dx, np.arange(out_h) + dy
        rows = F[b][:, np.clip(sx, 0, W - 1)][:, :, np.clip(sy, 0, H - 1)]
        if border == 1:
            inside = ((sx >= 0) & (sx < W))[:, None] & ((sy >= 0) & (sy < H))[None, :]
            rows = np.where(inside[None], rows, np.zeros((), F.dtype))
        out[b] = rows
    return out


def clamped(win, offs):
    o = np.asarray(offs, np.int64)
    return np.stack([np.clip(o[:, 0], win[3], win[4]), np.clip(o[:, 1], win[5], win[6])], 1).astype(np.int32)


class World:
    """a staggered Hallway batch, two windows behind it and a third one full: its rollout and, per logical time, what
    FrameStackRef held (numpy)"""

    def __init__(self, form, size, nstack, n=N, steps=T, learner=False):
        import torch
        self.grey = form == "grey"
        self.b = make("MiniWorld-Hallway-v0", n=n, obs_width=size[0], obs_height=size[1], max_episode_steps=EPISODE, greyscale=self.grey)
        self.d = d = Driver(self.b, steps, nstack, grey=self.grey)
        self.ro, self.n, self.steps = d.ro, n, steps
        if learner:
            d.ro.learner_enable()
        rng = np.random.default_rng(101)
        d.reset()
        for w in range(3):
            for _ in range(steps):
                d.step(actions(rng, n))
            if w < 2:
                d.update()   # two after_updates: frames of the window before are read
        assert d.ro.step == steps and d.windows == 2
        self.snap = {t: d.snap[t].cpu().numpy() for t in range(steps + 1)}
        self.total = (steps + 1) * n
        self.dtypes = [torch.float32] if self.grey else [torch.float32, torch.uint8]

    def rows(self, idx, dtype):
        F = np.stack([self.snap[int(i) // self.n][int(i) % self.n] for i in idx])
        return F if "float" in str(dtype) else F.astype(np.uint8)

    def check(self, got, idx, win, offs, dtype, tag):
        import torch
        want = torch.from_numpy(windowed(self.rows(idx, dtype), win, offs))
        assert got.dtype == dtype and tuple(got.shape) == tuple(want.shape), (tag, got.shape, want.shape)
        assert torch.equal(got.cpu(), want), (tag, str(dtype), int((got.cpu() != want).sum()))


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(form, size, nstack):
        key = (form, size, nstack)
        if key not in made:
            made[key] = World(form, size, nstack)
        return made[key]
    yield get
    for w in made.values():
        w.b.close()


CASES = {
    (80, 60): [("shift", 4), ("shift", 61), ("crop", 64, 48), ("crop", 76, 57), ("crop", 80, 60), ("translate", 96, 72), ("center_crop", 64, 48)],
    (10, 6): [("shift", 2), ("crop", 6, 4), ("crop", 4, 3), ("translate", 14, 10), ("crop", 1, 4)],
}
ALL_CASES = [(size, case) for size in CASES for case in CASES[size]]


# ------------------------------------------------------------------------------------- explicit and unclamped offsets
@pytest.mark.parametrize("nstack", [1, 4])
@pytest.mark.parametrize("form", ["rgb", "grey"])
@pytest.mark.parametrize("size,case", ALL_CASES, ids=["%dx%d-%s" % (s + ("_".join(map(str, c)),)) for s, c in ALL_CASES])
def test_explicit_offsets_equal_the_frame_stack(worlds, size, case, form, nstack):
    import torch
    w = worlds(form, size, nstack)
    aug = augment(*case)
    win = aug.bind(*size)
    rng = np.random.default_rng(sum(map(ord, repr((size, case)))))
    idx = rng.permutation(w.total)   # every (t, e) of the window
    offs = np.stack([rng.integers(win[3], win[4] + 1, w.total), rng.integers(win[5], win[6] + 1, w.total)], 1).astype(np.int64)
    offs[:4] = [(win[3], win[5]), (win[3], win[6]), (win[4], win[5]), (win[4], win[6])]   # the four corners of the range
    offs[4] = (0, 0)
    offs[5:11] = [(1000, 1000), (-1000, 1000), (1000, -1000), (-1000, -1000), (I32_MIN, I32_MAX), (I32_MAX, I32_MIN)]   # clamped on the device
    dev_idx = torch.from_numpy(idx).to(w.b.device)
    dev_offs = torch.from_numpy(offs.astype(np.int32)).to(w.b.device)
    for dt in w.dtypes:
        got, used = w.ro.gather(dev_idx, dtype=dt, augment=aug, offsets=dev_offs, return_offsets=True)
        w.check(got, idx, win, offs, dt, (size, case, form, nstack))
        assert used.dtype == torch.int32 and np.array_equal(used.cpu().numpy(), clamped(win, offs))
        # the clamped pairs give the same rows; offsets that live on the host are uploaded
        assert torch.equal(w.ro.gather(dev_idx, dtype=dt, augment=aug, offsets=clamped(win, offs)), got)
    assert aug.calls == 0   # nothing was drawn
    if nstack > 1:   # zero groups occur and stay zero
        ages = w.ro.ages.cpu().numpy()
        assert (ages < nstack - 1).any() and (ages == nstack - 1).any()
        F = w.rows(idx, torch.float32)
        young = np.array([ages[i // N, i % N] == 0 for i in idx])
        C = F.shape[1] // nstack
        assert young.any() and not got.cpu().numpy()[young][:, :C * (nstack - 1)].any()
    assert w.ro.rejected() == 0


def test_bad_offsets_are_refused_on_the_host(worlds):
    import torch
    w = worlds("rgb", (80, 60), 4)
    aug = augment("shift", 4)
    idx = torch.arange(5, device=w.b.device)
    for bad in ([[0, 0]] * 4, [[0.5, 0]] * 5, [0] * 5, torch.zeros((5, 2), dtype=torch.int64, device=w.b.device),
                torch.zeros((5, 3), dtype=torch.int32, device=w.b.device)):
        with pytest.raises(ValueError):
            w.ro.gather(idx, augment=aug, offsets=bad)
    with pytest.raises(ValueError):
        w.ro.gather(idx, offsets=[[0, 0]] * 5)   # offsets without an augment
    with pytest.raises(ValueError, match="bound to 80 x 60"):
        worlds("rgb", (10, 6), 4).ro.gather(idx, augment=aug)
    assert aug.calls == 0


# ------------------------------------------------------------------------------------- offsets drawn on the device
@pytest.mark.parametrize("form,size,nstack,case", [("rgb", (80, 60), 4, ("shift", 4)), ("rgb", (80, 60), 1, ("crop", 64, 48)),
                                                   ("grey", (80, 60), 4, ("translate", 96, 72)), ("rgb", (10, 6), 4, ("crop", 6, 4)),
                                                   ("grey", (10, 6), 1, ("shift", 2)), ("rgb", (80, 60), 4, ("center_crop", 64, 48))])
def test_device_draws_equal_offsets_of(worlds, form, size, nstack, case):
    import torch
    w = worlds(form, size, nstack)
    aug = augment(*case, **({} if case[0] == "center_crop" else {"seed": 7}))
    rng = np.random.default_rng(5)
    idx = np.concatenate([rng.permutation(w.total)[:20], [3, 3, 41, 3]])   # the same index more than once
    dev_idx = torch.from_numpy(idx).to(w.b.device)
    seen = []
    for call in range(3):
        assert aug.calls == call
        got, offs = w.ro.gather(dev_idx, augment=aug, return_offsets=True)
        assert aug.calls == call + 1   # one per call
        want_offs = aug.offsets_of(idx, call=call)
        assert offs.dtype == torch.int32 and np.array_equal(offs.cpu().numpy(), want_offs)
        w.check(got, idx, aug.window, want_offs, torch.float32, (case, call))
        assert torch.equal(got[20], got[21]) and torch.equal(got[20], got[23])   # one index, one draw
        seen.append(want_offs)
    if case[0] != "center_crop":
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    # obs(t) draws for the indices t * N .. t * N + N - 1
    got = w.ro.obs(2, augment=aug)
    w.check(got, np.arange(N) + 2 * N, aug.window, aug.offsets_of(np.arange(N) + 2 * N, call=3), torch.float32, "obs")
    assert aug.calls == 4
    # a host index list is checked on the host first
    with pytest.raises(ValueError):
        w.ro.gather([0, w.total], augment=aug)
    assert aug.calls == 4 and w.ro.rejected() == 0


# ------------------------------------------------------------------------------------- identity: a cross-check, not the yardstick
@pytest.mark.parametrize("form,size", [("rgb", (80, 60)), ("rgb", (10, 6)), ("grey", (80, 60)), ("grey", (10, 6))])
def test_identity_window_equals_the_plain_gather(worlds, form, size):
    import torch
    w = worlds(form, size, 4)
    aug = augment("crop", *size)
    assert aug.bind(*size) == size + (0, 0, 0, 0, 0)
    idx = torch.from_numpy(np.random.default_rng(3).permutation(w.total)).to(w.b.device)
    for dt in w.dtypes:
        assert torch.equal(w.ro.gather(idx, dtype=dt, augment=aug), w.ro.gather(idx, dtype=dt))


# ------------------------------------------------------------------------------------- rejected rows, canaries, errors
@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_rejected_rows_and_canaries(worlds, dtype):
    import torch
    from gym_miniworld_amd import _lib
    w = worlds("rgb", (80, 60), 4)
    b, ro = w.b, w.ro
    dt = getattr(torch, dtype)
    aug = augment("crop", 64, 48)
    win = aug.bind(80, 60)
    idx = np.array([5, -1, w.total - 1, w.total, 0, 2 ** 40, 17, 5], np.int64)
    bad = np.array([1, 3, 5])
    good = np.setdiff1d(np.arange(len(idx)), bad)
    offs = np.array([[16, 12], [I32_MAX, I32_MIN], [0, 0], [3, 3], [7, 5], [I32_MIN, I32_MAX], [16, 0], [0, 12]], np.int64)
    assert ro.rejected() == 0
    dev_idx, dev_offs = torch.from_numpy(idx).to(b.device), torch.from_numpy(offs.astype(np.int32)).to(b.device)
    got = ro.gather(dev_idx, dtype=dt, augment=aug, offsets=dev_offs)
    assert ro.rejected() == 3 and ro.rejected() == 0   # each such row once
    assert not got[bad].any()
    w.check(got[good], idx[good], win, offs[good], dt, "good rows")
    assert got[good].any()
    # through the C ABI into the middle of a larger buffer: the rows before and after keep their canary
    canary = 171
    big = torch.full((10, 12, 64, 48), canary, dtype=dt, device=b.device)
    cwin = _lib.MwbRolloutWindow(*win, 0)
    _lib.check(b.L.mwb_rollout_gather_window(b.h, ctypes.c_void_p(dev_idx.data_ptr()), 8, ctypes.byref(cwin), ctypes.c_void_p(dev_offs.data_ptr()),
                                             ctypes.c_void_p(big[1].data_ptr()), int(dtype == "float32"), b._stream()))
    assert torch.equal(big[1:9], got) and bool((big[0] == canary).all()) and bool((big[9] == canary).all())
    assert ro.rejected() == 3
    # the drawn offsets of a list with rejected rows: any int64 index is hashed
    drawn = torch.full((10, 2), canary, dtype=torch.int32, device=b.device)
    _lib.check(b.L.mwb_rollout_window_offsets(b.h, ctypes.byref(cwin), 7, 3, ctypes.c_void_p(dev_idx.data_ptr()), 8, ctypes.c_void_p(drawn[1].data_ptr()),
                                              b._stream()))
    seeded = augment("crop", 64, 48, seed=7)
    seeded.bind(80, 60)
    assert np.array_equal(drawn[1:9].cpu().numpy(), seeded.offsets_of(idx, call=3)) and bool((drawn[0] == canary).all()) and bool((drawn[9] == canary).all())
    # count == 0 is a no-op
    _lib.check(b.L.mwb_rollout_gather_window(b.h, None, 0, ctypes.byref(cwin), None, None, 1, b._stream()))
    _lib.check(b.L.mwb_rollout_window_offsets(b.h, ctypes.byref(cwin), 0, 0, None, 0, None, b._stream()))
    empty = ro.gather(torch.zeros(0, dtype=torch.int64, device=b.device), dtype=dt, augment=aug)
    assert empty.shape == (0, 12, 64, 48) and ro.rejected() == 0


def test_errors():
    import torch
    from gym_miniworld_amd import _lib
    from test_gpu_rollout import expect
    from test_rollout_window_host import BAD_WINDOWS
    b = make("MiniWorld-Hallway-v0", max_episode_steps=EPISODE)
    ro = b.rollout_enable(2, 4)
    frame_bytes = 80 * 60 * 3
    assert ro.nbytes == (2 + 4) * N * frame_bytes + 3 * N * (1 + 4 + 8) + 2 * N * 4   # a rollout is what it was
    b.reset()
    aug = augment("shift", 4)
    idx = torch.zeros(1, dtype=torch.int64, device=b.device)
    offs = torch.zeros((1, 2), dtype=torch.int32, device=b.device)
    expect(ESTATE, "nothing has been pushed", lambda: ro.gather(idx, augment=aug, offsets=offs))   # before the first push
    ro.push(after_reset=True)
    assert ro.gather(idx, augment=aug).shape == (1, 12, 80, 60)
    assert ro.nbytes == (2 + 4) * N * frame_bytes + 3 * N * (1 + 4 + 8) + 2 * N * 4   # ... also after a windowed gather
    out = torch.empty((1, 12, 80, 60), device=b.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for win, _ in BAD_WINDOWS:   # every limit, through the C ABI
        cwin = _lib.MwbRolloutWindow(*win, 0)
        assert b.L.mwb_rollout_gather_window(b.h, ptr(idx), 1, ctypes.byref(cwin), ptr(offs), ptr(out), 1, b._stream()) == EINVAL, win
        assert b"mwb_rollout_gather_window" in b.L.mwb_last_error()
        assert b.L.mwb_rollout_window_offsets(b.h, ctypes.byref(cwin), 0, 0, ptr(idx), 1, ptr(offs), b._stream()) == EINVAL, win
        assert b"mwb_rollout_window_offsets" in b.L.mwb_last_error()
    cwin = _lib.MwbRolloutWindow(80, 60, 0, -4, 4, -4, 4, 0)
    L = b.L
    assert L.mwb_rollout_gather_window(b.h, None, 1, ctypes.byref(cwin), ptr(offs), ptr(out), 1, b._stream()) == EINVAL
    assert L.mwb_rollout_gather_window(b.h, ptr(idx), 1, ctypes.byref(cwin), None, ptr(out), 1, b._stream()) == EINVAL
    assert L.mwb_rollout_gather_window(b.h, ptr(idx), 1, ctypes.byref(cwin), ptr(offs), None, 1, b._stream()) == EINVAL
    assert L.mwb_rollout_gather_window(b.h, ptr(idx), 1, None, ptr(offs), ptr(out), 1, b._stream()) == EINVAL
    assert L.mwb_rollout_gather_window(b.h, ptr(idx), -1, ctypes.byref(cwin), ptr(offs), ptr(out), 1, b._stream()) == EINVAL
    assert L.mwb_rollout_gather_window(b.h, ptr(idx), 1, ctypes.byref(cwin), ptr(offs), ptr(out), 2, b._stream()) == EINVAL
    assert L.mwb_rollout_gather_window(b.h, ptr(idx), 1, ctypes.byref(cwin), ptr(offs), ctypes.c_void_p(out.data_ptr() + 4), 1, b._stream()) == EINVAL
    two = torch.zeros((2, 2), dtype=torch.int32, device=b.device)
    assert L.mwb_rollout_gather_window(b.h, ptr(idx), 1, ctypes.byref(cwin), ctypes.c_void_p(two.data_ptr() + 4), ptr(out), 1, b._stream()) == EINVAL
    assert L.mwb_rollout_window_offsets(b.h, ctypes.byref(cwin), 0, 0, ptr(idx), 1, ctypes.c_void_p(two.data_ptr() + 4), b._stream()) == EINVAL
    assert L.mwb_rollout_window_offsets(b.h, ctypes.byref(cwin), 0, 0, None, 1, ptr(offs), b._stream()) == EINVAL
    assert L.mwb_rollout_window_offsets(b.h, ctypes.byref(cwin), 0, 0, ptr(idx), -1, ptr(offs), b._stream()) == EINVAL
    assert ro.rejected() == 0
    b.close()

    plain = make("MiniWorld-Hallway-v0")   # no rollout
    assert plain.L.mwb_rollout_gather_window(plain.h, None, 0, ctypes.byref(cwin), None, None, 1, None) == ESTATE
    plain.close()

    g = make("MiniWorld-Hallway-v0", greyscale=True, max_episode_steps=EPISODE)
    gro = g.rollout_enable(2, 4, grey=True)
    g.reset()
    gro.push(after_reset=True)
    expect(EINVAL, "float32", lambda: gro.obs(0, dtype=torch.uint8, augment=augment("shift", 4)))   # uint8 from a grey ring
    g.close()


# ------------------------------------------------------------------------------------- minibatches
def test_minibatch_and_generator():
    import torch
    w = World("rgb", (80, 60), 4, learner=True)
    ro, b = w.ro, w.b
    rng = np.random.default_rng(9)
    adv = torch.from_numpy(rng.standard_normal((T, N)).astype(np.float32)).to(b.device)
    ro.action_log_probs.copy_(torch.from_numpy(rng.standard_normal((T, N)).astype(np.float32)))
    ro.returns.copy_(torch.from_numpy(rng.standard_normal((T + 1, N)).astype(np.float32)))
    aug, twin = augment("shift", 4, seed=11), augment("shift", 4, seed=11)
    idx = torch.from_numpy(rng.permutation(T * N)[:13]).to(b.device)
    plain = ro.minibatch(idx, adv)
    got = ro.minibatch(idx, adv, augment=aug)
    assert aug.calls == 1
    assert torch.equal(got[0], ro.gather(idx, augment=twin)) and twin.calls == 1   # the same call number
    w.check(got[0], idx.cpu().numpy(), aug.window, aug.offsets_of(idx.cpu().numpy(), call=0), torch.float32, "minibatch")
    for x, y in zip(plain[1:], got[1:]):   # the six columns are unchanged
        assert torch.equal(x, y)
    assert not torch.equal(plain[0], got[0])

    # one pass: 48 rows in minibatches of 48 // 5 = 9, one call number throughout
    c0 = aug.calls
    perm = torch.randperm(T * N, device=b.device, generator=torch.Generator(device=b.device).manual_seed(21)).cpu().numpy()
    seen = []
    batches = list(enumerate(ro.feed_forward_generator(adv, 5, generator=torch.Generator(device=b.device).manual_seed(21), augment=aug)))
    plain_batches = list(ro.feed_forward_generator(adv, 5, generator=torch.Generator(device=b.device).manual_seed(21)))
    assert len(batches) == len(plain_batches) == 6
    for (j, batch), pb in zip(batches, plain_batches):
        first = 9 * j
        part = perm[first:first + 9]
        seen.extend(part.tolist())
        w.check(batch[0], part, aug.window, aug.offsets_of(part, call=c0), torch.float32, ("generator", first))
        assert batch[1] is None and all(torch.equal(x, y) for x, y in zip(batch[2:], pb[2:]))   # the permutation and the cut are as before
    assert sorted(seen) == list(range(T * N))   # every transition exactly once
    assert aug.calls == c0 + 1
    # the calls counter moves when the pass is exhausted, not before
    it = ro.feed_forward_generator(adv, 5, augment=aug)
    next(it)
    assert aug.calls == c0 + 1
    for _ in it:
        pass
    assert aug.calls == c0 + 2 and ro.rejected() == 0
    b.close()


# ------------------------------------------------------------------------------------- a frame larger than a CU's LDS
def test_large_frame():
    import torch
    w = World("rgb", (320, 240), 1, n=2, steps=1)
    assert 320 * 240 * 3 > 160 * 1024
    rng = np.random.default_rng(15)
    idx = np.arange(w.total)
    dev_idx = torch.from_numpy(idx).to(w.b.device)
    for case in (("shift", 8), ("crop", 256, 192)):
        aug = augment(*case)
        win = aug.bind(320, 240)
        offs = np.stack([rng.integers(win[3], win[4] + 1, w.total), rng.integers(win[5], win[6] + 1, w.total)], 1)
        offs[0], offs[1] = (win[3], win[6]), (win[4], win[5])
        for dt in w.dtypes:
            got = w.ro.gather(dev_idx, dtype=dt, augment=aug, offsets=offs)
            w.check(got, idx, win, offs, dt, case)
        got, drawn = w.ro.gather(dev_idx, augment=aug, return_offsets=True)
        w.check(got, idx, win, aug.offsets_of(idx, call=0), torch.float32, case)
    assert w.ro.rejected() == 0
    w.b.close()
