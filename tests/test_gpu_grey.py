"""GPU: greyscale observations (mwb_grey_enable / mwb_grey_output / mwb_grey_convert, MWB_STACK_GREY).

The yardstick throughout is grey_ref.py - GreyscaleWrapper.observation + .float() restated in NumPy - applied to the handle's own
`obs`, whose bytes the rest of the suite holds to the oracle.  Every comparison is exact equality of float32 values."""
import ctypes
import os
from contextlib import contextmanager

import numpy as np
import pytest

from grey_ref import grey_of_channels, grey_ref
from stack_ref import FrameStackRef

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4


@contextmanager
def environ(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make(env_id, n, seed, **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    return BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)


def assert_grey_is_f_of_obs(h, tag):
    want = grey_ref(h.obs.cpu().numpy(), h.layout)
    got = h.grey.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32, (tag, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (tag, int(bad.sum()), "pixels differ; first at", tuple(np.argwhere(bad)[0]))


# ------------------------------------------------------------------------------------------------ 1. every colour
@pytest.fixture(scope="module")
def all_colours():
    """all 2^24 RGB triples, pixel i = (R, G, B) = (i & 255, (i >> 8) & 255, i >> 16), and their grey values"""
    i = np.arange(1 << 24, dtype=np.uint32)
    r, g, b = (i & 255).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i >> 16).astype(np.uint8)
    return r, g, b, grey_of_channels(r, g, b)


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
def test_every_colour_converts_exactly(all_colours, layout):
    import torch
    r, g, b, want = all_colours
    h = make("MiniWorld-Hallway-v0", 1, 0)
    if layout == "HWC":
        rgb = np.stack([r, g, b], axis=1).reshape(1, 4096, 4096, 3)
    else:
        rgb = np.stack([r, g, b], axis=0).reshape(1, 3, 4096, 4096)
    out = h.grey_convert(torch.from_numpy(rgb), layout)
    assert out.shape == ((1, 4096, 4096, 1) if layout == "HWC" else (1, 1, 4096, 4096)) and out.dtype == torch.float32
    got = out.cpu().numpy().reshape(-1)
    bad = got != want
    print(layout, "colours that differ:", int(bad.sum()))
    assert not bad.any(), (layout, int(bad.sum()), "first colour", int(np.argmax(bad)))
    h.close()


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
def test_convert_frames_of_any_size(layout):
    """several frames whose pixel count is no multiple of 4 (the pixel-by-pixel path) and frames spanning more than one block"""
    import torch
    h = make("MiniWorld-Hallway-v0", 1, 0)
    rng = np.random.default_rng(5)
    for n, W, H in ((3, 33, 21), (2, 130, 70), (1, 1, 1)):
        rgb = rng.integers(0, 256, (n, H, W, 3) if layout == "HWC" else (n, 3, W, H), dtype=np.uint8)
        got = h.grey_convert(torch.from_numpy(rgb), layout).cpu().numpy()
        assert np.array_equal(got, grey_ref(rgb, layout)), (layout, n, W, H)
    h.close()


# ------------------------------------------------------------------------------------------------ 2. frames
FRAME_ENVS = [("MiniWorld-Hallway-v0", 3), ("MiniWorld-PutNext-v0", 6), ("MiniWorld-YMaze-v0", 3), ("MiniWorld-PickupObjs-v0", 5)]


@pytest.mark.parametrize("size", [(80, 60), (42, 30)])
@pytest.mark.parametrize("layout", ["HWC", "CWH"])
@pytest.mark.parametrize("env_id,n_act", FRAME_ENVS)
def test_grey_frames_equal_f_of_obs_and_nothing_else_changes(env_id, n_act, layout, size):
    """one box, six boxes, polygon rooms, the entity path; 6 envs under MWB_SPLIT=3: one bulk launch holds three whole-frame and
    six half-frame workgroups (rows of a 42 x 30 HWC frame start at r * 42 pixels, columns of a CWH one at x * 30: no multiples
    of 4, so the grey ranges have pixel-by-pixel ends).  The twin without grey gets the same seed and actions."""
    import torch
    n, steps = 6, 24
    W, H = size
    depth = (layout == "HWC") == (W == 80)   # with depth: HWC 80 x 60 and CWH 42 x 30
    kw = dict(layout=layout, obs_width=W, obs_height=H, want_depth=depth)
    with environ(MWB_SPLIT="3"):
        a = make(env_id, n, 11, greyscale=True, **kw)
        b = make(env_id, n, 11, **kw)
    assert a.grey.shape == ((n, H, W, 1) if layout == "HWC" else (n, 1, W, H)) and a.grey.dtype == torch.float32 and b.grey is None

    def check(tag):
        assert_grey_is_f_of_obs(a, tag)
        assert torch.equal(a.obs, b.obs), (tag, "obs")
        assert torch.equal(a.reward64, b.reward64) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), (tag, "reward / done")
        if depth:
            assert torch.equal(a.depth, b.depth), (tag, "depth")

    a.reset(); b.reset()
    check("reset")
    rng = np.random.default_rng(3)
    for t in range(steps):
        acts = torch.from_numpy(rng.integers(0, n_act, n).astype(np.int32))
        a.grey.fill_(-1.0)   # the buffer is rewritten in full by every pass
        a.step(acts); b.step(acts)
        check((env_id, layout, size, t))
    a.grey.fill_(-1.0)
    a.render(); b.render()
    check("render")
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 3. reused and regenerated frames
@pytest.mark.parametrize("no_reuse", [None, "1"])
@pytest.mark.parametrize("layout", ["HWC", "CWH"])
def test_grey_of_reused_and_regenerated_frames(layout, no_reuse):
    """max_episode_steps = 3: every third step regenerates envs on the side stream; the agents are put against the east wall of the
    room facing it and move_forward is held, half of the envs are left out by a skip mask: frames are reused from the cache"""
    import torch
    n, steps = 8, 24
    with environ(MWB_NO_FRAME_REUSE=no_reuse):
        a = make("MiniWorld-OneRoom-v0", n, 9, layout=layout, greyscale=True, max_episode_steps=3)
    a.reset()
    assert_grey_is_f_of_obs(a, "reset")
    a.frame_reuse_stats()
    fwd = torch.full((n,), 2, dtype=torch.int32)
    skip = torch.zeros(n, dtype=torch.uint8)
    skip[1::2] = 1
    reused = rendered = dones = 0
    for t in range(steps):
        if t % 6 == 0:   # the room is (0, 10) x (0, 10), agent radius 0.4: touching the east wall, facing +x
            a.set_agent(0, pos_xz=np.stack([np.full(n, 10.0 - 0.4 - 0.01), np.linspace(3.0, 7.0, n)], axis=1), dir=np.zeros(n))
        a.grey.fill_(-1.0)
        a.step(fwd, skip_mask=skip if t % 2 else None)
        assert_grey_is_f_of_obs(a, (layout, no_reuse, t))
        dones += int(a.done.sum())
        r0, r1 = a.frame_reuse_stats()
        reused, rendered = reused + r0, rendered + r1
    print(layout, no_reuse, "reused", reused, "rendered", rendered, "dones", dones)
    assert dones > 0 and reused + rendered == n * steps
    if no_reuse:
        assert reused == 0
    else:
        assert reused > 0, "no frame was reused: the case proves nothing"
    a.close()


# ------------------------------------------------------------------------------------------------ 4. grey stack
def forward_heavy_actions(rng, n, p_forward=0.6):
    return np.where(rng.random(n) < p_forward, 2, rng.integers(0, 2, n)).astype(np.int32)


@pytest.mark.parametrize("nstack", [1, 4])
@pytest.mark.parametrize("form", ["shifting", "sliding", "fused"])
def test_grey_stack_equals_the_reference_stack(form, nstack):
    """28 steps: the window (nstack + 8 planes) wraps after 9 steps, three times; episodes of 10 steps end on the way; the fused
    form also takes a partial reset"""
    import torch
    from gym_miniworld_amd import _lib
    n, steps = 8, 28
    W, H = 80, 60
    a = make("MiniWorld-MazeS3-v0", n, 17, layout="CWH", greyscale=True, max_episode_steps=10)
    st = a.stack_enable(nstack, "float32", sliding=form != "shifting", fused=form == "fused", grey=True)
    assert st.shape == (n, nstack, W, H) and st.dtype == torch.float32
    first, planes = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(a.L.mwb_stack_window(a.h, ctypes.byref(first), ctypes.byref(planes)))
    assert planes.value == (nstack if form == "shifting" else nstack + _lib.STACK_SLACK_FRAMES) and first.value == 0
    ref = FrameStackRef(n, nstack, (1, W, H))
    f = lambda: torch.from_numpy(grey_ref(a.obs.cpu().numpy(), "CWH"))   # noqa: E731
    a.reset()
    assert torch.equal(a.stack_update(after_reset=True).cpu(), ref.reset(f())), (form, nstack, "reset")
    a.frame_reuse_stats()
    rng = np.random.default_rng(19)
    dones = wraps = 0
    last = 0
    for t in range(steps):
        if form == "fused" and t == 13:   # a step for the window: masked envs start over, the others append their frame once more
            mask = torch.zeros(n, dtype=torch.uint8)
            mask[::3] = 1
            a.reset(mask)
            assert torch.equal(a.stack_update().cpu(), ref.partial_reset(f(), mask)), (form, nstack, "partial reset")
        a.step(torch.from_numpy(forward_heavy_actions(rng, n)))
        got = a.stack_update()
        assert got.shape == (n, nstack, W, H)
        assert torch.equal(got.cpu(), ref.step(f(), a.done.cpu())), (form, nstack, t)
        assert torch.equal(got[:, -1:], a.grey), (form, nstack, t, "newest plane != grey frame")
        dones += int(a.done.sum())
        _lib.check(a.L.mwb_stack_window(a.h, ctypes.byref(first), None))
        wraps += first.value < last
        last = first.value
    reused, rendered = a.frame_reuse_stats()
    print(form, nstack, "dones", dones, "wraps", wraps, "reused", reused)
    assert dones > 0 and (form == "shifting" or wraps >= 2)
    a.close()


@pytest.mark.parametrize("frame_stack", [4, 0])
def test_vec_env_greyscale(frame_stack):
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    n, steps, W, H = 8, 24, 80, 60
    env = MiniWorldVecEnv("MiniWorld-MazeS3-v0", n, seed=4, greyscale=True, frame_stack=frame_stack, max_episode_steps=10)
    k = frame_stack or 1
    assert env.observation_space.shape == (k, W, H) and env.observation_space.dtype == np.float32
    ref = FrameStackRef(n, k, (1, W, H))
    f = lambda: torch.from_numpy(grey_ref(env.batch.obs.cpu().numpy(), "CWH"))   # noqa: E731
    obs = env.reset()
    assert obs.shape == (n, k, W, H) and obs.dtype == torch.float32 and obs.device.type == "cuda"
    assert torch.equal(obs.cpu(), ref.reset(f()))
    rng = np.random.default_rng(23)
    ended = 0
    for t in range(steps):
        acts = torch.from_numpy(forward_heavy_actions(rng, n).astype(np.int64)).unsqueeze(1).to(env.device)
        obs, rew, done, infos = env.step(acts)
        assert torch.equal(obs.cpu(), ref.step(f(), done)), (frame_stack, t)
        ended += int(done.sum())
    assert ended > 0
    env.close()


@pytest.mark.parametrize("frame_stack", [4, 0])
def test_vec_env_greyscale_graph_replay_equals_eager_steps(frame_stack):
    """graph=True: after two eager steps the step - the grey render kernels and, with frame_stack, the shifting grey stack's pass -
    is captured and replayed; observations, rewards and dones equal the eager (fused, sliding) twin's"""
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    n = 8
    a = MiniWorldVecEnv("MiniWorld-MazeS3-v0", n, seed=6, greyscale=True, frame_stack=frame_stack, graph=True, max_episode_steps=5)
    b = MiniWorldVecEnv("MiniWorld-MazeS3-v0", n, seed=6, greyscale=True, frame_stack=frame_stack, graph=False, max_episode_steps=5)
    assert torch.equal(a.reset(), b.reset())
    g = torch.Generator().manual_seed(1)
    ended = 0
    for t in range(12):
        act = torch.randint(0, 3, (n, 1), generator=g)
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and np.array_equal(da, db), (frame_stack, t)
        ended += int(da.sum())
    assert a._graph is not None and b._graph is None and ended > 0
    a.close(); b.close()


def test_vec_env_greyscale_shapes_and_make_vec_envs():
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv, make_vec_envs
    env = MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, seed=1, greyscale=True, transpose=False)
    assert env.observation_space.shape == (60, 80, 1)
    obs = env.reset()
    assert obs.shape == (2, 60, 80, 1) and np.array_equal(obs.cpu().numpy(), grey_ref(env.batch.obs.cpu().numpy(), "HWC"))
    env.close()
    with pytest.raises(AssertionError):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 2, seed=1, greyscale=True, to_float=False)
    env = make_vec_envs("MiniWorld-Hallway-v0", 1, 2, device="cuda:0", greyscale=True)
    assert env.observation_space.shape == (4, 80, 60)
    obs = env.reset()
    assert obs.shape == (2, 4, 80, 60) and obs.dtype == torch.float32
    assert np.array_equal(obs[:, -1:].cpu().numpy(), grey_ref(env.batch.obs.cpu().numpy(), "CWH")) and not obs[:, :-1].any()
    env.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals():
    from gym_miniworld_amd import _lib
    grey = _lib.STACK_GREY
    a = make("MiniWorld-Hallway-v0", 2, 1, layout="CWH")
    L = a.L
    p, nb = ctypes.c_void_p(), ctypes.c_size_t()
    assert L.mwb_grey_output(a.h, ctypes.byref(p), ctypes.byref(nb)) == ESTATE                  # before mwb_grey_enable
    assert L.mwb_stack_enable(a.h, 4, 1 | grey) == ESTATE and b"mwb_grey_enable" in L.mwb_last_error()   # a grey stack without grey
    assert L.mwb_grey_enable(a.h) == 0
    assert L.mwb_grey_enable(a.h) == ESTATE                                                     # already enabled
    assert L.mwb_grey_output(a.h, ctypes.byref(p), ctypes.byref(nb)) == 0 and p.value and nb.value == 2 * 80 * 60 * 4
    assert L.mwb_stack_enable(a.h, 4, 0 | grey) == EINVAL                                       # uint8 grey stack
    assert L.mwb_stack_enable(a.h, 4, 0 | grey | _lib.STACK_FUSED) == EINVAL
    assert L.mwb_stack_enable(a.h, 4, 1 | grey | _lib.STACK_FUSED) == 0
    a.close()
    b = make("MiniWorld-Hallway-v0", 2, 1)
    b.reset()
    assert b.L.mwb_grey_enable(b.h) == ESTATE and b"before the first" in b.L.mwb_last_error()   # after the first reset
    b.close()
    c = make("MiniWorld-Hallway-v0", 2, 1, obs_width=33, obs_height=21)
    assert c.L.mwb_grey_enable(c.h) == EINVAL and b"multiple of 4" in c.L.mwb_last_error()      # W*H % 4 != 0
    c.close()
    with pytest.raises(_lib.MwbError):
        make("MiniWorld-Hallway-v0", 2, 1, obs_width=33, obs_height=21, greyscale=True)
    with environ(MWB_TILE="40x30"):
        d = make("MiniWorld-PickupObjs-v0", 2, 1)
    assert d.L.mwb_grey_enable(d.h) == EINVAL and b"tiles" in d.L.mwb_last_error()              # frames rendered in tiles
    d.close()
