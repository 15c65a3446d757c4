"""GPU: the step's bulk render launch compiled for 80 x 60 frames (render_fixed_kernel: size, layout, "has depth" and the
MWB_DEBUG / MWB_EXP words as compile-time constants) against the generic render_kernel.  Nothing of the choice may show in a
result: every test drives a default handle and a twin created under MWB_NO_FIXED=1 with the same seed and the same actions and
wants obs, depth, reward, done, ep_steps, the frame-reuse counters and the fused stack's window equal bit for bit at every step.
MWB_SPLIT=4 at 16 envs gives every launch whole-frame blocks, half-frame blocks and reuse copies."""
import os
from contextlib import contextmanager

import pytest

pytestmark = pytest.mark.gpu

N = 16
FWD = 2


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


def make(env_id, fixed, debug=None, n=N, seed=21, **kw):
    """MWB_NO_FIXED, MWB_SPLIT and MWB_DEBUG are read when a handle is created"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    with environ(MWB_NO_FIXED=None if fixed else "1", MWB_SPLIT="4", MWB_DEBUG=debug):
        return BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)


def random_actions(h, g):
    """mostly move_forward (agents run into walls: reused frames), the task's other actions in between"""
    import torch
    n = h.num_envs
    return torch.where(torch.rand(n, generator=g) < 0.5, torch.full((n,), FWD), torch.randint(0, h.n_actions, (n,), generator=g)).to(torch.int32)


def assert_same(a, b, tag):
    import torch
    assert torch.equal(a.obs, b.obs), (tag, "obs", (a.obs != b.obs).reshape(a.num_envs, -1).any(dim=1).nonzero().flatten().tolist())
    if a.depth is not None:
        assert torch.equal(a.depth, b.depth), (tag, "depth")
    assert torch.equal(a.reward64, b.reward64) and torch.equal(a.reward, b.reward), (tag, "reward")
    assert torch.equal(a.done, b.done) and torch.equal(a.ep_steps, b.ep_steps), (tag, "done / ep_steps")
    if a.grey is not None:
        assert torch.equal(a.grey, b.grey), (tag, "grey")


def lockstep(a, b, steps, tag, stack=False):
    """reset both, then `steps` random steps; everything compared after every step.  Returns the frames (reused, rendered) and the
    number of episodes that ended"""
    import torch
    for h in (a, b):
        if stack:
            h.stack_enable(4, dtype="float32", fused=True)
        h.reset()
        if stack:
            h.stack_update(after_reset=True)
        h.frame_reuse_stats()
    assert_same(a, b, (tag, "reset"))
    g = torch.Generator().manual_seed(5)
    reused = rendered = ended = 0
    for t in range(steps):
        acts = random_actions(a, g)
        for h in (a, b):
            h.obs.zero_()
            if h.depth is not None:
                h.depth.fill_(-1.0)
            h.step(acts)
        assert_same(a, b, (tag, t))
        got = a.frame_reuse_stats()
        assert got == b.frame_reuse_stats(), (tag, t, "frame_reuse_stats")
        reused, rendered, ended = reused + got[0], rendered + got[1], ended + int(a.done.sum())
        if stack:
            assert torch.equal(a.stack_update(), b.stack_update()), (tag, t, "window")
    return reused, rendered, ended


TASKS = [
    ("one box", "MiniWorld-Hallway-v0", {}),
    ("two boxes", "MiniWorld-TMazeTwoBoxDynamic-v0", {}),
    ("six boxes", "MiniWorld-PutNext-v0", {}),
    ("polygon rooms", "MiniWorld-YMaze-v0", {}),
    ("maze, envs regenerate", "MiniWorld-MazeS3-v0", dict(max_episode_steps=7)),
]


@pytest.mark.parametrize("depth", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("layout", ["HWC", "CWH"])
@pytest.mark.parametrize("name,env_id,kw", TASKS, ids=[t[0] for t in TASKS])
def test_fixed_equals_generic(name, env_id, kw, layout, depth):
    a = make(env_id, True, layout=layout, want_depth=depth, **kw)
    b = make(env_id, False, layout=layout, want_depth=depth, **kw)
    assert a.bulk_variant() == 1 and b.bulk_variant() == 0
    reused, rendered, ended = lockstep(a, b, 40, (name, layout, depth), stack=layout == "CWH")
    assert reused + rendered == 40 * N and rendered > 0
    if "regenerate" in name:
        assert ended >= 5 * N   # a step limit of 7: every env was regenerated (side stream) five times
    a.close(); b.close()


GENERIC = [
    ("64 x 48", "MiniWorld-Hallway-v0", dict(obs_width=64, obs_height=48, want_depth=True), None),
    ("MWB_DEBUG=1", "MiniWorld-Hallway-v0", dict(want_depth=True), "1"),
    ("grey", "MiniWorld-Hallway-v0", dict(greyscale=True), None),
    ("entity task", "MiniWorld-PickupObjs-v0", dict(want_depth=True), None),
]


@pytest.mark.parametrize("name,env_id,kw,debug", GENERIC, ids=[c[0] for c in GENERIC])
def test_generic_kernel_where_it_must_be(name, env_id, kw, debug):
    a = make(env_id, True, debug=debug, **kw)
    b = make(env_id, False, debug=debug, **kw)
    assert a.bulk_variant() == 0 and b.bulk_variant() == 0
    lockstep(a, b, 10, name)
    a.close(); b.close()


def test_graph_replay_of_the_fixed_variant():
    """one captured step of a fixed-variant handle, replayed five times against eager steps of its twin"""
    import torch
    a = make("MiniWorld-MazeS3-v0", True, want_depth=True, max_episode_steps=7)
    b = make("MiniWorld-MazeS3-v0", True, want_depth=True, max_episode_steps=7)
    assert a.bulk_variant() == 1 and b.bulk_variant() == 1
    a.reset(); b.reset()
    acts = torch.full((N,), FWD, dtype=torch.int32, device="cuda")
    a.step(acts); b.step(acts)            # eager warm-up, both handles in lock-step
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):         # capture only records; nothing executes
        b.step(acts)
    a.frame_reuse_stats(); b.frame_reuse_stats()
    g = torch.Generator().manual_seed(9)
    for t in range(5):
        acts.copy_(random_actions(a, g))
        for h in (a, b):
            h.obs.zero_()
            h.depth.fill_(-1.0)
        a.step(acts)
        graph.replay()
        assert_same(b, a, ("replay", t))
        assert a.frame_reuse_stats() == b.frame_reuse_stats(), t
    a.close(); b.close()
