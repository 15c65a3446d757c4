"""GPU: the fixed-shape bulk render kernels of the one-box rectangle-room tasks without depth keep a batch of interior pixels' texel
footprints in flight and finish the batch when the wave's next one is due (interior_issue / interior_finish); the
other fixed-shape kernels run the same emit() with the single-call path.  What that can get wrong is a batch that is
never finished, finished twice or finished with another batch's pixels, so every case puts the agents into a directed pose,
STEPS a default handle and an MWB_NO_FIXED=1 twin (render(), reset() and the side stream never run the fixed kernel) with a
turn, and wants obs and depth bit-equal.  obs is zeroed and depth filled with -1 before the step: a lost batch is a block of
untouched pixels.  Every pose runs under both layouts, with and without depth, and with MWB_SPLIT 0, 4 and N (N: every env is
a pair of half-frame workgroups).

The poses are built from each env's own geometry (no world coordinates here):
  nose      0.12 m in front of a wall, square to it: every work item is uniform, 75 interior batches back to back
  corridor  down the longest free axis of a Maze: many 8-sample pixels between the interior batches
  box_near  Hallway's box 1.3 m ahead: the box gate demotes interior pixels, some waves' only batch is their last
  box_far   OneRoom's box seen from the far corner: few 8-sample batches, most of the work in the leftover pooling
  sky       SimToRealPush facing its box: sky and box surfaces (no fetch) beside fetched ones
  boxes     four of PutNext's boxes lined up in front of the agent: three and four distinct surfaces in a pixel"""
import math
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 16
LEFT = 0
TURN = math.radians(15.0)   # turn_step without domain randomisation
POSE_CACHE = {}


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


def make(env_id, fixed, split, n=N, **kw):
    """MWB_NO_FIXED and MWB_SPLIT are read when a handle is created"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    with environ(MWB_NO_FIXED=None if fixed else "1", MWB_SPLIT=str(split)):
        return BatchedMiniWorld(env_id, num_envs=n, seed=33, **kw)


def heading(d):
    return np.array([math.cos(d), -math.sin(d)])


def free_run(segs, p, d):
    """distance from p along heading d to the nearest wall segment (segs [n, 4]: x0 z0 x1 z1)"""
    f, a, sd = heading(d), segs[:, 0:2], segs[:, 2:4] - segs[:, 0:2]
    den = f[0] * sd[:, 1] - f[1] * sd[:, 0]
    w = a - p
    with np.errstate(divide="ignore", invalid="ignore"):
        t, u = (w[:, 0] * sd[:, 1] - w[:, 1] * sd[:, 0]) / den, (w[:, 0] * f[1] - w[:, 1] * f[0]) / den
    hit = (np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1)
    return float(t[hit].min()) if hit.any() else 0.0


def longest_axis(segs, p):
    return max((free_run(segs, p, k * math.pi / 2), k * math.pi / 2) for k in range(4))


def poses(h, kind):
    """-> (pos_xz [n, 2], dir [n], boxes_pos [n, B, 3] or None): the pose the TURN leaves, so dir is given one turn short"""
    st = h.get_state()
    n, B = h.num_envs, h.n_boxes
    pos = st["agent_pos"][:, [0, 2]].copy()
    dirs = st["agent_dir"].copy()
    boxes = st["boxes_pos"].copy() if B else None
    for e in range(n):
        p = pos[e].copy()
        segs = h.get_geometry(e)[1]
        if kind == "nose":
            d = (e % 4) * math.pi / 2
            pos[e] = p + heading(d) * max(0.0, free_run(segs, p, d) - 0.12)
            dirs[e] = d
        elif kind == "corridor":
            dirs[e] = longest_axis(segs, p)[1]
        elif kind == "box_near":
            run, d = longest_axis(segs, p)
            boxes[e, 0, [0, 2]] = p + heading(d) * 1.3   # (nearer than 1.1 m the episode ends and the env regenerates)
            dirs[e] = d
        elif kind == "box_far":
            lo, hi = segs.reshape(-1, 2).min(axis=0) + 0.6, segs.reshape(-1, 2).max(axis=0) - 0.6
            b = boxes[e, 0, [0, 2]]
            p = np.array([lo[0] if b[0] - lo[0] > hi[0] - b[0] else hi[0], lo[1] if b[1] - lo[1] > hi[1] - b[1] else hi[1]])
            pos[e] = p
            dirs[e] = math.atan2(-(b[1] - p[1]), b[0] - p[0])
        elif kind == "sky":
            b = boxes[e, 0, [0, 2]]
            dirs[e] = math.atan2(-(b[1] - p[1]), b[0] - p[0])
        elif kind == "boxes":
            run, d = longest_axis(segs, p)
            v, side = heading(d), np.array([heading(d)[1], -heading(d)[0]])
            for b in range(min(B, 4)):   # 1.6 m apart: two boxes next to each other end PutNext's episode
                boxes[e, b, [0, 2]] = p + v * (1.5 + 1.6 * b) + side * (0.3 * (b % 3 - 1))
            dirs[e] = d
        else:
            raise KeyError(kind)
    return pos, dirs - TURN, boxes


def step_pair(a, b, kind, tag, stack=False):
    """both handles into the pose, one turn, everything compared; returns a's frames"""
    import torch
    assert a.bulk_variant() != b.bulk_variant() and a.bulk_variant() == 1, (tag, a.bulk_variant(), b.bulk_variant())
    for h in (a, b):
        if stack:
            h.stack_enable(4, dtype="float32", fused=True)
        h.reset()
        if stack:
            h.stack_update(after_reset=True)
    key = (b.env_id, kind)
    if key not in POSE_CACHE:   # the worlds depend on the task and the seed only
        POSE_CACHE[key] = poses(b, kind)
    pos, dirs, boxes = POSE_CACHE[key]
    acts = torch.full((a.num_envs,), LEFT, dtype=torch.int32)
    for h in (a, b):
        if boxes is not None:
            h.set_state(0, boxes_pos=boxes)
        h.set_agent(0, pos_xz=pos, dir=dirs, step_count=np.zeros(h.num_envs, np.int32))
        h.frame_reuse_stats()
        h.obs.zero_()
        if h.depth is not None:
            h.depth.fill_(-1.0)
        h.step(acts)
    assert a.frame_reuse_stats() == b.frame_reuse_stats() == (0, a.num_envs), tag   # a turn: every frame is rendered
    # (an env whose episode ended got its frame from the side stream's generic kernel: a few may, where a moved box landed beside another)
    assert int(a.done.sum()) == int(b.done.sum()) <= a.num_envs // 4, (tag, "episodes ended", int(a.done.sum()), int(b.done.sum()))
    bad = (a.obs != b.obs).reshape(a.num_envs, -1).sum(dim=1)
    assert torch.equal(a.obs, b.obs), (tag, "obs: differing bytes per env", bad.tolist())
    if a.depth is not None:
        assert torch.equal(a.depth, b.depth), (tag, "depth")
        assert bool((b.depth > 0).all()), (tag, "the twin left depth untouched somewhere")
    if stack:
        assert torch.equal(a.stack_update(), b.stack_update()), (tag, "window")
    return a.obs


POSES = [
    ("nose", "MiniWorld-Maze-v0"),
    ("corridor", "MiniWorld-Maze-v0"),
    ("box_near", "MiniWorld-Hallway-v0"),
    ("box_far", "MiniWorld-OneRoom-v0"),
    ("sky", "MiniWorld-SimToRealPush-v0"),
    ("boxes", "MiniWorld-PutNext-v0"),
]


@pytest.mark.parametrize("depth", [False, True], ids=["rgb", "depth"])
@pytest.mark.parametrize("layout", ["HWC", "CWH"])
@pytest.mark.parametrize("kind,env_id", POSES, ids=[p[0] for p in POSES])
def test_pipelined_equals_generic(kind, env_id, layout, depth):
    for split in (0, 4, N):
        a = make(env_id, True, split, layout=layout, want_depth=depth)
        b = make(env_id, False, split, layout=layout, want_depth=depth)
        obs = step_pair(a, b, kind, (kind, layout, depth, split))
        if kind == "nose" and depth:   # the pose is what it claims: for most envs nothing but the wall, at arm's length
            far = a.depth.reshape(N, -1).max(dim=1).values
            assert int((far < 0.5).sum()) >= N // 2, (kind, far.tolist())
        assert int(obs.max()) > 0
        a.close(); b.close()


def test_polygon_rooms():
    for split in (0, N):
        a = make("MiniWorld-YMaze-v0", True, split, want_depth=True)
        b = make("MiniWorld-YMaze-v0", False, split, want_depth=True)
        step_pair(a, b, "corridor", ("ymaze", split))
        a.close(); b.close()


def test_fused_float32_stack_window():
    a = make("MiniWorld-Maze-v0", True, 4, layout="CWH")
    b = make("MiniWorld-Maze-v0", False, 4, layout="CWH")
    step_pair(a, b, "corridor", "stack", stack=True)
    a.close(); b.close()
