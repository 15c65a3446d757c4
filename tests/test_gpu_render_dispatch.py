"""GPU: the compacted work lists of a step's bulk render launch.  prep_kernel(mode 2) sorts the envs of the cost order in use into
those the launch renders (R) and those whose last frame it copies (C); the blocks of the launch find their work through
mwb_dispatch_map (whole frames, the halves of the last min(MWB_SPLIT, R) of them, then the copies).  Nothing of that may show in a
result: every test drives handles with the lists and a twin created under MWB_NO_FRAME_REUSE=1 (every env not regenerated is
rendered) with the same seed and calls; obs (zeroed before the step) and depth must be equal bit for bit, equal a plain render() of
the state the step left, and frame_reuse_stats() must return exactly the crafted (C, R).

R and C are crafted through the poses: an agent touching a wall and facing it is blocked by move_forward (its frame is reused), a
free agent moves (rendered), a turning one is rendered."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCKED, FREE, TURN = 0, 1, 2
FWD, LEFT = 2, 0


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


def make(env_id, n, seed, split=None, no_reuse=False, **kw):
    """MWB_SPLIT and MWB_NO_FRAME_REUSE are read when a handle is created"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    with environ(MWB_SPLIT=None if split is None else str(split), MWB_NO_FRAME_REUSE="1" if no_reuse else None):
        return BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)


def pose(h):
    st = h.get_state()
    n = len(st["agent_dir"])
    return np.concatenate([st["agent_pos"].reshape(n, -1), st["agent_dir"].reshape(n, 1)], axis=1)


def zero_outputs(*handles):
    for h in handles:
        h.obs.zero_()
        if h.depth is not None:
            h.depth.fill_(-1.0)


def assert_same_outputs(a, b, tag):
    import torch
    assert torch.equal(a.obs, b.obs), (tag, "obs", (a.obs != b.obs).reshape(a.num_envs, -1).any(dim=1).nonzero().flatten().tolist()[:8])
    if a.depth is not None:
        assert torch.equal(a.depth, b.depth), (tag, "depth")
    assert torch.equal(a.reward64, b.reward64) and torch.equal(a.done, b.done) and torch.equal(a.ep_steps, b.ep_steps), (tag, "reward / done / ep_steps")


def hallway_poses(n):
    """the hallway is (-1, 11) x (-2, 2), agent radius 0.4, the box in its east end: touching the west wall and facing it (blocked by
    move_forward) / in the middle facing west (free)"""
    z = np.linspace(-1.0, 1.0, n) if n > 1 else np.zeros(1)
    blocked = np.stack([np.full(n, -1.0 + 0.4 + 0.01), z, np.full(n, np.pi)], axis=1)
    free = blocked.copy()
    free[:, 0] = 3.0
    return blocked, free


def settled_poses(handles, n, max_steps=300):
    """any task: move_forward until every agent has run into something (all handles in lock-step: same seed, same state).  Returns
    the poses then (blocked) and the same places facing the other way (free: the agent came from there)"""
    import torch
    fwd = torch.full((n,), FWD, dtype=torch.int32)
    prev = pose(handles[0])
    for t in range(max_steps):
        for h in handles:
            h.step(fwd)
        cur = pose(handles[0])
        stuck = (cur == prev).all(axis=1) & (handles[0].done.cpu().numpy() == 0)
        prev = cur
        if stuck.all():
            break
    assert stuck.all(), "move_forward did not bring every agent up against something"
    free = cur.copy()
    free[:, -1] += np.pi
    return cur[:, [0, 2, 3]], free[:, [0, 2, 3]]


def crafted_step(handles, twin, blocked, free, kinds, tag, regen=None, mes=None):
    """Place every agent by its kind, refresh the frames on record (render()), zero the outputs, step - blocked and free agents with
    move_forward, the others turning - and check every handle against the twin, the counts and a plain render().  regen: envs whose
    step counter is set one short of max_episode_steps `mes`: the step ends their episode and regenerates them (side chain)."""
    import torch
    n = len(kinds)
    kinds = np.asarray(kinds)
    placed = np.where((kinds == FREE)[:, None], free, blocked)
    acts = torch.from_numpy(np.where(kinds == TURN, LEFT, FWD).astype(np.int32))
    regen = np.zeros(n, bool) if regen is None else np.asarray(regen, bool)
    every = list(handles) + [twin]
    for h in every:
        h.set_agent(0, pos_xz=placed[:, :2].copy(), dir=placed[:, 2].copy(), step_count=np.where(regen, (mes or 0) - 1, 0).astype(np.int32))
        h.render()
        h.frame_reuse_stats()
    before = pose(twin)
    zero_outputs(*every)
    for h in every:
        h.step(acts)
    after = pose(twin)
    done = twin.done.cpu().numpy() != 0
    assert (done == regen).all(), (tag, "episodes ended", done.nonzero()[0].tolist(), "meant", regen.nonzero()[0].tolist())
    same = (after == before).all(axis=1)
    assert same[(kinds == BLOCKED) & ~regen].all(), (tag, "a move meant to be blocked was not")
    assert not same[(kinds != BLOCKED) & ~regen].any(), (tag, "an agent meant to move or turn stayed as it was")
    C = int(((kinds == BLOCKED) & ~regen).sum())
    assert twin.frame_reuse_stats() == (0, n), tag
    for h in handles:
        assert_same_outputs(h, twin, tag)
        got = h.frame_reuse_stats()
        assert got == (C, n - C), (tag, "frames (reused, rendered)", got, "crafted", (C, n - C))   # n - C = R + the regenerated ones
        obs_step, dep_step = h.obs.clone(), None if h.depth is None else h.depth.clone()
        zero_outputs(h)
        h.render()
        assert torch.equal(h.obs, obs_step), (tag, "render() != step")
        if dep_step is not None:
            assert torch.equal(h.depth, dep_step), (tag, "render() depth != step")
    return C, n - C - int(regen.sum())


def patterns(n):
    """kinds per env: R = 0, C = 0, and mixtures in both orders (R < MWB_SPLIT whenever MWB_SPLIT >= n)"""
    i = np.arange(n)
    return [("R=0", np.full(n, BLOCKED)), ("C=0 moving", np.full(n, FREE)), ("C=0 turning", np.full(n, TURN)),
            ("thirds", i % 3), ("thirds reversed", (2 - i % 3)), ("one renders", np.where(i == n - 1, TURN, BLOCKED)),
            ("one reused", np.where(i == 0, BLOCKED, FREE))]


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64])
@pytest.mark.parametrize("env_id", ["MiniWorld-Hallway-v0", "MiniWorld-Maze-v0"])
def test_crafted_counts_at_every_split(env_id, n):
    splits = [0, 1, n, n + 3]
    handles = [make(env_id, n, 31, split=s, want_depth=True) for s in splits]
    twin = make(env_id, n, 31, no_reuse=True, want_depth=True)
    for h in handles + [twin]:
        h.reset()
    blocked, free = hallway_poses(n) if "Hallway" in env_id else settled_poses(handles + [twin], n)
    seen = set()
    for name, kinds in patterns(n):
        C, R = crafted_step(handles, twin, blocked, free, kinds, (env_id, n, name))
        seen.add((C == 0, R == 0))
    assert (True, False) in seen and (False, True) in seen   # C = 0 and R = 0 both happened
    if n >= 2:
        assert (False, False) in seen
    for h in handles + [twin]:
        h.close()


@pytest.mark.parametrize("n", [3, 64])
def test_a_step_that_regenerates_some_envs(n):
    """Hallway with a step limit: the envs whose episode the step ends are in neither list - the side chain regenerates and renders
    them - and are counted as rendered"""
    mes = 40
    handles = [make("MiniWorld-Hallway-v0", n, 8, split=s, want_depth=True, max_episode_steps=mes) for s in (0, 2, n)]
    twin = make("MiniWorld-Hallway-v0", n, 8, no_reuse=True, want_depth=True, max_episode_steps=mes)
    for h in handles + [twin]:
        h.reset()
    blocked, free = hallway_poses(n)
    i = np.arange(n)
    for name, kinds, regen in (("one of each, the blocked one ends", i % 3, i % 3 == 0), ("the turning one ends", i % 3, i % 3 == 2),
                               ("every env ends", i % 3, np.ones(n, bool)), ("all blocked, every second ends", np.full(n, BLOCKED), i % 2 == 0)):
        crafted_step(handles, twin, blocked, free, kinds, ("regen", n, name), regen=regen, mes=mes)
    for h in handles + [twin]:
        h.close()


INSTANCES = [
    ("HWC", "MiniWorld-Maze-v0", dict(layout="HWC"), None),
    ("CWH", "MiniWorld-Maze-v0", dict(layout="CWH"), None),
    ("depth", "MiniWorld-Maze-v0", dict(layout="CWH", want_depth=True), None),
    ("fused stack f32", "MiniWorld-Maze-v0", dict(layout="CWH"), "float32"),
    ("fused stack u8", "MiniWorld-Maze-v0", dict(layout="CWH"), "uint8"),
    ("grey", "MiniWorld-Maze-v0", dict(layout="HWC", greyscale=True), None),
    ("grey CWH", "MiniWorld-Maze-v0", dict(layout="CWH", greyscale=True), None),
    ("YMaze (POLY)", "MiniWorld-YMaze-v0", dict(want_depth=True), None),
    ("PutNext (NBOX 6)", "MiniWorld-PutNext-v0", dict(want_depth=True), None),
    ("PickupObjs (entities)", "MiniWorld-PickupObjs-v0", dict(want_depth=True), None),
]


@pytest.mark.parametrize("name,env_id,kw,stack", INSTANCES, ids=[c[0] for c in INSTANCES])
def test_every_render_instantiation_at_three_envs(name, env_id, kw, stack):
    """one env reused, one moving, one turning, through every kernel instantiation and copy-out form; MWB_SPLIT 0, 1 and 3"""
    import torch
    n = 3
    handles = [make(env_id, n, 77, split=s, **kw) for s in (0, 1, 3)]
    twin = make(env_id, n, 77, no_reuse=True, **kw)
    every = handles + [twin]
    for h in every:
        if stack:
            h.stack_enable(4, dtype=stack, fused=True)
        h.reset()
        if stack:
            h.stack_update(after_reset=True)
    blocked, free = settled_poses(every, n)
    for kinds in ([BLOCKED, FREE, TURN], [TURN, BLOCKED, BLOCKED], [BLOCKED, BLOCKED, BLOCKED], [FREE, TURN, BLOCKED]):
        if kw.get("greyscale"):
            for h in every:
                h.grey.fill_(-1.0)
        crafted_step(handles, twin, blocked, free, kinds, (name, kinds))
        for h in handles:
            if kw.get("greyscale"):
                assert torch.equal(h.grey, twin.grey), (name, kinds, "grey")
        if stack:   # crafted_step's render() calls are no step: the windows hold the step's frames
            want = twin.stack_update()
            for h in handles:
                assert torch.equal(h.stack_update(), want), (name, kinds, "window")
    for h in every:
        h.close()


@pytest.mark.parametrize("env_id", ["MiniWorld-Maze-v0", "MiniWorld-FourRooms-v0"])
def test_random_rollout_equals_the_twin(env_id):
    """300 envs, domain randomisation, 40 random steps: the order map is rewritten underneath throughout"""
    import torch
    n = 300
    a = make(env_id, n, 12, domain_rand=True, want_depth=True)
    s = make(env_id, n, 12, split=100, domain_rand=True, want_depth=True)
    b = make(env_id, n, 12, no_reuse=True, domain_rand=True, want_depth=True)
    for h in (a, s, b):
        h.reset()
        h.frame_reuse_stats()
    g = torch.Generator().manual_seed(3)
    for t in range(40):
        acts = torch.where(torch.rand(n, generator=g) < 0.6, torch.full((n,), FWD), torch.randint(0, 2, (n,), generator=g)).to(torch.int32)
        if t % 8 == 7:
            zero_outputs(a, s, b)
        for h in (a, s, b):
            h.step(acts)
        if t % 8 == 7:
            assert_same_outputs(a, b, (env_id, t))
            assert_same_outputs(s, b, (env_id, t, "split 100"))
    reused, rendered = a.frame_reuse_stats()
    assert reused > 0 and reused + rendered == 40 * n and s.frame_reuse_stats() == (reused, rendered)
    for h in (a, s, b):
        h.close()


def test_graph_replay_with_changing_counts():
    """one captured step, replayed 12 times while the actions move R and C from one extreme to the other: the lists and the mapping are
    decided on the device"""
    import torch
    n = 64
    a = make("MiniWorld-Maze-v0", n, 4, want_depth=True)
    b = make("MiniWorld-Maze-v0", n, 4, want_depth=True)
    a.reset(); b.reset()
    settled_poses([a, b], n)
    acts = torch.full((n,), FWD, dtype=torch.int32, device="cuda")
    a.step(acts); b.step(acts)            # eager warm-up, both handles in lock-step (everybody stays blocked)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):             # capture only records; nothing executes
        b.step(acts)
    a.frame_reuse_stats(); b.frame_reuse_stats()
    i = torch.arange(n)
    counts = []
    for t in range(12):
        # turning moves nobody: after a step in which everybody turned, move_forward is blocked for those still facing their wall
        new = [torch.full((n,), FWD), torch.where(i % 2 == 0, FWD, LEFT), torch.where(i % 2 == 0, FWD, 1), torch.full((n,), LEFT),
               torch.full((n,), 1), torch.where(i < t, FWD, LEFT)][t % 6]
        acts.copy_(new.to(torch.int32))
        zero_outputs(a, b)
        a.step(acts)
        g.replay()
        assert_same_outputs(b, a, ("replay", t))
        got = a.frame_reuse_stats()
        assert b.frame_reuse_stats() == got, t
        counts.append(got)
    assert len(set(counts)) >= 3 and any(c[0] == n for c in counts) and any(c[0] == 0 for c in counts), counts
    a.close(); b.close()


def test_65537_envs_a_third_of_them_blocked():
    """the compaction's loop over tiles and the counts at the top of the index range: envs of period 3 (tests/periodic.py) - blocked,
    moving, turning - whose first period is compared with a twin of three envs"""
    import torch
    from periodic import assert_periodic, periodic_actions, periodic_seeds
    n, P = 65537, 3
    kw = dict(want_depth=True, obs_width=16, obs_height=12, layout="CWH")   # 576-byte frames: a handle is a few hundred MB
    big = make("MiniWorld-Hallway-v0", n, None, **kw)
    big.seed(periodic_seeds(n, P, base=50))
    twin = make("MiniWorld-Hallway-v0", P, None, no_reuse=True, **kw)
    twin.seed(periodic_seeds(P, P, base=50))
    big.reset(); twin.reset()
    kinds = np.arange(n) % P   # BLOCKED, FREE, TURN
    blocked, free = hallway_poses(P)
    placed_P = np.where((kinds[:P] == FREE)[:, None], free, blocked)
    placed = placed_P[np.arange(n) % P]
    acts_P = torch.from_numpy(np.where(kinds[:P] == TURN, LEFT, FWD).astype(np.int32))
    big.set_agent(0, pos_xz=placed[:, :2].copy(), dir=placed[:, 2].copy())
    twin.set_agent(0, pos_xz=placed_P[:, :2].copy(), dir=placed_P[:, 2].copy())
    big.render(); twin.render()
    big.frame_reuse_stats()
    zero_outputs(big, twin)
    big.step(periodic_actions(acts_P, n)); twin.step(acts_P)
    C = int((kinds == BLOCKED).sum())
    assert big.frame_reuse_stats() == (C, n - C)
    for what in ("obs", "depth", "reward64", "done", "ep_steps"):
        x = getattr(big, what)
        assert_periodic(x, P, what)
        assert torch.equal(x[:P], getattr(twin, what)), what
    big.close(); twin.close()
