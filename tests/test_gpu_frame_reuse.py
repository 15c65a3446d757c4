"""GPU: last-frame reuse.  A step that leaves an env as it was (a blocked move, an env the skip mask leaves out) copies the env's last
frame from the handle's private cache instead of rendering it.  Every test drives a handle with reuse and a twin created under
MWB_NO_FRAME_REUSE=1 with the same seed and actions: after EVERY step obs, depth, reward64, done and ep_steps must be equal bit
for bit - whatever was done to the output buffers in between, whichever entry point changed the state."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


def make_twins(env_id, n, seed, **kw):
    """(handle with reuse, twin without); the switch is read when a handle is created"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    with environ(MWB_NO_FRAME_REUSE=None):
        a = BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)
    with environ(MWB_NO_FRAME_REUSE="1"):
        b = BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)
    return a, b


def assert_twins_equal(a, b, tag):
    import torch
    assert torch.equal(a.obs, b.obs), (tag, "obs", int((a.obs != b.obs).reshape(a.num_envs, -1).any(dim=1).sum()))
    if a.depth is not None:
        assert torch.equal(a.depth, b.depth), (tag, "depth")
    assert torch.equal(a.reward64, b.reward64) and torch.equal(a.done, b.done) and torch.equal(a.ep_steps, b.ep_steps), (tag, "reward / done / ep_steps")


def scribble(*handles):
    """the outputs are the caller's: a step must rewrite every byte of them, reused frame or not"""
    for h in handles:
        h.obs.zero_()
        if h.depth is not None:
            h.depth.fill_(-1.0)


def forward_heavy_actions(rng, n, p_forward=0.6):
    """turn_left / turn_right / move_forward with P(move_forward) = p_forward: an agent that keeps running into walls"""
    return np.where(rng.random(n) < p_forward, 2, rng.integers(0, 2, n)).astype(np.int32)


def pose(st):
    return np.concatenate([st["agent_pos"].reshape(len(st["agent_dir"]), -1), st["agent_dir"].reshape(-1, 1)], axis=1).view(np.uint64)


@pytest.mark.parametrize("layout", ["HWC", "CWH"])
@pytest.mark.parametrize("dr", [0, 1])
def test_maze_blocked_moves_reuse_the_frame_and_equal_the_twin(layout, dr):
    import torch
    n, steps = 256, 80
    a, b = make_twins("MiniWorld-Maze-v0", n, seed=21, domain_rand=bool(dr), want_depth=True, layout=layout)
    a.reset(); b.reset()
    assert_twins_equal(a, b, "reset")
    a.frame_reuse_stats(); b.frame_reuse_stats()
    rng = np.random.default_rng(7)
    prev = pose(a.get_state())
    total = 0
    for t in range(steps):
        acts = torch.from_numpy(forward_heavy_actions(rng, n))
        scribble(a, b)
        a.step(acts); b.step(acts)
        assert_twins_equal(a, b, (layout, dr, t))
        cur = pose(a.get_state())
        unchanged = (cur == prev).all(axis=1) & (a.done.cpu().numpy() == 0)   # pose bit-equal, episode not regenerated
        prev = cur
        reused, rendered = a.frame_reuse_stats()
        print("step %d: reused %d rendered %d, poses unchanged %d" % (t, reused, rendered, int(unchanged.sum())))
        assert reused == int(unchanged.sum()) and reused + rendered == n, (layout, dr, t, reused, rendered, int(unchanged.sum()))
        assert b.frame_reuse_stats() == (0, n)
        total += reused
        if t in (39, 79):   # the step's frames are the frames of the state it left
            obs_step, dep_step = a.obs.clone(), a.depth.clone()
            scribble(a, b)
            a.render(); b.render()
            assert torch.equal(a.obs, obs_step) and torch.equal(a.depth, dep_step), (layout, dr, t, "render() != step")
            assert a.frame_reuse_stats() == (0, 0)   # not a step pass
    assert total > 0
    a.close(); b.close()


@pytest.mark.parametrize("env_id,n_act", [("MiniWorld-PutNext-v0", 6), ("MiniWorld-SimToRealPush-v0", 4)])
def test_carrying_and_pushing_tasks_equal_the_twin(env_id, n_act):
    """pickup, carry, drop (PutNext: a carried box follows every move and turn) and the boxes SimToRealPush shoves about"""
    import torch
    n, steps = 128, 80
    a, b = make_twins(env_id, n, seed=5, want_depth=True)
    a.reset(); b.reset()
    a.frame_reuse_stats()
    rng = np.random.default_rng(3)
    for t in range(steps):
        acts = torch.from_numpy(rng.integers(0, n_act, n).astype(np.int32))
        scribble(a, b)
        a.step(acts); b.step(acts)
        assert_twins_equal(a, b, (env_id, t))
    reused, rendered = a.frame_reuse_stats()
    print(env_id, "reused", reused, "rendered", rendered)
    assert reused + rendered == n * steps
    a.close(); b.close()


# seed of the batch and of the action stream (np.random.default_rng(aseed).integers(0, n_act, (60, 64)), the task's whole action
# range), chosen on the CPU oracle so that some env picks an object up (the step's frame shows it through a render override; the
# state has already lost / respawned it) and bumps into something on the very next step: PickupObjs env 48 at step 9,
# CollectHealth env 43 at step 8.  Reusing the override frame there would show an entity the state no longer has.
@pytest.mark.parametrize("env_id,seed,aseed", [("MiniWorld-PickupObjs-v0", 700, 41), ("MiniWorld-CollectHealth-v0", 700, 0)])
def test_a_blocked_move_after_a_render_override_is_rendered(env_id, seed, aseed):
    import torch
    n, steps = 64, 60
    a, b = make_twins(env_id, n, seed=seed, want_depth=True)
    a.reset(); b.reset()
    a.frame_reuse_stats()
    acts_all = np.random.default_rng(aseed).integers(0, a.n_actions, (steps, n))
    st = a.get_state()
    prev_pose, prev_ovr = pose(st), np.zeros(n, bool)
    prev_count = st["task_i"].copy()
    trapped = 0
    for t in range(steps):
        acts = acts_all[t].astype(np.int32)
        scribble(a, b)
        a.step(torch.from_numpy(acts)); b.step(torch.from_numpy(acts))
        assert_twins_equal(a, b, (env_id, t))
        st = a.get_state()
        done = a.done.cpu().numpy() != 0
        cur = pose(st)
        if a.task == "PickupObjs":
            ovr = st["task_i"] > prev_count            # an object left the list in this step
        else:
            ovr = (st["task_f"] == 100) & (acts == 4)  # a kit was used and respawned (health starts at 100, the step takes 2)
        blocked = np.isin(acts, (2, 3)) & (cur == prev_pose).all(axis=1) & ~done
        trapped += int((prev_ovr & blocked).sum())
        prev_pose, prev_ovr, prev_count = cur, ovr & ~done, st["task_i"].copy()
    reused, rendered = a.frame_reuse_stats()
    print(env_id, "reused", reused, "rendered", rendered, "override then blocked", trapped)
    assert trapped >= 1, "the chosen stream no longer contains an override followed by a blocked move"
    assert reused + rendered == n * steps
    a.close(); b.close()


def test_setters_invalidate_the_cached_frame():
    """set_agent / set_state put the agent against a wall, facing it: the blocked move that follows must show the new place, not
    the frame on record from before the teleport"""
    import torch
    n = 16
    a, b = make_twins("MiniWorld-OneRoom-v0", n, seed=9, want_depth=True)   # the room is (0, 10) x (0, 10), agent radius 0.4
    a.reset(); b.reset()
    fwd = torch.full((n,), 2, dtype=torch.int32)
    a.step(fwd); b.step(fwd)
    a.frame_reuse_stats()
    z = np.linspace(3.0, 7.0, n)
    for k, (x, d) in enumerate(((10.0 - 0.4 - 0.01, 0.0), (0.4 + 0.01, np.pi))):   # touching the east wall facing +x, then the west wall facing -x
        before = a.obs.clone()
        for h in (a, b):
            if k == 0:
                h.set_agent(0, pos_xz=np.stack([np.full(n, x), z], axis=1), dir=np.full(n, d))
            else:
                h.set_state(0, agent_pos=np.stack([np.full(n, x), np.zeros(n), z], axis=1), agent_dir=np.full(n, d))
        placed = pose(a.get_state())
        scribble(a, b)
        a.step(fwd); b.step(fwd)
        assert_twins_equal(a, b, ("teleport", k))
        stayed = (pose(a.get_state()) == placed).all(axis=1) & (a.done.cpu().numpy() == 0)
        assert stayed.sum() >= n // 2, "the move was meant to be blocked"
        assert a.frame_reuse_stats() == (0, n), "a frame from before the setter was reused"
        obs_step, dep_step = a.obs.clone(), a.depth.clone()
        assert int((obs_step != before).reshape(n, -1).any(dim=1).sum()) >= 1
        a.render()
        assert torch.equal(a.obs, obs_step) and torch.equal(a.depth, dep_step), k
        scribble(a, b)
        a.step(fwd); b.step(fwd)   # blocked again, and now the frame on record is the right one
        assert_twins_equal(a, b, ("after teleport", k))
        reused, rendered = a.frame_reuse_stats()
        assert reused >= int(stayed.sum()) - int((a.done.cpu().numpy() != 0).sum()) and reused + rendered == n
    a.close(); b.close()


def test_skip_mask_partial_reset_and_domain_rand_switch():
    import torch
    n = 128
    a, b = make_twins("MiniWorld-Maze-v0", n, seed=33, want_depth=True)
    a.reset(); b.reset()
    a.frame_reuse_stats()
    rng = np.random.default_rng(11)
    skip = torch.zeros(n, dtype=torch.uint8)
    skip[::2] = 1
    for t in range(12):   # half of the envs are not stepped: their frame stands
        acts = torch.from_numpy(forward_heavy_actions(rng, n))
        scribble(a, b)
        a.step(acts, skip_mask=skip); b.step(acts, skip_mask=skip)
        assert_twins_equal(a, b, ("skip", t))
        reused, rendered = a.frame_reuse_stats()
        assert reused >= n // 2 and reused + rendered == n, (t, reused, rendered)
    fwd = torch.full((n,), 2, dtype=torch.int32)
    for t in range(12):   # everybody walks into a wall
        a.step(fwd); b.step(fwd)
    assert_twins_equal(a, b, "forward")
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[n // 2:] = 1
    scribble(a, b)
    a.reset(mask); b.reset(mask)   # a partial reset renders everybody ...
    assert_twins_equal(a, b, "partial reset")
    a.frame_reuse_stats()
    scribble(a, b)
    a.step(fwd); b.step(fwd)       # ... and the blocked step after it reuses the frames of those it left alone
    assert_twins_equal(a, b, "step after partial reset")
    reused, rendered = a.frame_reuse_stats()
    assert reused > 0 and reused + rendered == n
    a.set_domain_rand(True); b.set_domain_rand(True)
    scribble(a, b)
    a.step(fwd); b.step(fwd)
    assert_twins_equal(a, b, "after set_domain_rand")
    assert a.frame_reuse_stats() == (0, n)
    a.close(); b.close()


def test_the_path_without_reset_overlap():
    """MWB_NO_OVERLAP=1: one render launch for everybody, regenerated envs included"""
    import torch
    n, steps = 128, 40
    with environ(MWB_NO_OVERLAP="1"):
        a, b = make_twins("MiniWorld-MazeS3-v0", n, seed=2, want_depth=True, layout="CWH", max_episode_steps=25)
    a.reset(); b.reset()
    a.frame_reuse_stats()
    rng = np.random.default_rng(13)
    for t in range(steps):
        acts = torch.from_numpy(forward_heavy_actions(rng, n))
        scribble(a, b)
        a.step(acts); b.step(acts)
        assert_twins_equal(a, b, ("no overlap", t))
    reused, rendered = a.frame_reuse_stats()
    print("no overlap: reused", reused, "rendered", rendered)
    assert reused > 0 and reused + rendered == n * steps
    a.close(); b.close()


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_fused_frame_stack_windows_equal_the_twin(dtype):
    """4 frames, CWH, written by the render kernels themselves - a reused frame has to enter the window like a rendered one; 24
    steps take the window past its end twice"""
    import torch
    n, steps = 96, 24
    a, b = make_twins("MiniWorld-MazeS3-v0", n, seed=17, layout="CWH", max_episode_steps=15)
    for h in (a, b):
        h.stack_enable(4, dtype=dtype, fused=True)
    a.reset(); b.reset()
    assert torch.equal(a.stack_update(after_reset=True), b.stack_update(after_reset=True))
    a.frame_reuse_stats()
    rng = np.random.default_rng(19)
    for t in range(steps):
        acts = torch.from_numpy(forward_heavy_actions(rng, n))
        scribble(a, b)
        a.step(acts); b.step(acts)
        assert_twins_equal(a, b, (dtype, t))
        assert torch.equal(a.stack_update(), b.stack_update()), (dtype, t, "window")
    reused, rendered = a.frame_reuse_stats()
    assert reused > 0 and reused + rendered == n * steps
    a.close(); b.close()
