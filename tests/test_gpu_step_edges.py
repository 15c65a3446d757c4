"""GPU: single steps at the decision edges of MiniWorldEnv.step against the reference's own outcomes
(tests/golden/stepedge_<task>.npz; tests/step_edges.py builds the start states, tests/test_oracle_step_edges.py says what the
files hold and pins the oracle to them).  One handle per (task, world seed): every env gets the world's seed, one reset, one
set_state with the cases' start states, one step with the per-case action vector - and agent pose, every entity's pose,
carrying, step count, reward64, done, ep_steps, goal_pos and the entity tasks' list / counters are the fixture's bit for bit.
The handles do not reset themselves (auto_reset=False), so that a case that ends its episode keeps its pose.  Every task runs
as step(), as step_repeat(repeat=1) and with a skip_mask that leaves every other case out (those stay as they were set); and
mwb_intersect answers at every decisive point what MiniWorldEnv.intersect answered there."""
import os

import numpy as np
import pytest

import step_edges as SE

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def make_handle(task, seed, n):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    env_id, _, _, args = SE.SPEC[task]
    b = BatchedMiniWorld(env_id, num_envs=n, seed=None, auto_reset=False, task_args=args)
    b.seed(np.full(n, seed, np.uint64))
    return b


def put_start(b, st):
    b.set_state(0, agent_pos=st["agent_pos"], agent_dir=st["agent_dir"], boxes_pos=st["ents_pos"], boxes_dir=st["ents_dir"],
                carrying=st["carrying"], step_count=st["step_count"])


def assert_outcome(b, w, rows, tag):
    """envs `rows` (bool [n]) hold the fixture's outcome"""
    out, st = w["out"], b.get_state()
    E = out["ents_pos"].shape[1]
    eq = lambda x, y: np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()   # noqa: E731

    def check(name, got, want):
        got, want = np.asarray(got)[rows], np.asarray(want)[rows]
        if not eq(got, want):
            bad = np.nonzero(np.any((got != want).reshape(len(got), -1), axis=1))[0]
            cases = np.nonzero(rows)[0][bad]
            raise AssertionError((tag, name, [(int(c), SE.FAMILIES[w["family"][c]], int(w["sub"][c])) for c in cases[:6]], len(cases)))
    check("agent_pos", st["agent_pos"], out["agent_pos"])
    check("agent_dir", st["agent_dir"], out["agent_dir"])
    check("carrying", st["carrying"], out["carrying"])
    check("step_count", st["step_count"], out["step_count"])
    alive = out["alive"].astype(bool)
    if b.ent_task:
        check("alive", st["ent_alive"], out["alive"].astype(np.int32))
        if not np.isnan(out["health"]).all():
            check("health", st["task_f"], out["health"])
        if (out["num_picked"] >= 0).all():
            check("num_picked", st["task_i"], out["num_picked"])
    else:
        assert alive.all()
    check("ents_pos", np.where(alive[..., None], st["boxes_pos"][:, :E], 0.0), np.where(alive[..., None], out["ents_pos"], 0.0))
    check("ents_dir", np.where(alive, st["boxes_dir"][:, :E], 0.0), np.where(alive, out["ents_dir"], 0.0))
    check("reward64", b.reward64.cpu().numpy(), out["reward"])
    check("done", b.done.cpu().numpy(), out["done"])
    check("ep_steps", b.ep_steps.cpu().numpy(), out["step_count"])
    if not np.isnan(out["goal_pos"]).any():
        check("goal_pos", b.goal_pos.cpu().numpy(), out["goal_pos"])


def assert_untouched(b, w, rows, tag):
    st, start = b.get_state(), w["start"]
    E = start["ents_pos"].shape[1]
    for name, got, want in (("agent_pos", st["agent_pos"], start["agent_pos"]), ("agent_dir", st["agent_dir"], start["agent_dir"]),
                            ("ents_pos", st["boxes_pos"][:, :E], start["ents_pos"]), ("ents_dir", st["boxes_dir"][:, :E], start["ents_dir"]),
                            ("carrying", st["carrying"], start["carrying"]), ("step_count", st["step_count"], start["step_count"])):
        assert np.ascontiguousarray(got[rows]).tobytes() == np.ascontiguousarray(want[rows]).tobytes(), (tag, "a skipped env changed", name)
    assert not b.done.cpu().numpy()[rows].any(), (tag, "a skipped env is done")


def check_world(b, w, n, tag):
    """the world is the reference's, in every env"""
    st = b.get_state()
    E = w["reset/ents_pos"].shape[0]
    assert b.n_boxes == E and np.array_equal(b.get_geometry(n - 1, max_segs=16384)[1], w["reset/wall_segs"]), tag
    for i in (0, n // 2, n - 1):
        assert np.array_equal(st["agent_pos"][i], w["reset/agent_pos"]) and st["agent_dir"][i] == float(w["reset/agent_dir"]), tag
        assert np.array_equal(st["boxes_pos"][i], w["reset/ents_pos"]) and np.array_equal(st["boxes_dir"][i], w["reset/ents_dir"]), tag


@pytest.mark.parametrize("task", list(SE.SPEC))
def test_steps_at_the_edges_are_the_references(task):
    import torch
    worlds, _ = SE.load(os.path.join(GOLD, "stepedge_%s.npz" % task))
    for seed, w in worlds.items():
        n = len(w["family"])
        b = make_handle(task, seed, n)
        acts = torch.from_numpy(w["action"].astype(np.int32))
        every = np.ones(n, bool)
        for mode in ("step", "repeat", "skip"):
            tag = (task, seed, mode)
            b.seed(np.full(n, seed, np.uint64))
            b.reset()
            if mode == "step":
                check_world(b, w, n, tag)
            put_start(b, w["start"])
            if mode == "step":
                b.step(acts)
                assert_outcome(b, w, every, tag)
            elif mode == "repeat":
                b.step_repeat(acts, 1)
                assert (b.taken.cpu().numpy() == 1).all(), tag
                assert_outcome(b, w, every, tag)
            else:
                skip = (np.arange(n) % 2 == 1)
                b.step(acts, skip_mask=torch.from_numpy(skip.astype(np.uint8)))
                assert_outcome(b, w, ~skip, tag)
                assert_untouched(b, w, skip, tag)
        b.close()


@pytest.mark.parametrize("task", [t for t in SE.SPEC if t != "SimToRealPush"])   # (its step draws the step length: no point recorded)
def test_intersect_at_the_decisive_points_is_the_references(task):
    """mwb_intersect where move_agent and the pickup probe ask MiniWorldEnv.intersect: nothing, a wall, or WHICH entity - of two in
    reach the one that stands earlier in the list"""
    worlds, _ = SE.load(os.path.join(GOLD, "stepedge_%s.npz" % task))
    asked = 0
    for seed, w in worlds.items():
        n = len(w["family"])
        b = make_handle(task, seed, n)
        b.reset()
        check_world(b, w, n, (task, seed))
        put_start(b, w["start"])
        wrong = []
        for c in np.nonzero(w["hit"] >= 0)[0]:
            got = b.intersect(int(c), float(w["hit_pos"][c, 0]), float(w["hit_pos"][c, 1]), float(w["hit_radius"][c]))
            asked += 1
            if got != w["hit"][c]:
                wrong.append((int(c), SE.FAMILIES[w["family"][c]], int(w["sub"][c]), got, int(w["hit"][c])))
        assert not wrong, (task, seed, wrong[:6], len(wrong))
        b.close()
    assert asked > 0
