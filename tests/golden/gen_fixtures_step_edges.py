#!/usr/bin/env python3
"""Golden vectors for single steps at the decision edges of MiniWorldEnv.step (tests/step_edges.py builds the start states).
Same method as gen_fixtures_ents.py: the UNMODIFIED reference runs under the inert `gym` / `pyglet` stand-ins of _inert_deps.py;
what is kept is data only - start states and what the reference's own step() made of them.

Run:  python tests/golden/gen_fixtures_step_edges.py [--out DIR] [task prefixes ...]     (build container only)
Outputs: stepedge_<task>.npz

Per world seed `s<seed>/`: the world after reset() (wall_segs, the entity list with radii, heights and their scalar types), and
for every case its family / group / sub-group ids, the start state (agent pose, every entity's pos and dir, carrying,
step_count, the action), the outcome (the same, plus reward as float64, done, which entities are still in the list, the
task's info values) and `hit`: what MiniWorldEnv.intersect itself returns at the decisive point of a move or a pickup (0
nothing, 1 a wall, 2 + k the k-th entity of the list), with the point and radius it was asked about.

Groups whose eight recorded outcomes do not straddle their decision (sub 0) or do (sub 1: the groups around the threshold a
float64 sum would give, where the reference adds in float32) are dropped; the restated predicate may be an ulp off the
reference's.  At most a tenth of a family's groups may go that way and at least one must stay: asserted here, and again on the
committed files by tests/test_oracle_step_edges.py.  `meta/numpy_major` and `ents_radius_f32` record which scalar semantics the
files carry."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_fixtures as G  # noqa: E402,F401  (installs the stand-ins, imports the reference)

import step_edges as SE  # noqa: E402
from gym_miniworld.entity import Entity  # noqa: E402
from gym_miniworld.envs import (CollectHealth, FourRooms, Hallway, Maze, PickupObjs, PutNext, RoomObjs, Sign,  # noqa: E402
                                SimToRealPush, TMazeTwoBoxDynamic, YMaze)

OUT = HERE
# task -> (reference class, constructor kwargs, world seeds)
TASKS = {
    "Maze": (Maze, {}, (0, 1)),
    "MazeR9C9": (Maze, {"num_rows": 9, "num_cols": 9}, (0, 1)),
    "MazeR16C16": (Maze, {"num_rows": 16, "num_cols": 16}, (0, 1)),
    "YMaze": (YMaze, {}, (0, 1)),
    "FourRooms": (FourRooms, {}, (0, 1)),
    "Hallway": (Hallway, {}, (0, 1, 2)),
    "TMazeTwoBoxDynamic": (TMazeTwoBoxDynamic, {}, (0, 1)),
    "PutNext": (PutNext, {}, (0, 1, 2)),
    "PickupObjs": (PickupObjs, {}, (0, 1, 2, 3)),
    "RoomObjs": (RoomObjs, {}, (0, 1)),
    "CollectHealth": (CollectHealth, {}, (0, 1)),
    "Sign": (Sign, {}, (0, 1)),
    "SimToRealPush": (SimToRealPush, {}, (0, 1, 2)),   # always randomised: every case starts from the generator state reset() left
}
THETAS = (0.5, 1.15, 2.0, 2.7, -0.6, -1.3, -2.2, -2.75)   # approach directions of the entity families: no sine or cosine near 0 or 1


def world_of(env):
    ents = [e for e in env.entities if e is not env.agent]
    assert env.entities[-1] is env.agent
    segs = np.asarray(env.wall_segs)
    segs4 = np.concatenate([segs[:, 0, [0, 2]], segs[:, 1, [0, 2]]], axis=1)
    p = env.params
    w = SE.World(segs4, [e.radius for e in ents], [e.height for e in ents], [bool(e.is_static) for e in ents], env.agent.radius,
                 env.max_forward_step, p.sample(None, "forward_step"), p.sample(None, "forward_drift"), p.sample(None, "turn_step"), env.agent.cam_height)
    base = SE.make_state(env.agent.pos, env.agent.dir, [np.asarray(e.pos, float) for e in ents], [float(e.dir) for e in ents])
    return ents, w, base


def heading_cycle():
    i = 0
    while True:
        yield SE.HEADING_OFFSETS[i % len(SE.HEADING_OFFSETS)]
        i += 1


def plan(task, env, ents, w, base):
    """the groups of one world, family by family"""
    out = []
    offs = heading_cycle()
    S = len(w.segs)
    add = lambda g: out.append(g) if g is not None else None   # noqa: E731
    f32 = [isinstance(r, np.float32) for r in w.radius]
    if task.startswith("Maze"):   # one wall_interior group per segment group index of the world
        for gi in range((S + 7) // 8):
            for margins in ((SE.MARGIN,), (SE.MARGIN_TIGHT,)):
                g = None
                for j in range(gi * 8, min(S, gi * 8 + 8)):
                    g = SE.wall_interior_group(w, base, j, 2 + gi % 2, next(offs), margins)
                    if g is not None:
                        break
                if g is not None:
                    break
            add(g)
    if task == "YMaze":   # slanted segments
        for j in range(S):
            a, b = w.segs[j, :2], w.segs[j, 2:]
            if min(abs(a[0] - b[0]), abs(a[1] - b[1])) > 0.05:
                for act in (2, 3):
                    add(SE.wall_interior_group(w, base, j, act, next(offs)))
    if task == "FourRooms":
        for point in SE.end_points(w):
            for quadrant in range(4):
                add(SE.wall_endpoint_group(w, base, point, 2 + quadrant % 2, next(offs) * 0.3, quadrant))
        for j in range(0, S, 3):
            add(SE.wall_interior_group(w, base, j, 2 + j % 2, next(offs)))
    movable = [k for k in range(w.E) if float(w.radius[k]) > 0]
    if task in ("Hallway", "TMazeTwoBoxDynamic", "PutNext", "PickupObjs", "CollectHealth", "RoomObjs"):
        for k in movable[:8]:
            n = 0
            for i, th in enumerate(THETAS):
                g = SE.agent_entity_group(w, base, k, 2 + (i + k) % 2, th)
                if g is None:
                    continue
                add(g)
                if f32[k]:   # tag_gap: the same approach around the float64 sum's threshold
                    add(SE.agent_entity_group(w, base, k, 2 + (i + k) % 2, th, sum64=True))
                n += 1
                if n == 3:
                    break
    if task == "PutNext":
        for pi, (k, m) in enumerate(((0, 1), (1, 3), (2, 5), (0, 4), (3, 4))):
            for th in THETAS[pi:] + THETAS[:pi]:
                g = SE.agent_entity_two_group(w, base, k, m, 2, th)
                if g is not None:
                    add(g)
                    break
    goals = {"Hallway": [0], "TMazeTwoBoxDynamic": [0, 1], "Sign": [ents.index(o) for pair in getattr(env, "_objects", []) for o in pair]}.get(task, [])
    for k in goals:
        n = 0
        for i, th in enumerate(THETAS):
            g = SE.near_done_group(w, base, k, 2 + (i + k) % 2 if task != "Sign" else 2, th, others=goals)
            if g is None:
                continue
            add(g)
            if f32[k]:
                add(SE.near_done_group(w, base, k, 2, th, sum64=True, others=goals))
            n += 1
            if n == 3:
                break
    if task in ("PutNext", "PickupObjs"):
        for k in movable:
            n = 0
            for th in THETAS:
                g = SE.pickup_reach_group(w, base, k, th)
                if g is None:
                    continue
                add(g)
                if f32[k]:
                    add(SE.pickup_reach_group(w, base, k, th, sum64=True))
                n += 1
                if n == 2:
                    break
        for pi, (k, m) in enumerate(zip(movable[:-1], movable[1:])):   # two in reach: the lower index is the one picked up
            for th in THETAS[pi:] + THETAS[:pi]:
                g = SE.pickup_two_group(w, base, k, m, th)
                if g is not None:
                    add(g)
                    break
        for j in range(S):
            for k in movable[:3]:
                add(SE.pickup_wall_group(w, base, j, k, next(offs)))
    if task in ("PutNext", "RoomObjs"):
        for k in movable[:3]:
            for j in range(S):
                for act in (2, 0, 1):
                    add(SE.carry_wall_group(w, base, k, j, act, next(offs)))
            for m in [m for m in movable if m != k][:2]:
                for i, act in enumerate((2, 0, 1)):
                    for th in THETAS[i:]:
                        g = SE.carry_entity_group(w, base, k, m, act, th)
                        if g is None:
                            continue
                        add(g)
                        if f32[k] or f32[m]:
                            add(SE.carry_entity_group(w, base, k, m, act, th, sum64=True))
                        break
    if task == "PutNext":
        red, yel = ents.index(env.red_box), ents.index(env.yellow_box)
        for th in THETAS[:4]:
            add(SE.entity_near_group("putnext_rule", w, base, red, yel, th, 5, red))
        y = float(SE.carry_pos(w, np.zeros(3), 0.0, red)[1])
        assert y > 0.3
        for th in THETAS[4:]:
            add(SE.entity_near_group("near_3d", w, base, red, yel, th, 0, -1, y_i=y))
    if task == "SimToRealPush":
        for b in (0, 1):
            for th in THETAS:
                add(SE.push_shove_group(w, base, b, th))
        for i, th in enumerate(THETAS[:6]):
            add(SE.push_goal_group(w, base, float(env.goal_dist), th, i % 2))
    return out


def hit_code(env, ents, r):
    if r is None or r is False:
        return 0
    if r is True:
        return 1
    assert isinstance(r, Entity)
    return 2 + (len(ents) if r is env.agent else ents.index(r))


def run_world(task, cls, kwargs, seed):
    env = cls(**kwargs)
    env.seed(seed)
    env.reset()
    ents, w, base = world_of(env)
    E = len(ents)
    groups = plan(task, env, ents, w, base)
    rng0 = env.rand.np_random.get_state()
    list0 = list(env.entities)
    extra0 = {k: getattr(env, k) for k in ("health", "num_picked_up") if hasattr(env, k)}
    n = len(groups) * SE.GROUP
    rec = {"family": np.zeros(n, np.int32), "group": np.zeros(n, np.int32), "sub": np.zeros(n, np.int32), "action": np.zeros(n, np.int32),
           "decider": np.zeros(n, np.int32), "clamp": np.zeros(n, np.int32), "margin": np.zeros(n),
           "hit": np.full(n, -1, np.int32), "hit_pos": np.zeros((n, 2)), "hit_radius": np.zeros(n), "hit_self": np.full(n, -1, np.int32)}
    start = {"agent_pos": np.zeros((n, 3)), "agent_dir": np.zeros(n), "ents_pos": np.zeros((n, E, 3)), "ents_dir": np.zeros((n, E)),
             "carrying": np.zeros(n, np.int32), "step_count": np.zeros(n, np.int32)}
    out = {k: v.copy() for k, v in start.items()}
    out.update({"reward": np.zeros(n), "done": np.zeros(n, np.uint8), "alive": np.zeros((n, E), np.uint8), "health": np.full(n, np.nan),
                "goal_pos": np.full((n, 3), np.nan), "num_picked": np.full(n, -1, np.int32)})
    A = env.actions
    c = 0
    for gi, g in enumerate(groups):
        for st in g["states"]:
            # the world as reset() left it, then this case's start state
            env.entities[:] = list0
            env.rand.np_random.set_state(rng0)
            for k, v in extra0.items():
                setattr(env, k, v)
            env.agent.pos, env.agent.dir = st["agent_pos"].copy(), st["agent_dir"]
            for k, e in enumerate(ents):
                e.pos, e.dir = st["ents_pos"][k].copy(), float(st["ents_dir"][k])
            env.agent.carrying = ents[st["carrying"]] if st["carrying"] >= 0 else None
            env.step_count = st["step_count"]
            for k in ("family", "sub", "action", "decider", "clamp", "margin"):
                rec[k][c] = SE.FAMILY_ID[g[k]] if k == "family" else g[k]
            rec["group"][c] = gi
            for k in start:
                start[k][c] = st[k]
            act = g["action"]
            a = env.agent
            if env.domain_rand:   # the step draws its own step length: no point to ask about beforehand
                pt = None
            elif act in (int(A.move_forward), int(A.move_back)):   # what intersect() says where move_agent asks it
                fd = w.fwd_step if act == int(A.move_forward) else -w.fwd_step
                pt, rad = a.pos + a.dir_vec * fd + a.right_vec * w.fwd_drift, a.radius
            elif act == int(A.pickup):
                pt, rad = a.pos + a.dir_vec * 1.5 * a.radius, 1.2 * a.radius
            else:
                pt = None
            if pt is not None:
                rec["hit"][c] = hit_code(env, ents, env.intersect(a, pt, rad))
                rec["hit_pos"][c], rec["hit_radius"][c], rec["hit_self"][c] = [pt[0], pt[2]], rad, E
            _, r, d, info = env.step(act)
            out["agent_pos"][c], out["agent_dir"][c] = a.pos, a.dir
            for k, e in enumerate(ents):
                out["ents_pos"][c, k], out["ents_dir"][c, k] = e.pos, e.dir
                out["alive"][c, k] = any(e is x for x in env.entities)
            out["carrying"][c] = -1 if a.carrying is None else ents.index(a.carrying)
            out["step_count"][c], out["reward"][c], out["done"][c] = env.step_count, r, d
            if "health" in info:
                out["health"][c] = info["health"]
            if "goal_pos" in info:
                out["goal_pos"][c] = info["goal_pos"]
            if hasattr(env, "num_picked_up"):
                out["num_picked"][c] = env.num_picked_up
            c += 1
    # judged by the reference: sub 0 straddles, sub 1 does not
    flat = lambda d: {k: v for k, v in d.items()}   # noqa: E731
    dec = SE.decisions(flat(start), {**flat(out), "hit": rec["hit"]}) if n else np.zeros((0, 9))
    keep_g = np.zeros(len(groups), bool)
    built = np.zeros(len(SE.FAMILIES) * 2, np.int32)
    dropped = np.zeros(len(SE.FAMILIES) * 2, np.int32)
    if n:
        strad = SE.straddles(dec)
        for gi, g in enumerate(groups):
            slot = SE.FAMILY_ID[g["family"]] * 2 + g["sub"]
            built[slot] += 1
            keep_g[gi] = strad[gi] == (g["sub"] == 0)
            dropped[slot] += not keep_g[gi]
    keep = np.repeat(keep_g, SE.GROUP)
    blob = {"built": built, "dropped": dropped}
    blob.update({k: v[keep] for k, v in rec.items()})
    blob.update({"start/" + k: v[keep] for k, v in start.items()})
    blob.update({"out/" + k: v[keep] for k, v in out.items()})
    blob.update({"reset/wall_segs": w.segs, "reset/agent_pos": base["agent_pos"], "reset/agent_dir": np.array(base["agent_dir"]),
                 "reset/ents_pos": base["ents_pos"], "reset/ents_dir": base["ents_dir"],
                 "ents_radius": np.array([float(r) for r in w.radius]), "ents_radius_f32": np.array([isinstance(r, np.float32) for r in w.radius]),
                 "ents_height": np.array([float(h) for h in w.height]), "ents_height_f32": np.array([isinstance(h, np.float32) for h in w.height]),
                 "ents_static": np.array(w.static), "agent_radius": np.array(float(w.arad)), "max_forward_step": np.array(float(w.max_fwd)),
                 "max_episode_steps": np.array(float(env.max_episode_steps))})
    return blob


def check_caps(task, blobs):
    """at most a tenth of a family's groups dropped, no family without survivors"""
    built = sum(b["built"] for b in blobs)
    dropped = sum(b["dropped"] for b in blobs)
    for slot in np.nonzero(built)[0]:
        name = SE.FAMILIES[slot // 2] + (" (float64-sum groups)" if slot % 2 else "")
        assert dropped[slot] * 10 <= built[slot], (task, name, int(dropped[slot]), int(built[slot]))
        assert dropped[slot] < built[slot], (task, name)
    return built, dropped


def main():
    global OUT
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT = args[i + 1]
        os.makedirs(OUT, exist_ok=True)
        args = args[:i] + args[i + 2:]
    for task, (cls, kwargs, seeds) in TASKS.items():
        if args and not any(task.startswith(o) for o in args):
            continue
        blobs = [run_world(task, cls, kwargs, s) for s in seeds]
        built, dropped = check_caps(task, blobs)
        blob = {"meta/numpy_major": np.array(int(np.__version__.split(".")[0])), "meta/seeds": np.array(seeds, np.int64),
                "meta/families": np.array(SE.FAMILIES)}
        for s, b in zip(seeds, blobs):
            blob.update({"s%d/%s" % (s, k): v for k, v in b.items()})
        np.savez_compressed(os.path.join(OUT, "stepedge_%s.npz" % task), **blob)
        print(task, {SE.FAMILIES[i // 2] + ("/f64" if i % 2 else ""): "%d-%d" % (built[i], dropped[i]) for i in np.nonzero(built)[0]})


if __name__ == "__main__":
    main()
