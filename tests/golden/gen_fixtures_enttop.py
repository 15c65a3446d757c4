#!/usr/bin/env python3
"""render_top_view() streams of the tasks with a general entity list (meshes, image / text frames): the reference's map view
(miniworld.py:1087-1158) recorded under the inert `gym` / `pyglet` stand-ins, after a seeded prelude of policy steps.  Same method
as gen_fixtures_ents.py (whose helpers are imported, not copied): the UNMODIFIED reference runs, what is kept is data only.

Per case: the display list (rooms, then the STATIC entities in list order, compiled by reset()), this frame's glOrtho /
glLoadMatrixf / glClearColor, the non-static entities it drew and the agent's triangle with its colour and the normal that was
current when its glBegin was issued - tracked over the display list and this frame in call order; a vertex-array draw (a mesh)
issues no glNormal3f and so changes nothing.

Run:  python tests/golden/gen_fixtures_enttop.py [--out DIR] [task prefixes ...]     (build container only)
Outputs: enttop_<task>_dr<k>.json
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_fixtures_ents as GE  # noqa: E402  (installs the stand-ins, imports the reference)
from gen_fixtures_ents import choose, construct, describe_entities, parse_ent_stream, snapshot  # noqa: E402
from gen_fixtures import deps, parse_gl_log  # noqa: E402

OUT = HERE
# task -> (policy, prelude steps, stop rule); the stop rules give PickupObjs after a pick-up, RoomObjs while carrying, CollectHealth
# after a respawn (a collected medkit re-enters the list at its end), the others after a short wander
CASES = {
    "PickupObjs": ("collect", 400, "picked"), "RoomObjs": ("collect", 400, "carrying"), "CollectHealth": ("collect", 400, "respawned"),
    "ThreeRooms": ("wander", 25, None), "Sign": ("random", 8, None), "Sidewalk": ("wander", 25, None), "WallGap": ("wander", 25, None),
}


def capture_top(task, seed, dr):
    cls, kwargs = GE.ENT_TASKS[task]
    policy, n_max, stop = CASES[task]
    env = construct(cls, kwargs, dr)
    env.seed(seed)
    deps.GL_LOG.clear(); deps.GL_LOG_ENABLED[0] = True
    env.reset()
    deps.GL_LOG_ENABLED[0] = False
    reset_log = list(deps.GL_LOG); deps.GL_LOG.clear()
    arng = np.random.default_rng(9000 + seed)
    actions, stopped, extra = [], None, 0
    n0 = len(env.entities)
    for t in range(n_max):
        a = choose(env, policy, arng, t)
        first = env.entities[0]
        _, _, d, _ = env.step(a)
        actions.append(int(a))
        if d:
            return None   # the frame must be of the episode the prelude walked in: the caller takes the next seed
        if stopped is None:
            if stop == "picked" and getattr(env, "num_picked_up", 0) >= 1:
                stopped = t
            elif stop == "carrying" and env.agent.carrying is not None and t > 3:
                stopped = t
            elif stop == "respawned" and (env.entities[0] is not first or len(env.entities) != n0):
                stopped = t
        if stopped is not None:
            extra += 1
            if extra > 2:   # a few more steps: a carried object turned with the agent, a respawned medkit on the floor
                break
    if stop is not None and stopped is None:
        return None
    deps.GL_LOG_ENABLED[0] = True
    env.render_top_view()
    deps.GL_LOG_ENABLED[0] = False
    frame_log = list(deps.GL_LOG); deps.GL_LOG.clear()
    i0 = max(i for i, (n, _) in enumerate(reset_log) if n == "glNewList")
    i1 = max(i for i, (n, _) in enumerate(reset_log) if n == "glEndList")
    static_log = reset_log[i0:i1]
    room_polys, lights, _ = parse_gl_log(static_log)
    room_polys = [p for p in room_polys if not p["xform"] and p["tex_on"] and p["mode"] in ("GL_POLYGON", "GL_QUADS") and p["color"] == [1.0, 1.0, 1.0]]
    static_items = [it for it in parse_ent_stream(static_log) if it["xform"]]
    _, _, misc = parse_gl_log(frame_log)
    dyn_items = [it for it in parse_ent_stream(frame_log) if it["xform"]]
    # the agent's triangle: the last glBegin of the frame, parsed over the display list and the frame in call order so that its
    # vertices carry the normal current at that point
    agent = parse_ent_stream(static_log + frame_log)[-1]
    assert agent["type"] == "poly" and agent["mode"] == "GL_TRIANGLES" and not agent["xform"] and len(agent["verts"]) == 3
    assert all(c == [1.0, 0.0, 0.0] for c in agent["colors"]) and all(n == agent["norms"][0] for n in agent["norms"])
    st = snapshot(env)
    ents, desc = describe_entities(env)
    return {
        "task": task, "kwargs": kwargs, "seed": seed, "domain_rand": int(dr), "actions": actions,
        "lights": lights, "misc": {k: misc[k] for k in ("glOrtho", "glLoadMatrixf", "glClearColor")},
        "room_polys": room_polys, "static_items": static_items, "dynamic_items": dyn_items,
        "agent_tri": agent["verts"], "agent_color": agent["colors"][0], "agent_normal": agent["norms"][0],
        "extents": [float(env.min_x), float(env.max_x), float(env.min_z), float(env.max_z)],
        "room_tex": st["tex_names"].tolist(), "no_ceiling": st["no_ceiling"].tolist(),
        "agent_pos": st["agent_pos"].tolist(), "agent_dir": float(st["agent_dir"]),
        "carrying": -1 if env.agent.carrying is None else next(i for i, e in enumerate(ents) if e is env.agent.carrying),
        "ents": {k[5:]: (v.tolist()) for k, v in desc.items()},
    }


def main():
    global OUT
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT = args[i + 1]
        os.makedirs(OUT, exist_ok=True)
        args = args[:i] + args[i + 2:]
    only = args
    for task in CASES:
        if only and not any(task.startswith(o) for o in only):
            continue
        for dr in ((0,) if task in GE.NO_DR_KWARG else (0, 1)):
            g = next(g for g in (capture_top(task, seed, dr) for seed in range(1, 20)) if g is not None)
            with open(os.path.join(OUT, "enttop_%s_dr%d.json" % (task, dr)), "w") as fh:
                json.dump(g, fh, separators=(",", ":"))


if __name__ == "__main__":
    main()
