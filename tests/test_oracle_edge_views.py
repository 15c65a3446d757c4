"""CPU: the oracle at the directed edge poses of tests/edge_views.py against the brute-force rendition of the captured GL streams
RE-POSED: the stream keeps its polygons, its gluLookAt becomes (cam_pos, cam_pos + cam_dir, +Y) of the oracle's state (the relation
test_scene_inputs_equal_reference_gl_stream pins), and for family D the moved box's translate / rotate calls are rewritten.  The bars
are those of test_oracle_render.py and test_oracle_ents_render.py, nothing looser.  A sample at an even stride through every family
runs here (the GPU layer, test_gpu_edge_views.py, runs every pose against the oracle); the worst share per family is printed."""
import math

import numpy as np
import pytest

import edge_views as EV
from test_oracle_ents_render import load_stream as load_ent_stream, replay, soup_inputs
from test_oracle_render import load_stream, posed_env

BOX_STREAMS = [("Hallway", "Hallway", None, 0), ("FourRooms", "FourRooms", None, 0), ("FourRooms", "FourRooms", None, 1),
               ("MazeS3", "Maze", [3, 3, 3], 1), ("Maze", "Maze", None, 0), ("TMazeTwoBoxFeatures", "TMazeTwoBox", [1, 0, 0, 150], 1),
               ("YMaze", "YMaze", [0, 0, 0, 0], 0), ("YMaze", "YMaze", [0, 0, 0, 0], 1)]
PER_FAMILY = {"Maze": 2}   # poses per (stream, family), default 4: 8 streams, 28 (stream, family) pairs -> about 100 poses of 0.4 s (Maze: 4 s) each
ENT_STREAMS = [("PickupObjs", 2), ("CollectHealth", 2), ("ThreeRooms", 2), ("Sign", 3), ("Sidewalk", 2)]   # a pose costs 2 s (Sign) to 20 s (PickupObjs, ThreeRooms)


def reposed(g, env, entry):
    """the stream as the reference would have issued it from the entry's pose"""
    for b, (x, z, d) in enumerate(env.home_boxes):   # family D moves boxes
        env.set_box(b, x, z, d)
    EV.pose(env, entry)
    s = env.state()
    g2 = dict(g)
    g2["misc"] = dict(g["misc"])
    cp, cd = np.array(s.cam_pos), np.array(s.cam_dir)
    g2["misc"]["gluLookAt"] = list(cp) + list(cp + cd) + [0, 1.0, 0]
    box = entry[4]
    if box is not None:   # the boxes are the stream's last polygons, in entity order (test_scene_inputs_equal_reference_gl_stream)
        b, x, z, d = box
        polys = list(g["polys"])
        k = len(polys) - s.n_boxes + b
        p = dict(polys[k])
        assert p["xform"][0][0] == "translate" and p["xform"][1][0] == "rotate"
        p["xform"] = [["translate", x, 0.0, z], ["rotate", d * (180 / math.pi), 0.0, 1.0, 0.0]]
        polys[k] = p
        g2["polys"] = polys
    return g2


def sample(env, cat, per_family):
    """an even stride through each family's poses that the rendition can arbitrate (rule 6 of edge_views.py: YMaze only)"""
    junctions = EV.overlap_junctions(env.geometry())
    assert bool(junctions) == (env.task == "YMaze")
    s = env.state()
    hfov = math.atan(math.tan(math.radians(s.cam_fov_y) / 2) * env.W / env.H)

    def arbitrable(entry):
        EV.pose(env, entry)
        c = env.state().cam_pos
        return not EV.sees_overlap_junction(junctions, (c[0], c[2]), entry[3], hfov)
    out = []
    for fam in sorted({EV.family(e[0]) for e in cat}):
        own = [e for e in cat if EV.family(e[0]) == fam and (not junctions or arbitrable(e))]
        assert own, (fam, "no pose left")
        out += EV.strided(own, per_family)
    return out


@pytest.mark.parametrize("name,task,args,dr", BOX_STREAMS)
def test_box_tasks_edge_poses_equal_bruteforce_rendition(oracle_mod, name, task, args, dr):
    import soup_renderer as SR
    O = oracle_mod
    g = load_stream(name, dr)
    tex = O.load_textures()
    textures = {O.TEX_FILES[i]: tex[i][2] for i in tex}
    env = posed_env(O, g, task, args, dr)
    s = env.state()
    env.home_boxes = [(s.boxes_pos[b][0], s.boxes_pos[b][2], s.boxes_dir[b]) for b in range(s.n_boxes)]
    cat = EV.catalogue(env)
    fams = {EV.family(e[0]) for e in cat}
    assert {"A", "C"} <= fams and ("B" in fams) == (env.state().n_rooms > 1) and ("D" in fams) == (dr == 0)
    worst = {}
    for entry in sample(env, cat, PER_FAMILY.get(name, 4)):
        g2 = reposed(g, env, entry)
        d = np.abs(env.render_obs().astype(int) - SR.render_stream(g2, textures).astype(int))
        share = float((d.max(axis=2) > 1).mean())
        worst[EV.family(entry[0])] = max(worst.get(EV.family(entry[0]), 0.0), share)
        print("%s dr%d %-24s off by more than 1: %.5f  mean %.4f" % (name, dr, entry[0], share, d.mean()))
        assert share <= 2e-3 and d.mean() < 0.02, (name, dr, entry, share, float(d.mean()), int(d.max()))
    print("WORST %s dr%d %s" % (name, dr, " ".join("%s=%.5f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name,count", ENT_STREAMS)
def test_entity_tasks_edge_poses_equal_bruteforce_rendition(oracle_mod, name, count):
    import soup_renderer as SR
    O = oracle_mod
    g = load_ent_stream(name, 0)
    env = replay(O, g, name, 0)
    env.home_boxes = []   # only the agent moves
    textures, arrays = soup_inputs(O)
    cat = [e for e in EV.catalogue(env, tex_sizes=O.load_textures(len(O.TEX_FILES))) if EV.family(e[0]) == "E"]
    assert len(cat) >= 8
    frames = [e for e in cat if ":edge:" in e[0]]
    assert bool(frames) == (name in ("ThreeRooms", "Sign"))
    n_fr = min(len(frames), count // 2)
    picks = EV.strided([e for e in cat if e not in frames], count - n_fr) + EV.strided(frames, n_fr)
    worst = 1.0
    for entry in picks:
        g2 = reposed(g, env, entry)
        diff = np.abs(env.render_obs().astype(int) - SR.render_ent_stream(g2, textures, arrays).astype(int)).max(axis=2)
        frac = float((diff <= 1).mean())
        worst = min(worst, frac)
        print("%s %-16s within 1: %.5f  max %d  over 24: %.5f" % (name, entry[0], frac, int(diff.max()), float((diff > 24).mean())))
        assert frac >= 0.995 and np.median(diff) == 0, (name, entry, frac, int(diff.max()))
        assert (diff > 24).mean() <= 0.002, (name, entry, float((diff > 24).mean()))
    print("WORST %s E=%.5f (share within 1)" % (name, worst))


def _fresh(O, task, args, seed=3):
    from test_oracle_ents import sign_params
    env = O.OracleEnv(task, seed=seed, domain_rand=0, task_args=args, params=sign_params() if task == "Sign" else None)
    env.reset(render=False)
    tex = O.load_textures(len(O.TEX_FILES)) if O.TASKS[task] >= 10 else None
    return env, EV.catalogue(env, tex_sizes=tex)


@pytest.mark.parametrize("task,args", [("FourRooms", None), ("YMaze", [0, 0, 0, 0]), ("Maze", [3, 3, 3])])
def test_family_b_looks_at_both_sides_of_every_plane(oracle_mod, task, args):
    """a catalogue that silently collapsed (both headings on one side, every eye in one spot) must fail: the two headings of a pair
    across a portal plane show different frames, and so do the three eye positions of an opening"""
    env, cat = _fresh(oracle_mod, task, args)
    shots = {}
    for entry in cat:
        if EV.family(entry[0]) == "B":
            EV.pose(env, entry)
            shots[entry[0]] = env.render_obs()
    pairs = [(t, t.replace(":in:", ":out:")[:-1] + str(int(t[-1]) + 1)) for t in shots if ":in:" in t]
    pairs = [(a, b) for a, b in pairs if b in shots]   # rule 4 may have taken one of the two
    assert len(pairs) >= len(shots) // 3 >= 8
    for a, b in pairs:
        assert not np.array_equal(shots[a], shots[b]), (a, b)
    for t in shots:
        if ":q0:" in t and t.replace(":q0:", ":q1:") in shots and t.replace(":q0:", ":q2:") in shots:
            assert not np.array_equal(shots[t], shots[t.replace(":q0:", ":q1:")]) and not np.array_equal(shots[t], shots[t.replace(":q0:", ":q2:")]), t


@pytest.mark.parametrize("task,args", [("Hallway", None), ("FourRooms", None), ("TMazeTwoBox", [0, 0, 0, 100])])
def test_family_d_sweeps_cross_the_frame_borders(oracle_mod, task, args):
    """box pixels: where the frame differs from the same view with the box 3 m behind the agent.  Every sweep through a side border
    has frames with box pixels in the frame's border columns and frames with none there; where the box's last corner leaves (L:lo,
    R:hi) it has frames without any box pixel, where its first corner arrives (L:hi, R:lo) the box shows throughout.  Along the
    approach the box always shows (its top face, if nothing else), and its near face's bottom edge enters and leaves the bottom row."""
    env, cat = _fresh(oracle_mod, task, args)
    shown = {}
    for entry in cat:
        if EV.family(entry[0]) != "D":
            continue
        EV.pose(env, entry)
        with_box = env.render_obs()
        b, _, _, bdir = entry[4]
        behind = np.array(entry[1:3]) - 3.0 * EV.heading_vec(entry[3])
        env.set_box(b, float(behind[0]), float(behind[1]), bdir)
        px = (with_box != env.render_obs()).any(axis=2)
        shown.setdefault(EV.group(entry[0]), []).append((bool(px.any()), bool(px[-1].any()), bool(px[:, 0].any() or px[:, -1].any())))
    n_boxes = env.state().n_boxes
    assert len(shown) == n_boxes * (4 + 2 + 4) and all(len(v) == (3 if ":square:" in g else 17) for g, v in shown.items())
    for g, v in shown.items():
        EV.check_box_sweep(g, v)


@pytest.mark.parametrize("task,args", [("PickupObjs", [12, 5, 0, 0]), ("CollectHealth", [16, 0, 0, 0]), ("ThreeRooms", None), ("Sign", [10, 0, 0, 0]),
                                       ("Sidewalk", None)])
def test_family_e_shows_every_entity(oracle_mod, task, args):
    """each entity shows in at least one of its frames (against the same view with the entity a kilometre behind the agent), and
    the edge-on poses do see their frame's black side"""
    env, cat = _fresh(oracle_mod, task, args)
    s = env.state()
    shown = {}
    for entry in cat:
        if EV.family(entry[0]) != "E":
            continue
        EV.pose(env, entry)
        img = env.render_obs()
        if ":edge:" in entry[0]:
            shown.setdefault(EV.group(entry[0]), []).append(bool((img.max(axis=2) == 0).any()))
            continue
        b = int(entry[0].split(":")[1][1:])
        behind = np.array(entry[1:3]) - 1000.0 * EV.heading_vec(entry[3])
        env.set_box(b, float(behind[0]), float(behind[1]), s.boxes_dir[b])
        shown.setdefault(EV.group(entry[0]), []).append(not np.array_equal(img, env.render_obs()))
        env.set_box(b, s.boxes_pos[b][0], s.boxes_pos[b][2], s.boxes_dir[b])
    assert len(shown) >= 4
    for g, v in shown.items():
        assert any(v) and (":edge" in g or not all(v)), (g, v)
