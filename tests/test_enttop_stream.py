"""render_top_view for the tasks with mesh entities and frames (miniworld.py:1087-1158), CPU legs.

The reference's own map-view streams (tests/golden/enttop_*.json, generator gen_fixtures_enttop.py): the display list (rooms, the
static entities), this frame's glOrtho / modelview / clear colour, the non-static entities and the agent's triangle with the normal
that was current when it was drawn.  Pinned here: (a) the files are what the generator makes of the unmodified reference; (b) their
inputs equal the oracle's replayed state, and the agent's normal follows the frozen rule of DESIGN.md 5 computed from the entity
list alone; (c) the test-side orthographic rendition (tests/soup_top.py) equals the box tasks' already pinned one on their gltop_*
streams; (d) no fixture frame is vacuous - entities and meshes are in view, the frames' strips where the task has frames."""
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_oracle_ents_render import replay, soup_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
STREAMS = [("PickupObjs", 0), ("PickupObjs", 1), ("RoomObjs", 0), ("RoomObjs", 1), ("CollectHealth", 0), ("CollectHealth", 1),
           ("ThreeRooms", 0), ("ThreeRooms", 1), ("Sign", 0), ("Sidewalk", 0), ("Sidewalk", 1), ("WallGap", 0), ("WallGap", 1)]


def load(name, dr):
    with open(os.path.join(GOLD, "enttop_%s_dr%d.json" % (name, dr))) as fh:
        return json.load(fh)


def frozen_agent_normal(kinds, last_room_wall_normal):
    """the last glNormal3f before the agent's glBegin in call order, vertex arrays changing nothing.  Every Box and
    every image / text frame ends on its (0, -1, 0) face; meshes issue none; else the rooms' last wall quad decides."""
    if any(k in (0, 2, 3) for k in kinds):
        return [0.0, -1.0, 0.0]
    return [float(v) for v in last_room_wall_normal]


def test_fixture_set():
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(GOLD, "enttop_*.json")))
    assert names == sorted("enttop_%s_dr%d.json" % s for s in STREAMS)
    normals = set()
    for name, dr in STREAMS:
        g = load(name, dr)
        assert os.path.getsize(os.path.join(GOLD, "enttop_%s_dr%d.json" % (name, dr))) < 64 * 1024
        normals.add(tuple(g["agent_normal"]))
        if name == "PickupObjs":
            assert len(g["ents"]["kind"]) < 5   # after a pick-up: the object left the list
        if name == "RoomObjs":
            assert g["carrying"] >= 0
    assert len(normals) == 2   # both branches of the agent-normal rule


@pytest.mark.skipif(not os.path.isdir("/root/reference/gym_miniworld"), reason="needs the reference checkout")
def test_enttop_fixtures_round_trip(tmp_path):
    out = str(tmp_path)
    subprocess.check_call([sys.executable, os.path.join(GOLD, "gen_fixtures_enttop.py"), "--out", out], stdout=subprocess.DEVNULL)
    names = sorted(os.listdir(out))
    assert names == sorted(f for f in os.listdir(GOLD) if f.startswith("enttop_"))
    for f in names:
        with open(os.path.join(out, f)) as fa, open(os.path.join(GOLD, f)) as fb:
            assert json.load(fa) == json.load(fb), f


@pytest.mark.parametrize("name,dr", STREAMS)
def test_inputs_equal_the_oracle_state(oracle_mod, name, dr):
    O = oracle_mod
    g = load(name, dr)
    env = replay(O, g, name, dr)
    s, geo = env.state(), env.geometry()
    assert list(s.agent_pos) == g["agent_pos"] and s.agent_dir == g["agent_dir"] and s.carrying == g["carrying"]
    # the entity list: kinds and poses in list order (slots of the episode's first list, -2... = the agent)
    slots = [s.order[k] for k in range(s.n_order) if s.order[k] >= 0]
    assert [int(s.ents_kind[b]) for b in slots] == g["ents"]["kind"]
    assert [bool(s.ents_static[b]) for b in slots] == g["ents"]["static"]
    assert np.array_equal(np.array([list(s.boxes_pos[b]) for b in slots]).reshape(-1, 3), np.array(g["ents"]["pos"]).reshape(-1, 3))
    assert [s.boxes_dir[b] for b in slots] == g["ents"]["dir"]
    # extents and the glOrtho frame (80 x 60: the reference's obs_fb)
    o = geo["outline"]
    ext = [np.nanmin(o[:, :, 0]), np.nanmax(o[:, :, 0]), np.nanmin(o[:, :, 1]), np.nanmax(o[:, :, 1])]
    assert ext == g["extents"]
    l, r, b, t, n, f = g["misc"]["glOrtho"]
    w, h = ext[1] - ext[0] + 2, ext[3] - ext[2] + 2
    assert abs((r - l) / (t - b) - 80 / 60) < 1e-12 and (abs((r - l) - w) < 1e-12 or abs((t - b) - h) < 1e-12)
    assert abs((l + r) / 2 - (ext[0] + ext[1]) / 2) < 1e-12 and abs(-(b + t) / 2 - (ext[2] + ext[3]) / 2) < 1e-12 and (n, f) == (-100.0, 100.0)
    # the agent's triangle (entity.py:494-514; glVertex order p0, p2, p1)
    ax, az, ad, rad = s.agent_pos[0], s.agent_pos[2], s.agent_dir, s.agent_radius
    dv, rv = np.array([math.cos(ad), 0, -math.sin(ad)]) * rad, np.array([math.sin(ad), 0, math.cos(ad)]) * rad
    p = np.array([ax, 1.6, az])
    want = [p + dv, p + 0.75 * (-rv - dv), p + 0.75 * (rv - dv)]
    assert np.abs(np.array(g["agent_tri"]) - np.array(want)).max() < 1e-6 and g["agent_color"] == [1.0, 0.0, 0.0]
    # the frozen normal rule from the entity list alone; the rooms' last wall quad from the oracle's geometry
    last_wall = geo["wall_norms"][geo["quad_offsets"][-1] * 4 - 1]
    assert frozen_agent_normal(g["ents"]["kind"], last_wall) == [abs(v) if v == 0 else v for v in g["agent_normal"]]


@pytest.mark.parametrize("name,dr", [("YMaze", 0), ("FourRooms", 1), ("PutNext", 1)])
def test_soup_top_equals_the_pinned_box_rendition(oracle_mod, name, dr):
    import soup_renderer as SR
    import soup_top as ST
    O = oracle_mod
    with open(os.path.join(GOLD, "gltop_%s_dr%d.json" % (name, dr))) as fh:
        g = json.load(fh)
    tex = O.load_textures()
    textures = {O.TEX_FILES[i]: tex[i][2] for i in tex}
    for W, H in ((80, 60), (200, 150)):
        a, mask, _ = ST.render_top(ST.gltop_polys(g), g["misc"], textures, W, H)
        with np.errstate(all="ignore"):
            b = SR.render_stream(g, textures, W, H, ortho=True)
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 1, (name, W, H)
        assert mask.any()


@pytest.mark.parametrize("name,dr", STREAMS)
def test_fixture_frames_are_not_vacuous(oracle_mod, name, dr):
    import soup_top as ST
    g = load(name, dr)
    textures, arrays = soup_inputs(oracle_mod)
    img, mask, cover = ST.render_top(ST.enttop_polys(g, arrays), g["misc"], textures, 200, 150)
    assert cover["agent"].any() and cover["room"].mean() > 0.02
    assert (mask & ~cover["agent"]).sum() >= 20   # entities in view, beside the agent
    if name == "WallGap":
        # its one mesh, a 30 m building at (30, 0, 30), stands outside the map's extents (wallgap.py:43-51): the box and the agent
        assert cover["box"].any() and not cover["mesh"].any()
    else:
        assert cover["mesh"].sum() >= 10
    if name in ("ThreeRooms", "Sign"):
        assert cover["frame"].sum() >= 5
        assert (img[cover["frame"] & ~cover["mesh"] & ~cover["box"] & ~cover["agent"]].astype(int).sum(axis=1) < 3 * 255).all()
