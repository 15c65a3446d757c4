"""Directed camera poses at the geometric edges of the render spec (a helper, not a test).

Random headings at spawn positions cover the interior of the pose space.  The renderers' special cases sit on sets such poses hit
with probability zero: rays parallel to a wall, the eye on a plane two rooms share, the eye a float32 ulp from a wall, silhouettes
grazing the frame's border, faces seen exactly edge-on, portals in line.  catalogue(env) builds those poses from the world's own
geometry (env.geometry(), env.state()); its only constants are offsets, never world coordinates.

THE RULE for an admissible eye (cam_pos of the oracle's state after set_agent), asserted for every pose emitted:
  1. it is strictly inside a room, or on an edge shared by two rooms;
  2. wherever it is on a room's edge it is inside a portal's open interval, at least 1/8 of the opening's width from each jamb
     (so never on an unshared wall plane, a vertex or a jamb);
  3. it is never nearer than 0.05 m to a wall it faces within +-45 degrees (the reference's near plane is 0.04 m, and no renderer
     of this project models it);
  4. it is never inside an entity;
  5. rules 1 and 2 also hold for the eye and the world rounded to float32, which is what every renderer of this project works with:
     an eye 1e-7 m from a wall at x = -7 IS on that wall's plane once rounded (the wall then fills half the frame with one texel
     whose level of detail is undefined: the oracle takes the coarsest level, the z-buffer rendition level 0; measured 50 % of
     the pixels off by 3).  Family C therefore doubles its smallest distance from 1e-7 m until the rounded eye is off the plane.
  6. (only where the brute-force rendition arbitrates, test_oracle_edge_views.py) no corner of YMaze's overlap centimetre falls into
     the frame: see overlap_junctions().  The GPU layer runs these poses too, against the oracle.
"On" a plane means within EDGE_TOL = 1e-9 m in float64: points of the rotated edges of YMaze have no exact representation.
Poses are excluded by this rule only, never by a result.  Outside it (eye on a wall plane outside an opening, on a room corner,
on a jamb's end, outside every room) the z-buffer and the portal traversal legitimately disagree; see DESIGN.md.

Entries are (tag, agent_x, agent_z, agent_dir, box_pose_or_None), box_pose = (box index, x, z, dir).  Tags are
"<family>:<group ...>:<index in group>"; group(tag) names the sweep or pair a pose belongs to.
  A  axis-aligned headings k pi/2 and their float64 neighbours, at the agent's position and at the centres of junction rooms
  B  eye on a portal plane: the opening's midpoint and 1/8 points, looking across (0.3 rad off the normal, and on the axis) and along it
  C  eye 1e-7, 1e-3 and 0.05 m from an unportalled wall, headings 1e-3 rad off parallel, and head-on at 0.05 m
  D  a box's silhouette taken through the frame's four borders in quarter-pixel steps, and faces exactly edge-on / face-on
  E  entities' bounding circles at the frame's side borders; image / text frames seen from inside their own front plane
"""
import math

import numpy as np

EDGE_TOL = 1e-9
NEAR = 0.05
JAMB_SHARE = 1.0 / 8
MAX_SITES = 6          # junction rooms (A) and shared edges (B) of the maze tasks: the nearest ones
MAX_ENTS = 4           # entities per world (E)
BOX_DIST = 2.0         # family D: the box's distance from the eye
SWEEP = [j * 0.25 for j in range(-8, 9)]   # quarter-pixel steps, 2 pixels either side of an event


def family(tag):
    return tag[0]


def group(tag):
    return tag.rsplit(":", 1)[0]


def heading_vec(d):
    """the agent's forward direction in (x, z) (entity.py:437-444: dir_vec = (cos d, 0, -sin d))"""
    return np.array([math.cos(d), -math.sin(d)])


def bearing(frm, to):
    return math.atan2(-(to[1] - frm[1]), to[0] - frm[0])


def room_polys(geo):
    """[(room index, (n, 2) outline)] of the rooms that are drawn: YMaze's connector slivers have the opposite winding (culled)"""
    out = []
    for r, o in enumerate(geo["outline"]):
        o = o[~np.isnan(o[:, 0])]
        x, z = o[:, 0], o[:, 1]
        if (x * np.roll(z, -1) - np.roll(x, -1) * z).sum() < 0:
            out.append((r, o))
    return out


def edge_dists(o, p):
    """inward signed distance of point p from each edge's line of outline o"""
    a, b = o, np.roll(o, -1, axis=0)
    e = b - a
    return (e[:, 1] * (p[0] - a[:, 0]) - e[:, 0] * (p[1] - a[:, 1])) / np.hypot(e[:, 0], e[:, 1])


class Geom:
    """the drawn rooms' edges and the wall segments as arrays; f32: every coordinate rounded to float32, as the renderers hold them"""

    def __init__(self, geo, f32=False):
        rnd = (lambda a: np.asarray(a, np.float32).astype(np.float64)) if f32 else (lambda a: np.asarray(a, np.float64))
        self.geo = geo
        self.polys = [(r, rnd(o)) for r, o in room_polys(geo)]
        n = len(self.polys)
        self.a, self.e, self.valid = np.zeros((n, 4, 2)), np.ones((n, 4, 2)), np.zeros((n, 4), bool)
        for i, (r, o) in enumerate(self.polys):
            k = len(o)
            self.a[i, :k], self.e[i, :k], self.valid[i, :k] = o, np.roll(o, -1, axis=0) - o, True
        self.len = np.hypot(self.e[..., 0], self.e[..., 1])
        segs = rnd(geo["wall_segs"]).reshape(-1, 4)
        self.sa, self.sd = segs[:, 0:2], segs[:, 2:4] - segs[:, 0:2]

    def rooms_violation(self, eye):
        dist = (self.e[..., 1] * (eye[0] - self.a[..., 0]) - self.e[..., 0] * (eye[1] - self.a[..., 1])) / self.len
        dist = np.where(self.valid, dist, np.inf)
        if (dist > EDGE_TOL).all(axis=1).any():
            inside = True
        else:
            inside = False
        on_edges = 0
        for i in np.nonzero((dist >= -EDGE_TOL).all(axis=1) & ~(dist > EDGE_TOL).all(axis=1))[0]:
            r, o = self.polys[i]
            on = np.nonzero(np.abs(dist[i]) <= EDGE_TOL)[0]
            if len(on) != 1:
                return "on a vertex of room %d" % r
            k = int(on[0])
            along = float((eye - o[k]) @ self.e[i, k]) / float(self.len[i, k])
            ok = False
            for q in range(self.geo["portal_count"][r][k]):
                st, en = self.geo["portals"][r][k][q][:2]
                m = JAMB_SHARE * (en - st) - 1e-12
                ok |= bool(st + m <= along <= en - m)
            if not ok:
                return "on a wall plane or jamb of room %d" % r
            on_edges += 1
        if not inside and on_edges < 2:
            return "outside every room" if on_edges == 0 else "on an unshared edge"
        return None

    def faced_wall(self, eye, d):
        f = heading_vec(d)
        t = np.clip(((eye - self.sa) * self.sd).sum(axis=1) / (self.sd * self.sd).sum(axis=1), 0.0, 1.0)
        v = self.sa + t[:, None] * self.sd - eye
        dist = np.hypot(v[:, 0], v[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            bad = (dist < NEAR - 1e-12) & (dist > 0) & ((v @ f) / dist >= math.cos(math.pi / 4))
        return "%.3g m from a wall it faces" % dist[bad].min() if bad.any() else None

    def free_distance(self, p, f):
        """distance from p along unit vector f to the nearest wall segment"""
        den = f[0] * self.sd[:, 1] - f[1] * self.sd[:, 0]
        w = self.sa - p
        with np.errstate(divide="ignore", invalid="ignore"):
            t, u = (w[:, 0] * self.sd[:, 1] - w[:, 1] * self.sd[:, 0]) / den, (w[:, 0] * f[1] - w[:, 1] * f[0]) / den
        hit = (np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1)
        return float(t[hit].min()) if hit.any() else math.inf


def rule_violation(eye, d, G, s, frames=()):
    """None if the eye (x, z) with heading d is admissible, else the reason.  G: (Geom in float64, Geom in float32)"""
    eye = np.asarray(eye, float)
    eye32 = eye.astype(np.float32).astype(np.float64)
    why = G[0].rooms_violation(eye) or G[0].faced_wall(eye, d)
    why = why or (lambda w: w and "as float32: " + w)(G[1].rooms_violation(eye32))
    if why:
        return why
    for b in range(s.n_boxes):
        if s.ents_alive[b] and s.ents_radius[b] > 0 and math.hypot(eye[0] - s.boxes_pos[b][0], eye[1] - s.boxes_pos[b][2]) <= s.ents_radius[b]:
            return "inside entity %d" % b
    for fr in frames:
        lx, lz = fr.local(eye)
        if -EDGE_TOL <= lx <= fr.depth + EDGE_TOL and abs(lz) <= fr.half_w + EDGE_TOL:
            return "inside frame %d" % fr.index
    return None


class Frame:
    """an ImageFrame / TextFrame: a slab [0, depth] x [-w/2, w/2] in its own x / z axes, the picture on its +x face"""

    def __init__(self, index, s, tex_sizes):
        self.index = index
        self.pos = np.array([s.boxes_pos[index][0], s.boxes_pos[index][2]])
        self.dir = s.boxes_dir[index]
        self.normal = heading_vec(self.dir)
        self.tangent = np.array([math.sin(self.dir), math.cos(self.dir)])
        self.depth = 0.05   # entity.py:148-360: every frame's depth
        tex = [t for t in s.ents_tex[index] if t >= 0]
        if s.ents_kind[index] == 2:   # ImageFrame: height = width * tex.height / tex.width
            w, h = tex_sizes[tex[0]][:2]
            self.half_w = 0.5 * s.ents_height[index] * w / h
        else:                         # TextFrame: one square cell of the frame's height per character
            self.half_w = 0.5 * s.ents_height[index] * sum(1 for t in s.ents_tex[index] if t != -1)

    def local(self, p):
        v = np.asarray(p, float) - self.pos
        return float(v @ self.normal), float(v @ self.tangent)


def overlap_junctions(geo):
    """room corners that lie inside another drawn room, or within 2 cm of it without touching it: YMaze's arms overlap its hub by a
    centimetre (envs/ymaze.py:39-52), so two wall ends nearly coincide there.  The z-buffer shows whichever is nearer, the portal
    traversal the one of the room it is in: the pixel column of such a corner is ill-defined (test_oracle_render.py,
    test_ymaze_random_views_against_bruteforce_rendition; measured at this catalogue's poses: one column, 0.85 % of the frame off by 2,
    from the hub's centre; two columns, 1.19 % off by up to 4, from a point 0.5 m off it).  Rooms that touch exactly (every other
    task) have none."""
    polys = room_polys(geo)
    out = []
    for r, o in polys:
        for v in o:
            for r2, o2 in polys:
                if r2 == r:
                    continue
                a, e = o2, np.roll(o2, -1, axis=0) - o2
                t = np.clip(((v - a) * e).sum(axis=1) / (e * e).sum(axis=1), 0.0, 1.0)
                near = float(np.hypot(*(a + t[:, None] * e - v).T).min())
                if (edge_dists(o2, v) > EDGE_TOL).all() or EDGE_TOL < near < 0.02:
                    out.append(v)
                    break
    return out


def sees_overlap_junction(junctions, eye, d, hfov):
    """rule 6, for the brute-force arbitration only: does an overlap junction fall into the frame (or within 0.05 rad of its side)?"""
    return any(abs(math.remainder(bearing(eye, j) - d, 2 * math.pi)) <= hfov + 0.05 for j in junctions)


def junction_rooms(geo):
    """rooms connect_rooms made between two rooms that do not touch (miniworld.py:757-843): exactly the edges 1 and 3 are open, over
    their whole length, and the room is smaller than the rooms it joins"""
    polys = room_polys(geo)
    area = {r: abs(float((o[:, 0] * np.roll(o[:, 1], -1) - np.roll(o[:, 0], -1) * o[:, 1]).sum())) / 2 for r, o in polys}
    mean = sum(area.values()) / len(area)
    out = []
    for r, o in polys:
        pc = list(geo["portal_count"][r])
        if len(o) == 4 and pc == [0, 1, 0, 1] and area[r] < mean:
            whole = all(geo["portals"][r][k][0][0] == 0 and abs(geo["portals"][r][k][0][1] - np.linalg.norm(o[(k + 1) % 4] - o[k])) < 1e-9 for k in (1, 3))
            if whole:
                out.append((r, o.mean(axis=0)))
    return out


def shared_edges(geo):
    """[(a, unit edge direction, inward normal, start, end)] for every portal of every drawn room, one entry per plane"""
    out, seen = [], set()
    for r, o in room_polys(geo):
        for k in range(len(o)):
            for q in range(geo["portal_count"][r][k]):
                a, b = o[k], o[(k + 1) % len(o)]
                e = (b - a) / np.linalg.norm(b - a)
                st, en = geo["portals"][r][k][q][:2]
                mid = a + e * (st + en) / 2
                key = (round(float(mid[0]), 6), round(float(mid[1]), 6))
                if key in seen:
                    continue
                seen.add(key)
                out.append((a, e, np.array([e[1], -e[0]]), float(st), float(en)))
    return out


def catalogue(env, W=None, H=None, tex_sizes=None):
    """env: an OracleEnv after reset(render=False) (or any later state).  The agent is moved while the catalogue is built and put
    back before it returns.  W, H: the frame the poses are meant for (default the env's own).  tex_sizes: texture id -> (w, h),
    needed for the worlds with an ImageFrame."""
    W, H = W or env.W, H or env.H
    geo, s0 = env.geometry(), env.state()
    G = (Geom(geo), Geom(geo, f32=True))
    base = np.array([s0.agent_pos[0], s0.agent_pos[2]])
    base_dir = s0.agent_dir
    fwd = s0.cam_fwd_disp
    th = math.tan(math.radians(s0.cam_fov_y) / 2)
    tw = th * W / H
    hfov = math.atan(tw)
    frames = [Frame(b, s0, tex_sizes) for b in range(s0.n_boxes) if s0.ents_alive[b] and s0.ents_kind[b] in (2, 3)]
    out = []

    def emit(tag, eye, d, box=None, optional=False):
        """the agent that puts the EYE at `eye` (cam_pos = agent_pos + cam_fwd_disp * dir_vec, entity.py:457-470)"""
        ag = np.asarray(eye, float) - fwd * heading_vec(d)
        env.set_agent(float(ag[0]), float(ag[1]), float(d))
        if box is not None:
            env.set_box(*box)
        s = env.state()
        why = rule_violation((s.cam_pos[0], s.cam_pos[2]), d, G, s, frames)
        if why is not None and (optional or why.startswith("inside")):   # rule 4 depends on where the world's entities happen to be
            return False
        assert why is None, (tag, why, tuple(s.cam_pos), d)
        out.append((tag, float(ag[0]), float(ag[1]), float(d), box))
        return True

    by_dist = lambda pts: sorted(range(len(pts)), key=lambda i: float(np.hypot(*(pts[i] - base))))   # noqa: E731

    # ---- A: axis-aligned headings
    heads = []
    for k in range(-2, 3):
        h = k * (math.pi / 2)
        heads += [float(np.nextafter(h, -np.inf)), h, float(np.nextafter(h, np.inf))]
    assert 0.0 in heads and math.pi in heads and -math.pi in heads
    junc = [c for _, c in junction_rooms(geo)]
    if env.task == "YMaze":   # its junction is the triangular hub
        junc = [o.mean(axis=0) for _, o in room_polys(geo) if len(o) == 3]
    junc = [junc[i] for i in by_dist(junc)[:MAX_SITES]]
    for i, h in enumerate(heads):   # the agent stays where it is
        emit("A:p0:%02d" % i, base + fwd * heading_vec(h), h)
    for p, site in enumerate(junc):
        for i, h in enumerate(heads):
            emit("A:p%d:%02d" % (p + 1, i), site, h)

    # ---- B: eye on a portal plane
    edges = shared_edges(geo)
    mids = [a + e * (st + en) / 2 for a, e, n, st, en in edges]
    order = by_dist(mids)
    if env.task == "Maze":
        order = order[:MAX_SITES]
    for j, ei in enumerate(order):
        a, e, n, st, en = edges[ei]
        phi = bearing((0, 0), n)
        ka = int(round(phi / (math.pi / 2)))   # the axis nearest the normal (the normal itself for an axis-aligned edge), as k pi/2 exactly
        ka = ka if abs(ka) <= 2 else ka - 4 * (1 if ka > 0 else -1)
        axis = [ka * (math.pi / 2), (ka + 2 if ka <= 0 else ka - 2) * (math.pi / 2)]
        hs = [phi + 0.3, phi + math.pi + 0.3, phi - 0.3, phi + math.pi - 0.3, None, None, phi + math.pi / 2, phi - math.pi / 2]
        for q, share in enumerate((0.5, JAMB_SHARE, 1 - JAMB_SHARE)):
            eye = a + e * (st + share * (en - st))
            for i, h in enumerate(hs):
                emit("B:e%d:q%d:%s:%d" % (j, q, ("in", "out")[i % 2] if i < 6 else "along", i), eye, axis[i - 4] if h is None else math.remainder(h, 2 * math.pi))

    # ---- C: near an unportalled wall of the agent's room (else of the nearest room that has one)
    walls, own = [], []
    for r, o in room_polys(geo):
        for k in range(len(o)):
            if geo["portal_count"][r][k] == 0:
                a, b = o[k], o[(k + 1) % len(o)]
                walls.append(((a + b) / 2, (b - a) / np.linalg.norm(b - a)))
                if (edge_dists(o, base) > 0).all():
                    own.append(walls[-1])
    walls = own or walls
    for i in by_dist([w[0] for w in walls]):   # the nearest wall that no entity sits at
        mid, e = walls[i]
        n = np.array([e[1], -e[0]])
        psi = bearing((0, 0), e)
        mark, ok = len(out), True
        tiny = 1e-7   # doubled until the eye is off the wall plane as a float32 too (rule 5)
        while G[1].rooms_violation((mid + n * tiny).astype(np.float32).astype(np.float64)) is not None and tiny < 1e-4:
            tiny *= 2
        for k, dist in enumerate((tiny, 1e-3, NEAR)):
            ok &= emit("C:d%d:0" % k, mid + n * dist, psi - 1e-3)
            ok &= emit("C:d%d:1" % k, mid + n * dist, psi + 1e-3)
        ok &= emit("C:d2:2", mid + n * NEAR, bearing((0, 0), -n))
        if ok:
            break
        del out[mark:]

    # ---- D: box silhouettes through the frame's borders (box-only tasks, the eye at the agent: no domain randomisation)
    box_task = s0.n_boxes > 0 and all(s0.ents_kind[b] == 0 for b in range(s0.n_boxes)) and not frames
    if box_task and s0.n_boxes <= 2 and fwd == 0 and s0.cam_pitch == 0 and rule_violation(base, base_dir, G, s0) is None:
        cand = [k * (2 * math.pi / 64) - math.pi + 0.01 for k in range(64)]
        b0 = max(cand, key=lambda c: G[0].free_distance(base, heading_vec(c)))
        px_w = hfov - math.atan(tw * (1 - 2.0 / W))
        for b in range(s0.n_boxes):
            half, bdir = s0.boxes_size[b] / 2, s0.boxes_dir[b]
            centre = base + BOX_DIST * heading_vec(b0)
            c_, s_ = math.cos(bdir), math.sin(bdir)
            rel = []
            for lx, lz in ((-half, -half), (-half, half), (half, -half), (half, half)):
                corner = centre + np.array([c_ * lx + s_ * lz, -s_ * lx + c_ * lz])
                rel.append(math.remainder(bearing(base, corner) - b0, 2 * math.pi))
            box = (b, float(centre[0]), float(centre[1]), float(bdir))
            for side, sg in (("L", 1.0), ("R", -1.0)):
                for ev, r_ in (("hi", max(rel)), ("lo", min(rel))):
                    for i, q in enumerate(SWEEP):
                        emit("D:b%d:%s:%s:%02d" % (b, side, ev, i), base, math.remainder(b0 + r_ - sg * hfov + q * px_w, 2 * math.pi), box)
            # approach along the central ray, the near face square to it: its bottom and its top edge cross the frame's bottom border
            for ev, hgt in (("bottom", s0.cam_height), ("top", s0.cam_height - s0.boxes_size[b])):
                for i, q in enumerate(SWEEP):
                    y_ndc = -1.0 + q * (2.0 / H)
                    dist = hgt / (th * -y_ndc) + half
                    c2 = base + dist * heading_vec(b0)
                    emit("D:b%d:near:%s:%02d" % (b, ev, i), base, b0, (b, float(c2[0]), float(c2[1]), float(b0)))
            # faces exactly face-on / edge-on: dir = heading + k pi/2; shifted sideways by half a box a side face's plane holds the eye
            side_v = np.array([heading_vec(b0)[1], -heading_vec(b0)[0]])
            for k in range(4):
                for i, off in enumerate((0.0, half, -half)):
                    c2 = centre + off * side_v
                    emit("D:b%d:square:k%d:%d" % (b, k, i), base, b0, (b, float(c2[0]), float(c2[1]), float(b0 + k * (math.pi / 2))))

    # ---- E: entities (only the agent moves)
    if not box_task and s0.n_boxes and rule_violation(base + fwd * heading_vec(base_dir), base_dir, G, s0, frames) is None:
        eye_of = lambda d: base + fwd * heading_vec(d)   # noqa: E731  the agent stays where it is
        n = 0
        for b in range(s0.n_boxes):
            if not s0.ents_alive[b] or s0.ents_radius[b] <= 0 or n == MAX_ENTS:
                continue
            c = np.array([s0.boxes_pos[b][0], s0.boxes_pos[b][2]])
            dist = float(np.hypot(*(c - base)))
            if dist <= s0.ents_radius[b] or G[0].free_distance(base, (c - base) / dist) < dist:   # inside it, or a wall in between
                continue
            n += 1
            a_, beta = math.asin(s0.ents_radius[b] / dist), bearing(base, c)
            i = 0
            for side, sg in (("L", 1.0), ("R", -1.0)):   # the bounding circle tangent to the border outside / inside, and half way each
                for off in (a_, -a_, a_ / 2, -a_ / 2):
                    d = math.remainder(beta - sg * (hfov + off), 2 * math.pi)
                    emit("E:e%d:%d" % (b, i), eye_of(d), d)
                    i += 1
        for fr in frames:   # from inside the front face's plane, beyond the frame's end: the picture exactly edge-on, and 1e-3 rad off
            i = 0
            for sg in (1.0, -1.0):
                eye = fr.pos + fr.depth * fr.normal + sg * max(1.5, fr.half_w + 0.375) * fr.tangent
                look = bearing((0, 0), -sg * fr.tangent)
                for d in (look, look + 1e-3, look - 1e-3):
                    if emit("E:f%d:edge:%d" % (fr.index, i), eye, math.remainder(d, 2 * math.pi), optional=True):
                        i += 1
            assert i >= 3, ("no admissible edge-on pose for frame", fr.index)

    env.set_agent(float(base[0]), float(base[1]), float(base_dir))
    for b in range(s0.n_boxes if box_task else 0):
        env.set_box(b, s0.boxes_pos[b][0], s0.boxes_pos[b][2], s0.boxes_dir[b])
    fams = {family(t[0]) for t in out}
    assert "A" in fams and "C" in fams, fams
    assert len({t[0] for t in out}) == len(out), "tags are unique"
    return out


def pose(env, entry):
    """put an OracleEnv into a catalogue entry's pose"""
    _, x, z, d, box = entry
    env.set_agent(x, z, d)
    if box is not None:
        env.set_box(box[0], box[1], box[2], box[3])


def strided(entries, n):
    """n entries at an even stride through the list (not its head)"""
    if len(entries) <= n:
        return list(entries)
    return [entries[min(len(entries) - 1, int((k + 0.5) * len(entries) / n) + k)] for k in range(n)]


def check_box_sweep(g, v):
    """family D's non-vacuity: g a group tag, v its frames' (any box pixel, any in the bottom row, any in the two border columns)"""
    leaving = g.endswith(":L:lo") or g.endswith(":R:hi")
    if ":L:" in g or ":R:" in g:
        assert any(c for _, _, c in v) and not all(c for _, _, c in v), (g, v)
    if leaving:
        assert any(a for a, _, _ in v) and not all(a for a, _, _ in v), (g, v)
    else:
        assert all(a for a, _, _ in v), (g, v)
    if g.endswith(":near:bottom"):
        assert any(r for _, r, _ in v) and not all(r for _, r, _ in v), (g, v)
