"""Directed start states for MiniWorldEnv.step at its decision edges (plain NumPy: no GPU, no oracle, no reference).

Every threshold of a step is a strict `<` on a float64 distance that a random rollout lands within a few ulps of essentially
never.  This module builds CASE GROUPS: eight start states that differ in ONE start coordinate, four on either side of the
pair of adjacent doubles s0 < s1 on which a float64 restatement of the reference's predicate flips (s0 - 3 ulp .. s0 and
s1 .. s1 + 3 ulp).  The restatement - intersect_circle_segs (math.py:25-57), MiniWorldEnv.intersect / near / _get_carry_pos
and the pickup probe (miniworld.py:933-971, 594-606, 682-689) - is written with the NumPy calls of the reference and is
handed the reference's own scalars: an `np.float32` radius stays an np.float32, so that under NumPy >= 2 a sum such as
`agent.radius + ent.radius` is a float32 exactly where the reference's is.  tests/golden/gen_fixtures_step_edges.py feeds it
the worlds of the unmodified reference and records what the reference then does; whether a group straddles its decision is
judged by those recorded outcomes, never by the restatement.

Headings are never axis-aligned: every family turns its approach direction by HEADING_OFFSETS, so that the sine and the cosine
of agent.dir and the association (a + c * fd) + s * drift are part of every decision.

A candidate is dropped when anything but the intended obstacle lies within threshold + MARGIN of the decisive point.  One
exception, recorded per group as `margin`: the 0.25 m side walls of a Maze's connecting passages have the rooms' own walls as
collinear neighbours 0.019 m farther from any landing point, so the groups that hold only such segments are built with
MARGIN_TIGHT - the neighbours still stand 1e14 ulps behind the decision."""
import math

import numpy as np

FAMILIES = ("wall_interior", "wall_endpoint", "agent_entity", "agent_entity_two", "near_done", "pickup_reach", "pickup_two", "pickup_wall",
            "carry_move_wall", "carry_move_entity", "carry_turn_wall", "carry_turn_entity", "putnext_rule", "near_3d",
            "push_shove", "push_goal")
FAMILY_ID = {n: i for i, n in enumerate(FAMILIES)}
HEADING_OFFSETS = (0.45, -0.7, 1.0, -0.3, 0.8, -1.1)   # radians off the straight approach: sines and cosines in 0.29 .. 0.96
MARGIN, MARGIN_TIGHT = 0.05, 0.01
GROUP = 8


class World:
    """What a step reads of a world that does not change within a group.  segs [n, 4] float64 (a.x a.z b.x b.z); radius /
    height: the entities' scalars AS THE REFERENCE HOLDS THEM (float or np.float32), list order = entity-list order without
    the agent, which is the list's last entry; arad the agent's radius; fwd_step / fwd_drift / turn_step what
    params.sample(None, ...) returns; max_fwd = env.max_forward_step; cam_height the agent's."""

    def __init__(self, segs, radius, height, static, arad, max_fwd, fwd_step, fwd_drift, turn_step, cam_height):
        segs = np.asarray(segs, np.float64).reshape(-1, 4)
        self.segs = segs
        self.segs3 = np.zeros((len(segs), 2, 3))
        self.segs3[:, 0, 0], self.segs3[:, 0, 2], self.segs3[:, 1, 0], self.segs3[:, 1, 2] = segs.T
        self.radius, self.height, self.static = list(radius), list(height), list(static)
        self.E = len(self.radius)
        self.arad, self.max_fwd, self.fwd_step, self.fwd_drift, self.turn_step, self.cam_height = arad, max_fwd, fwd_step, fwd_drift, turn_step, cam_height


def make_state(agent_pos, agent_dir, ents_pos, ents_dir, carrying=-1, step_count=0):
    return {"agent_pos": np.array(agent_pos, np.float64), "agent_dir": float(agent_dir), "ents_pos": np.array(ents_pos, np.float64).reshape(-1, 3),
            "ents_dir": np.array(ents_dir, np.float64).reshape(-1), "carrying": int(carrying), "step_count": int(step_count)}


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


# ------------------------------------------------------------------------------------------- the reference's predicates, restated
def dir_vec(d):
    return np.array([math.cos(d), 0, -math.sin(d)])


def right_vec(d):
    return np.array([math.sin(d), 0, math.cos(d)])


def seg_dists(w, point):
    """intersect_circle_segs up to its comparison: the distance of every segment's closest point"""
    px, _, pz = point
    point = np.array([px, 0, pz])
    a, b = w.segs3[:, 0, :], w.segs3[:, 1, :]
    ab, ap = b - a, point - a
    proj = np.sum(ap * ab, axis=1) / np.sum(ab * ab, axis=1)
    proj = np.expand_dims(np.clip(proj, 0, 1), axis=1)
    return np.linalg.norm((a + proj * ab) - point, axis=1)


def seg_proj(w, point, j):
    a, b = w.segs3[j, 0], w.segs3[j, 1]
    p = np.array([point[0], 0, point[2]])
    return float(np.sum((p - a) * (b - a)) / np.sum((b - a) * (b - a)))


def add(x, y, sum64):
    """x + y as NumPy adds the reference's scalars, or - for the groups that show the rule matters - in float64 throughout"""
    return float(x) + float(y) if sum64 else x + y


def intersect(w, st, self_idx, pos, radius, sum64=False, walls=True):
    """MiniWorldEnv.intersect -> 0 nothing, 1 a wall, 2 + k entity k (w.E = the agent, the last of the list)"""
    px, _, pz = pos
    pos = np.array([px, 0, pz])
    if walls and len(w.segs) and np.any(np.less(seg_dists(w, pos), radius)):
        return 1
    for k in range(w.E + 1):
        if k == self_idx:
            continue
        p = st["agent_pos"] if k == w.E else st["ents_pos"][k]
        pos2 = np.array([p[0], 0, p[2]])
        d = np.linalg.norm(pos2 - pos)
        if d < add(radius, w.arad if k == w.E else w.radius[k], sum64):
            return 2 + k
    return 0


def near_threshold(w, i, j, sum64=False):
    ri = w.arad if i == w.E else w.radius[i]
    rj = w.arad if j == w.E else w.radius[j]
    return add(add(ri, rj, sum64), 1.1 * w.max_fwd, sum64)


def near(w, st, i, j=None, sum64=False, agent_pos=None):
    j = w.E if j is None else j
    pos = lambda k: (st["agent_pos"] if agent_pos is None else agent_pos) if k == w.E else st["ents_pos"][k]   # noqa: E731
    return bool(np.linalg.norm(pos(i) - pos(j)) < near_threshold(w, i, j, sum64))


def carry_pos(w, agent_pos, d, k, sum64=False):
    dist = add(add(w.arad, w.radius[k], sum64), w.max_fwd, sum64)
    pos = agent_pos + dir_vec(d) * 1.05 * dist
    y_pos = max(add(add(w.cam_height, -w.height[k], sum64), -0.3, sum64), 0)
    return pos + np.array([0, 1, 0]) * y_pos


def move_target(w, st, action):
    fd = w.fwd_step if action == 2 else -w.fwd_step
    return st["agent_pos"] + dir_vec(st["agent_dir"]) * fd + right_vec(st["agent_dir"]) * w.fwd_drift


def move_verdict(w, st, action, sum64=False):
    """move_agent -> (what stopped the agent's circle, what stopped the carried entity's): (0, 0) = the move happens"""
    nxt = move_target(w, st, action)
    hit = intersect(w, st, w.E, nxt, w.arad, sum64)
    if hit or st["carrying"] < 0:
        return hit, 0
    k = st["carrying"]
    return 0, intersect(w, st, k, carry_pos(w, nxt, st["agent_dir"], k, sum64), w.radius[k], sum64)


def turn_verdict(w, st, action, sum64=False):
    d = st["agent_dir"] + (w.turn_step if action == 0 else -w.turn_step) * (math.pi / 180)
    k = st["carrying"]
    return 0 if k < 0 else intersect(w, st, k, carry_pos(w, st["agent_pos"], d, k, sum64), w.radius[k], sum64)


def pickup_verdict(w, st, sum64=False):
    test_pos = st["agent_pos"] + dir_vec(st["agent_dir"]) * 1.5 * w.arad
    return intersect(w, st, w.E, test_pos, 1.2 * w.arad, sum64)


# ------------------------------------------------------------------------------------------------------------- bisection
def ulps(x, k):
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def bisect(f, lo, hi):
    """adjacent doubles s0 < s1 between lo and hi with f(s0) != f(s1), or None when f(lo) == f(hi)"""
    flo = f(lo)
    if flo == f(hi):
        return None
    while math.nextafter(lo, hi) != hi:
        mid = lo + (hi - lo) / 2
        if mid == lo or mid == hi:
            mid = math.nextafter(lo, hi)
        if f(mid) == flo:
            lo = mid
        else:
            hi = mid
    return (lo, hi) if lo < hi else (hi, lo)


def group_values(s0, s1):
    return [ulps(s0, -k) for k in (3, 2, 1, 0)] + [ulps(s1, k) for k in (0, 1, 2, 3)]


def vary_agent(axis):
    def put(st, v):
        st = copy_state(st)
        st["agent_pos"][axis] = v
        return st
    return put


def vary_ent(k, axis):
    def put(st, v):
        st = copy_state(st)
        st["ents_pos"][k, axis] = v
        return st
    return put


def build_group(family, w, base, action, put, centre, verdict, sub=0, reach=1e-3, **info):
    """the group around the flip of verdict(state) between centre - reach and centre + reach of the varied coordinate"""
    edge = bisect(lambda v: verdict(put(base, v)), centre - reach, centre + reach)
    if edge is None:
        return None
    g = {"family": family, "sub": sub, "action": action, "states": [put(base, v) for v in group_values(*edge)], "decider": -1, "margin": MARGIN, "clamp": -1}
    g.update(info)
    return g


def isolated(w, st, point, radius, margin, skip_segs=(), skip_ents=(), self_idx=None, walls=True):
    """nothing but the skipped obstacles within threshold + margin of the decisive point"""
    if walls and len(w.segs):
        d = seg_dists(w, point)
        keep = np.ones(len(d), bool)
        keep[list(skip_segs)] = False
        if np.any(d[keep] < radius + margin):
            return False
    for k in range(w.E + 1):
        if k in skip_ents or k == self_idx:
            continue
        p = st["agent_pos"] if k == w.E else st["ents_pos"][k]
        if math.hypot(p[0] - point[0], p[2] - point[2]) < float(radius) + float(w.arad if k == w.E else w.radius[k]) + margin:
            return False
    return True


def heading_of(u):
    """agent.dir whose dir_vec is the unit vector (u[0], 0, u[1])"""
    return math.atan2(-u[1], u[0])


def rot(u, ang):
    c, s = math.cos(ang), math.sin(ang)
    return np.array([c * u[0] - s * u[1], s * u[0] + c * u[1]])


def start_for_landing(w, base, land, u, action):
    """the state from which `action` (2 forward, 3 back) moves the agent's centre to `land` along the direction u"""
    d = heading_of(u if action == 2 else -u)
    st = copy_state(base)
    st["agent_dir"] = d
    st["agent_pos"] = np.zeros(3)
    move = move_target(w, st, action)
    st["agent_pos"] = np.array([land[0], 0, land[1]]) - move
    return st


def main_axis(v):
    return 0 if abs(v[0]) >= abs(v[1]) else 2


# ---------------------------------------------------------------------------------------------------------------- families
def seg_frame(w, j):
    a, b = w.segs[j, :2], w.segs[j, 2:]
    t = (b - a) / np.linalg.norm(b - a)
    return a, b, t, np.array([-t[1], t[0]])


def wall_interior_group(w, base, j, action, off, margins=(MARGIN,)):
    """the move lands the circle's centre `arad` from the interior of segment j"""
    a, b, t, n0 = seg_frame(w, j)
    for margin in margins:
        for frac in (0.5, 0.37, 0.63):
            for n in (n0, -n0):
                foot = a + frac * (b - a)
                land = foot + n * w.arad
                u = rot(-n, off)
                if min(abs(u[0]), abs(u[1])) < 0.1:   # a slanted wall may turn the offset heading back onto an axis
                    u = rot(u, 0.3)
                st = start_for_landing(w, base, land, u, action)
                if st["carrying"] >= 0 or not isolated(w, st, (land[0], 0, land[1]), w.arad, margin, skip_segs=(j,), self_idx=w.E):
                    continue
                if not 0.02 < seg_proj(w, (land[0], 0, land[1]), j) < 0.98:
                    continue
                ax = main_axis(n)
                g = build_group("wall_interior", w, st, action, vary_agent(ax), st["agent_pos"][ax], lambda s: move_verdict(w, s, action)[0] != 0,
                                decider=j, margin=margin)
                if g is not None:
                    return g
    return None


def end_points(w):
    """(point, [(segment, 0 for its a end / 1 for its b end), ...]) for every point where segments end"""
    pts = {}
    for j in range(len(w.segs)):
        for end in (0, 1):
            p = w.segs[j, 2 * end:2 * end + 2]
            pts.setdefault((round(float(p[0]), 9), round(float(p[1]), 9)), []).append((j, end))
    return [(w.segs[lst[0][0], 2 * lst[0][1]:2 * lst[0][1] + 2].copy(), lst) for _, lst in sorted(pts.items())]


def wall_endpoint_group(w, base, point, action, off, quadrant):
    """the landing point is `arad` from a point where walls end (a jamb), on a diagonal past the end of every wall that ends
    there: proj clamps for each of them - to 1 where the point is the segment's b end, to 0 where it is its a end"""
    p, lst = point
    _, _, t, n = seg_frame(w, lst[0][0])
    v = rot(t, math.pi / 4 + quadrant * math.pi / 2)
    land = p + v * w.arad
    pt = (land[0], 0, land[1])
    st = start_for_landing(w, base, land, rot(-v, off), action)
    skip = [j for j, _ in lst]
    if not isolated(w, st, pt, w.arad, MARGIN, skip_segs=skip, self_idx=w.E):
        return None
    if not all(seg_proj(w, pt, j) > 1.05 if end else seg_proj(w, pt, j) < -0.05 for j, end in lst):
        return None
    ax = main_axis(v)
    return build_group("wall_endpoint", w, st, action, vary_agent(ax), st["agent_pos"][ax], lambda s: move_verdict(w, s, action)[0] != 0,
                       decider=skip[0], clamp=int(lst[0][1]))


def agent_entity_group(w, base, k, action, theta, sum64=False):
    """the move stops at arad + radius(k); sum64: the group around the threshold a float64 sum would give (sub 1)"""
    u = np.array([math.cos(theta), -math.sin(theta)])
    thr = float(add(w.arad, w.radius[k], sum64))
    if sum64 and thr == float(add(w.arad, w.radius[k], False)):
        return None   # the two sums agree to the last bit (RoomObjs: 1.5 + radius is exact in float32): nothing to show
    e = base["ents_pos"][k][[0, 2]]
    land = e - u * thr
    st = start_for_landing(w, base, land, u, action)
    if not isolated(w, st, (land[0], 0, land[1]), w.arad, MARGIN, skip_ents=(k,), self_idx=w.E):
        return None
    ax = main_axis(u)
    return build_group("agent_entity", w, st, action, vary_agent(ax), st["agent_pos"][ax], lambda s: move_verdict(w, s, action, sum64)[0], sub=int(sum64), decider=k)


def agent_entity_two_group(w, base, k, m, action, theta):
    """entities k < m, both at their thresholds of one landing point: along the group the move is stopped by m alone, then by
    both - where intersect has to name k, the lower index - then by k alone.  Entity m is moved to where that happens."""
    assert k < m
    u = np.array([math.cos(theta), -math.sin(theta)])
    e = base["ents_pos"][k][[0, 2]]
    land = e - u * float(w.arad + w.radius[k])
    um = rot(u, 2.1)   # m stands 120 degrees off the approach: the move that closes in on k backs away from m
    base = copy_state(base)
    tm = float(w.arad + w.radius[m])
    base["ents_pos"][m] = [land[0] + um[0] * (tm + 1e-3), 0, land[1] + um[1] * (tm + 1e-3)]
    st = start_for_landing(w, base, land, u, action)
    if not isolated(w, st, (land[0], 0, land[1]), w.arad, MARGIN, skip_ents=(k, m), self_idx=w.E):
        return None
    ax = main_axis(u)
    put = vary_agent(ax)
    edge = bisect(lambda v: move_verdict(w, put(st, v), action)[0] == 2 + k, st["agent_pos"][ax] - 1e-3, st["agent_pos"][ax] + 1e-3)
    if edge is None:
        return None
    vals = group_values(*edge)
    toward = move_verdict(w, put(st, vals[-1]), action)[0] == 2 + k   # does the coordinate grow towards k?
    both = vals[5] if toward else vals[2]   # the second value on k's side: from there outwards m must let go
    axm = main_axis(um)
    putm = vary_ent(m, axm)
    stb = put(st, both)
    only_m = lambda s: intersect(w, s, k, move_target(w, s, action), w.arad) == 2 + m   # noqa: E731  (k left out: is m in reach?)
    cm = land[0 if axm == 0 else 1] + um[0 if axm == 0 else 1] * tm
    em = bisect(lambda v: only_m(putm(stb, v)), cm - 2e-3, cm + 2e-3)
    if em is None:
        return None
    cin = em[0] if only_m(putm(stb, em[0])) else em[1]
    st2 = putm(st, cin)
    seq = [move_verdict(w, put(st2, v), action)[0] for v in vals]
    want = [2 + m] * 4 + [2 + k] * 4
    if (seq if toward else seq[::-1]) != want:
        return None
    last = put(st2, vals[7] if toward else vals[0])
    if only_m(last):   # past `both` entity m is out of reach: the four values on k's side are m + k, m + k, k, k
        return None
    return {"family": "agent_entity_two", "sub": 0, "action": action, "states": [put(st2, v) for v in vals], "decider": k, "margin": MARGIN, "clamp": m}


def near_done_group(w, base, k, action, theta, sum64=False, others=()):
    """a free move lands the agent at near()'s threshold of entity k"""
    u = np.array([math.cos(theta), -math.sin(theta)])
    thr = float(near_threshold(w, k, w.E, sum64))
    if sum64 and thr == float(near_threshold(w, k, w.E)):
        return None
    e = base["ents_pos"][k][[0, 2]]
    land = e - u * thr
    st = start_for_landing(w, base, land, u, action)
    pt = (land[0], 0, land[1])
    if not isolated(w, st, pt, w.arad, MARGIN, self_idx=w.E):   # the move itself is free, k included
        return None
    if any(math.hypot(*(st["ents_pos"][o][[0, 2]] - land)) < float(near_threshold(w, o, w.E)) + MARGIN for o in others if o != k):
        return None   # no other goal entity decides
    ax = main_axis(u)

    def verdict(s):
        hit = move_verdict(w, s, action, sum64)
        return (hit, hit == (0, 0) and near(w, s, k, None, sum64, agent_pos=move_target(w, s, action)))
    return build_group("near_done", w, st, action, vary_agent(ax), st["agent_pos"][ax], verdict, sub=int(sum64), decider=k)


def pickup_reach_group(w, base, k, theta, sum64=False):
    """action 4 with entity k at the probe's threshold (1.5 r ahead, radius 1.2 r)"""
    u = np.array([math.cos(theta), -math.sin(theta)])
    thr = float(add(1.2 * w.arad, w.radius[k], sum64))
    if sum64 and thr == float(add(1.2 * w.arad, w.radius[k], False)):
        return None
    e = base["ents_pos"][k][[0, 2]]
    probe = e - u * thr
    st = copy_state(base)
    st["agent_dir"] = heading_of(u)
    st["agent_pos"] = np.array([probe[0], 0, probe[1]]) - dir_vec(st["agent_dir"]) * 1.5 * w.arad
    if w.static[k] or not isolated(w, st, (probe[0], 0, probe[1]), 1.2 * w.arad, MARGIN, skip_ents=(k,), self_idx=w.E):
        return None
    ax = main_axis(u)
    return build_group("pickup_reach", w, st, 4, vary_agent(ax), st["agent_pos"][ax], lambda s: pickup_verdict(w, s, sum64), sub=int(sum64), decider=k)


def pickup_two_group(w, base, k, m, theta):
    """action 4 with entity k at the probe's threshold and entity m > k, moved there, well inside its reach: with both in reach
    the lower index is picked up, on the other side of the flip entity m"""
    assert k < m
    u = np.array([math.cos(theta), -math.sin(theta)])
    thr = float(1.2 * w.arad + w.radius[k])
    probe = base["ents_pos"][k][[0, 2]] - u * thr
    st = copy_state(base)
    side = probe + rot(u, 1.7) * 0.25
    st["ents_pos"][m] = [side[0], 0, side[1]]
    st["agent_dir"] = heading_of(u)
    st["agent_pos"] = np.array([probe[0], 0, probe[1]]) - dir_vec(st["agent_dir"]) * 1.5 * w.arad
    if w.static[k] or w.static[m] or not isolated(w, st, (probe[0], 0, probe[1]), 1.2 * w.arad, MARGIN, skip_ents=(k, m), self_idx=w.E):
        return None
    ax = main_axis(u)
    g = build_group("pickup_two", w, st, 4, vary_agent(ax), st["agent_pos"][ax], lambda s: pickup_verdict(w, s), decider=k, clamp=m)
    if g is not None and {pickup_verdict(w, s) for s in g["states"]} == {2 + k, 2 + m}:
        return g
    return None


def pickup_wall_group(w, base, j, k, off):
    """a wall at the probe's threshold and entity k well inside its reach: the wall cancels the pickup on one side of the flip"""
    a, b, t, n0 = seg_frame(w, j)
    for n in (n0, -n0):
        foot = a + 0.5 * (b - a)
        probe = foot + n * (1.2 * w.arad)
        u = rot(-n, off)
        st = copy_state(base)
        back = probe + n * 0.25   # entity k: a quarter of a metre behind the probe's centre, away from the wall
        st["ents_pos"][k] = [back[0], 0, back[1]]
        st["agent_dir"] = heading_of(u)
        st["agent_pos"] = np.array([probe[0], 0, probe[1]]) - dir_vec(st["agent_dir"]) * 1.5 * w.arad
        pt = (probe[0], 0, probe[1])
        if w.static[k] or not isolated(w, st, pt, 1.2 * w.arad, MARGIN, skip_segs=(j,), skip_ents=(k,), self_idx=w.E):
            continue
        if not 0.02 < seg_proj(w, pt, j) < 0.98:
            continue
        ax = main_axis(n)
        g = build_group("pickup_wall", w, st, 4, vary_agent(ax), st["agent_pos"][ax], lambda s: pickup_verdict(w, s), decider=j, clamp=k)
        if g is not None and {pickup_verdict(w, s) for s in g["states"]} == {1, 2 + k}:
            return g
    return None


def _carried_base(w, base, k, agent_pos, d):
    st = copy_state(base)
    st["agent_pos"], st["agent_dir"], st["carrying"] = np.array(agent_pos, np.float64), d, k
    st["ents_pos"][k] = carry_pos(w, st["agent_pos"], d, k)
    st["ents_dir"][k] = d
    return st


def carry_wall_group(w, base, k, j, action, off):
    """entity k is carried; the carried entity's next position is radius(k) from the interior of wall j: a move (2) is refused as
    a whole, a turn (0 / 1) restores agent.dir"""
    a, b, t, n0 = seg_frame(w, j)
    rk = w.radius[k]
    for n in (n0, -n0):
        foot = a + 0.5 * (b - a)
        cland = foot + n * float(rk)
        u = rot(-n, off)
        d_new = heading_of(u)
        reach = (carry_pos(w, np.zeros(3), d_new, k))[[0, 2]]
        if action == 2:
            st = _carried_base(w, base, k, np.zeros(3), d_new)
            apos = np.array([cland[0], 0, cland[1]]) - np.array([reach[0], 0, reach[1]]) - move_target(w, st, 2)
            st = _carried_base(w, base, k, apos, d_new)
            nxt = move_target(w, st, 2)
            verdict = lambda s: move_verdict(w, s, 2)   # noqa: E731
            fam = "carry_move_wall"
        else:
            d0 = d_new - (w.turn_step if action == 0 else -w.turn_step) * (math.pi / 180)
            d_new = d0 + (w.turn_step if action == 0 else -w.turn_step) * (math.pi / 180)
            reach = (carry_pos(w, np.zeros(3), d_new, k))[[0, 2]]
            apos = np.array([cland[0], 0, cland[1]]) - np.array([reach[0], 0, reach[1]])
            st = _carried_base(w, base, k, apos, d0)
            nxt = st["agent_pos"]
            verdict = lambda s: turn_verdict(w, s, action)   # noqa: E731
            fam = "carry_turn_wall"
        cp = (cland[0], 0, cland[1])
        if not isolated(w, st, cp, rk, MARGIN, skip_segs=(j,), self_idx=k) or not 0.02 < seg_proj(w, cp, j) < 0.98:
            continue
        if action == 2 and not isolated(w, st, nxt, w.arad, MARGIN, self_idx=w.E):
            continue
        ax = main_axis(n)
        g = build_group(fam, w, st, action, vary_agent(ax), st["agent_pos"][ax], verdict, decider=j, clamp=k)
        if g is not None:
            return g
    return None


def carry_entity_group(w, base, k, m, action, theta, sum64=False):
    """entity k is carried; its next position is radius(k) + radius(m) from entity m, which is moved there"""
    rk = w.radius[k]
    u = np.array([math.cos(theta), -math.sin(theta)])
    d_new = heading_of(u)
    a0 = base["agent_pos"]
    if action == 2:
        st = _carried_base(w, base, k, a0, d_new)
        nxt = move_target(w, st, 2)
        fam, verdict = "carry_move_entity", (lambda s: move_verdict(w, s, 2, sum64))
    else:
        d0 = d_new - (w.turn_step if action == 0 else -w.turn_step) * (math.pi / 180)
        d_new = d0 + (w.turn_step if action == 0 else -w.turn_step) * (math.pi / 180)
        st = _carried_base(w, base, k, a0, d0)
        nxt = st["agent_pos"]
        fam, verdict = "carry_turn_entity", (lambda s: turn_verdict(w, s, action, sum64))
    cp = carry_pos(w, nxt, d_new, k, sum64)
    um = rot(u, 0.9)
    thr = float(add(rk, w.radius[m], sum64))
    if sum64 and thr == float(add(rk, w.radius[m], False)):
        return None
    st["ents_pos"][m] = [cp[0] + um[0] * thr, 0, cp[2] + um[1] * thr]
    if not isolated(w, st, cp, rk, MARGIN, skip_ents=(m,), self_idx=k):
        return None
    if action == 2 and not isolated(w, st, nxt, w.arad, MARGIN, self_idx=w.E):
        return None
    ax = main_axis(um)
    return build_group(fam, w, st, action, vary_agent(ax), st["agent_pos"][ax], verdict, sub=int(sum64), decider=m, clamp=k)


def entity_near_group(family, w, base, i, j, theta, action, carrying, y_i=0.0):
    """near(ent i, ent j) at its threshold in the state the step leaves: entity i's start coordinate varies.  putnext_rule: i is
    carried and action 5 drops it where it is; near_3d: i floats y_i above the floor, nobody carries it, and the 3-D norm decides."""
    u = np.array([math.cos(theta), -math.sin(theta)])
    thr = float(near_threshold(w, i, j))
    flat = math.sqrt(thr * thr - y_i * y_i)
    e = base["ents_pos"][j][[0, 2]]
    st = copy_state(base)
    st["ents_pos"][i] = [e[0] - u[0] * flat, y_i, e[1] - u[1] * flat]
    st["carrying"] = carrying

    def verdict(s):
        s = copy_state(s)
        if action == 5:
            s["ents_pos"][i, 1] = 0
        return near(w, s, i, j)
    ax = main_axis(u)
    return build_group(family, w, st, action, vary_ent(i, ax), st["ents_pos"][i, ax], verdict, decider=i, clamp=j)


def push_shove_group(w, base, b, theta):
    """SimToRealPush (simtorealpush.py:109-125): the nominal forward move - max_forward_step along dir_vec, whatever step length
    the step then draws - touches box b at arad + radius(b), and the box is free to give way"""
    u = np.array([math.cos(theta), -math.sin(theta)])
    thr = float(w.arad + w.radius[b])
    e = base["ents_pos"][b][[0, 2]]
    probe = e - u * thr
    st = copy_state(base)
    st["agent_dir"] = heading_of(u)
    st["agent_pos"] = np.array([probe[0], 0, probe[1]]) - dir_vec(st["agent_dir"]) * w.max_fwd
    if not isolated(w, st, (probe[0], 0, probe[1]), w.arad, MARGIN, skip_ents=(b,), self_idx=w.E):
        return None
    vec = st["ents_pos"][b] - (st["agent_pos"] + dir_vec(st["agent_dir"]) * w.max_fwd)
    if not isolated(w, st, st["ents_pos"][b] + vec, w.radius[b], MARGIN, self_idx=b):   # where the shove puts the box
        return None
    ax = main_axis(u)

    def verdict(s):
        nxt = s["agent_pos"] + dir_vec(s["agent_dir"]) * w.max_fwd
        return bool(np.linalg.norm(s["ents_pos"][b] - nxt) < w.arad + w.radius[b])
    return build_group("push_shove", w, st, 2, vary_agent(ax), st["agent_pos"][ax], verdict, decider=b)


def push_goal_group(w, base, goal_dist, theta, action):
    """SimToRealPush: the boxes stand goal_dist apart when the step ends (a turn: nothing moves); box 0's start coordinate varies"""
    u = np.array([math.cos(theta), -math.sin(theta)])
    e = base["ents_pos"][1][[0, 2]]
    st = copy_state(base)
    st["ents_pos"][0] = [e[0] - u[0] * goal_dist, 0, e[1] - u[1] * goal_dist]
    ax = main_axis(u)
    return build_group("push_goal", w, st, action, vary_ent(0, ax), st["ents_pos"][0, ax],
                       lambda s: bool(np.linalg.norm(s["ents_pos"][0] - s["ents_pos"][1]) < goal_dist), decider=0, clamp=1)


# --------------------------------------------------------------------------------------------- judging recorded outcomes
def decisions(start, out):
    """One row per case of what the step DECIDED, from recorded arrays (dicts of [n, ...] arrays): everything of the outcome
    but the values that merely follow the varied start coordinate"""
    n = len(out["reward"])
    # (a carried entity is put where the agent's pose says at the end of every step: its pose follows the varied coordinate)
    free = np.arange(start["ents_pos"].shape[1])[None, :] != start["carrying"][:, None]
    cols = [np.any(out["agent_pos"] != start["agent_pos"], axis=1), out["agent_dir"] != start["agent_dir"], out["carrying"], out["done"],
            out["reward"], out["hit"], out["alive"].reshape(n, -1).sum(axis=1),
            np.any(np.any(out["ents_pos"] != start["ents_pos"], axis=2) & free, axis=1), np.any((out["ents_dir"] != start["ents_dir"]) & free, axis=1)]
    return np.stack([np.asarray(c, np.float64) for c in cols], axis=1)


def straddles(dec):
    """[n_groups] bool from decisions() rows in group order: do the eight cases of a group differ in what was decided?"""
    d = dec.reshape(-1, GROUP, dec.shape[1])
    return np.any(d != d[:, :1], axis=(1, 2))


# --------------------------------------------------------------------------------------------------- reading the fixtures
# fixture task -> (env id of the batched library, oracle task, oracle task_args, task_args override for the library or None)
SPEC = {
    "Maze": ("MiniWorld-Maze-v0", "Maze", None, None),
    "MazeR9C9": ("MiniWorld-Maze-v0", "Maze", [9, 9, 3], [9, 9, 3]),
    "MazeR16C16": ("MiniWorld-Maze-v0", "Maze", [16, 16, 3], [16, 16, 3]),
    "YMaze": ("MiniWorld-YMaze-v0", "YMaze", [0, 0, 0, 0], None),
    "FourRooms": ("MiniWorld-FourRooms-v0", "FourRooms", None, None),
    "Hallway": ("MiniWorld-Hallway-v0", "Hallway", None, None),
    "TMazeTwoBoxDynamic": ("MiniWorld-TMazeTwoBoxDynamic-v0", "TMazeTwoBox", [0, 0, 0, 100], None),
    "PutNext": ("MiniWorld-PutNext-v0", "PutNext", None, None),
    "PickupObjs": ("MiniWorld-PickupObjs-v0", "PickupObjs", [12, 5, 0, 0], None),
    "RoomObjs": ("MiniWorld-RoomObjs-v0", "RoomObjs", [10, 0, 0, 0], None),
    "CollectHealth": ("MiniWorld-CollectHealth-v0", "CollectHealth", [16, 0, 0, 0], None),
    "Sign": ("MiniWorld-Sign-v0", "Sign", [10, 0, 0, 0], None),
    "SimToRealPush": ("MiniWorld-SimToRealPush-v0", "SimToRealPush", None, None),
}
# the families every task's fixture must hold surviving groups of ("/f64": the groups around the float64 sum's threshold)
EXPECT = {
    "Maze": ["wall_interior"], "MazeR9C9": ["wall_interior"], "MazeR16C16": ["wall_interior"], "YMaze": ["wall_interior"],
    "FourRooms": ["wall_interior", "wall_endpoint"],
    "Hallway": ["agent_entity", "near_done"], "TMazeTwoBoxDynamic": ["agent_entity", "near_done"],
    "PutNext": ["agent_entity", "agent_entity_two", "pickup_reach", "pickup_two", "pickup_wall", "carry_move_wall", "carry_move_entity", "carry_turn_wall",
                "carry_turn_entity", "putnext_rule", "near_3d"],
    "PickupObjs": ["agent_entity", "agent_entity/f64", "pickup_reach", "pickup_reach/f64", "pickup_two", "pickup_wall"],
    "RoomObjs": ["agent_entity", "agent_entity/f64", "carry_move_wall", "carry_move_entity", "carry_move_entity/f64", "carry_turn_wall", "carry_turn_entity", "carry_turn_entity/f64"],
    "CollectHealth": ["agent_entity", "agent_entity/f64"],
    "Sign": ["near_done", "near_done/f64"],
    "SimToRealPush": ["push_shove", "push_goal"],
}
START_KEYS = ("agent_pos", "agent_dir", "ents_pos", "ents_dir", "carrying", "step_count")
OUT_KEYS = START_KEYS + ("reward", "done", "alive", "health", "goal_pos", "num_picked")


def load(path):
    """{seed: {"start": {...}, "out": {...}, other arrays by name}} of one stepedge_<task>.npz, and its meta arrays"""
    z = np.load(path)
    worlds = {}
    for s in z["meta/seeds"]:
        p = "s%d/" % s
        w = {k[len(p):]: z[k] for k in z.files if k.startswith(p) and not k.startswith((p + "start/", p + "out/"))}
        w["start"] = {k: z[p + "start/" + k] for k in START_KEYS}
        w["out"] = {k: z[p + "out/" + k] for k in OUT_KEYS}
        worlds[int(s)] = w
    return worlds, {k[5:]: z[k] for k in z.files if k.startswith("meta/")}


def judge(w):
    """(per group: does the reference's recorded outcome straddle, the group's family id, its sub) of one world of load()"""
    dec = decisions(w["start"], {**w["out"], "hit": w["hit"]})
    return straddles(dec), w["family"][::GROUP], w["sub"][::GROUP]
