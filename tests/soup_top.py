"""Brute-force software rendition of a captured render_top_view() stream (tests/golden/enttop_*.json, and the box tasks'
gltop_*.json): the map view of miniworld.py:1087-1158, orthographic, straight down, float64.

Independent cross-check of the HIP top view of the entity tasks.  Every polygon the reference handed to OpenGL (rooms, then the
static entities of the display list, then this frame's non-static entities - tests/soup_renderer.ent_stream_triangles - then the
agent's triangle with the normal that was current when it was drawn) is fanned into triangles; a triangle is front-facing from
above iff its winding runs counter-clockwise seen from +y (GL_CULL_FACE), and it is tested only against the samples inside its xz
footprint.  The highest front-facing hit wins (GL_LESS looking down), a tie goes to what was drawn first.  The render spec is the
obs path's: 8 samples per pixel, one shade per (pixel, polygon) with the attributes at the pixel centre (extrapolated), trilinear
REPEAT texturing with the LOD from the +1-pixel neighbours - here shifted ray ORIGINS, the direction being the same for all rays.
"""
import numpy as np

import soup_renderer as SR


def _origin_frame(misc, W, H):
    """window (wx, wy) -> world x = x0 + wx * sx, z = z1 - wy * sz (glOrtho + the fixed look-down modelview)"""
    o_l, o_r, o_b, o_t = misc["glOrtho"][:4]
    m = np.array(misc["glLoadMatrixf"]).reshape(4, 4).T   # column-major upload: eye = m @ world
    assert np.array_equal(m[:3, :3], [[1, 0, 0], [0, 0, -1], [0, 1, 0]]) and not m[:3, 3].any()
    return o_l, (o_r - o_l) / W, -o_b, (o_t - o_b) / H


def enttop_polys(g, mesh_arrays):
    """-> polygons in draw order (verts, vcol, texcs, tex, label in room / box / mesh / frame / agent) of an enttop_* stream"""
    polys = SR.ent_stream_triangles(g, mesh_arrays)
    labels = ["room"] * len(SR.polygons_from_stream({"polys": g["room_polys"], "room_tex": g["room_tex"]}))
    for it in g["static_items"] + g["dynamic_items"]:
        if it["type"] == "mesh":
            labels += ["mesh"] * len(mesh_arrays[it["mesh"]][0])
        else:
            n_per = {"GL_QUADS": 4, "GL_TRIANGLES": 3}[it["mode"]]
            box = len(it["verts"]) == 24 and not it["tex_on"]
            labels += ["box" if box else "frame"] * (len(it["verts"]) // n_per)
    assert len(labels) == len(polys)
    for p, lab in zip(polys, labels):
        p["label"] = lab
    polys.append(_agent(g, np.array(g["agent_tri"], float), np.array(g["agent_color"], float), np.array(g["agent_normal"], float)))
    return polys


def gltop_polys(g):
    """the same for a box task's gltop_* stream (rooms, boxes, then the agent as the last polygon)"""
    out = []
    polys = SR.polygons_from_stream(g)
    for i, p in enumerate(polys):
        if i == len(polys) - 1:
            out.append(_agent(g, p["verts"], p["color"], p["normal"]))
            continue
        n = len(p["verts"])
        col = _lit(g, np.broadcast_to(p["normal"], (n, 3)), np.broadcast_to(p["color"], (n, 3)))
        out.append({"verts": p["verts"], "vcol": col, "texcs": p["texcs"], "tex": p["tex"], "label": "room" if p["tex"] else "box"})
    return out


def _lit(g, normals, colors):
    Lp = np.array(g["lights"]["GL_POSITION"])
    assert Lp[3] == 0.0
    return SR._lit(normals, colors, SR._norm(Lp[:3]), np.array(g["lights"]["GL_AMBIENT"][:3]), np.array(g["lights"]["GL_DIFFUSE"][:3]))


def _agent(g, verts, color, normal):
    return {"verts": verts, "vcol": _lit(g, np.broadcast_to(normal, (3, 3)), np.broadcast_to(color, (3, 3))), "texcs": None, "tex": None,
            "label": "agent"}


def render_top(polys, misc, textures, W, H):
    """polys: enttop_polys / gltop_polys.  Returns (image (H, W, 3) uint8, mask (H, W) bool: some sample of the pixel sees an entity
    or the agent, cover: label -> (H, W) bool, the pixels some sample of which sees a polygon of that label)"""
    x0, sx, z1, sz = _origin_frame(misc, W, H)
    sky = np.array(misc["glClearColor"][:3])
    best_y = np.full((H, W, 8), -np.inf)   # rows from the BOTTOM of the frame (window y)
    best_p = np.full((H, W, 8), -1)
    for pi, p in enumerate(polys):
        v = np.asarray(p["verts"], float)
        for q in range(1, len(v) - 1):
            a, e1, e2 = v[0], v[q] - v[0], v[q + 1] - v[0]
            cr = e1[0] * e2[2] - e1[2] * e2[0]   # xz cross: < 0 <=> counter-clockwise seen from above <=> front-facing
            if not cr < 0:
                continue
            xs, zs = (a[0], a[0] + e1[0], a[0] + e2[0]), (a[2], a[2] + e1[2], a[2] + e2[2])
            i0, i1 = max(0, int(np.floor((min(xs) - x0) / sx)) - 1), min(W - 1, int(np.ceil((max(xs) - x0) / sx)) + 1)
            j0, j1 = max(0, int(np.floor((z1 - max(zs)) / sz)) - 1), min(H - 1, int(np.ceil((z1 - min(zs)) / sz)) + 1)
            if i0 > i1 or j0 > j1:
                continue
            J, I = np.mgrid[j0:j1 + 1, i0:i1 + 1]
            X = x0 + (I[..., None] + 0.5 + SR.SAMPLE_X[None, None]) * sx - a[0]
            Z = z1 - (J[..., None] + 0.5 + SR.SAMPLE_Y[None, None]) * sz - a[2]
            u = (X * e2[2] - Z * e2[0]) / cr
            w = (e1[0] * Z - e1[2] * X) / cr
            y = a[1] + u * e1[1] + w * e2[1]
            blk_y, blk_p = best_y[j0:j1 + 1, i0:i1 + 1], best_p[j0:j1 + 1, i0:i1 + 1]
            ok = (u >= -1e-12) & (w >= -1e-12) & (u + w <= 1 + 1e-12) & (y > blk_y)
            blk_y[ok] = y[ok]
            blk_p[ok] = pi
    cx = x0 + (np.arange(W) + 0.5) * sx
    cz = z1 - (np.arange(H) + 0.5) * sz
    CX, CZ = np.broadcast_to(cx[None], (H, W)).ravel(), np.broadcast_to(cz[:, None], (H, W)).ravel()
    bp = best_p.reshape(H * W, 8)
    acc = (bp == -1).sum(axis=1)[:, None] * sky[None]
    for pi in np.unique(bp[bp >= 0]):
        p = polys[pi]
        cnt = (bp == pi).sum(axis=1)
        idx = np.nonzero(cnt)[0]
        v = np.asarray(p["verts"], float)
        e1, e2 = v[1] - v[0], v[-1] - v[0]
        cr = e1[0] * e2[2] - e1[2] * e2[0]

        def bary(X, Z):
            X, Z = X - v[0, 0], Z - v[0, 2]
            return (X * e2[2] - Z * e2[0]) / cr, (e1[0] * Z - e1[2] * X) / cr

        def interp(A, ab):
            A = np.asarray(A, float)
            return A[0][None] + ab[0][:, None] * (A[1] - A[0])[None] + ab[1][:, None] * (A[-1] - A[0])[None]
        ab0 = bary(CX[idx], CZ[idx])
        col = interp(p["vcol"], ab0)
        if p["tex"] is not None:
            levels = textures[p["tex"]]
            h0, w0 = levels[0].shape[:2]
            st0, stx, sty = (interp(p["texcs"], ab0), interp(p["texcs"], bary(CX[idx] + sx, CZ[idx])),
                             interp(p["texcs"], bary(CX[idx], CZ[idx] - sz)))
            r1 = ((stx[:, 0] - st0[:, 0]) * w0) ** 2 + ((stx[:, 1] - st0[:, 1]) * h0) ** 2
            r2 = ((sty[:, 0] - st0[:, 0]) * w0) ** 2 + ((sty[:, 1] - st0[:, 1]) * h0) ** 2
            col = col * SR._trilinear(levels, st0[:, 0], st0[:, 1], np.maximum(r1, r2)) / 255.0
        acc[idx] += cnt[idx][:, None] * col
    img = np.floor(np.clip(acc / 8.0, 0, 1) * 255 + 0.5).astype(np.uint8).reshape(H, W, 3)[::-1]
    labels = np.array([p["label"] for p in polys] + ["sky"])
    lab = labels[best_p]   # best_p == -1 -> "sky"
    cover = {k: (lab == k).any(axis=2)[::-1] for k in ("room", "box", "mesh", "frame", "agent")}
    mask = cover["box"] | cover["mesh"] | cover["frame"] | cover["agent"]
    return img, mask, cover
