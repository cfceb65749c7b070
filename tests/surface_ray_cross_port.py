"""CPU restatement in numpy of REBVO's exhaustive cross-view ray check, SurfaceInt::checkDFRayCrossExaustive
(src/visualizer/surface_integrator.cpp:70-116), with the reference's own types and operation order: keyframe::transformTo
(include/mtracklib/keyframe.h:105-109), get3DPos (include/visualizer/depth_filler.h:115-122), computeDistance(Zeros)
(src/visualizer/depth_filler.cpp:170-182) and TooN's unit, norm, operator^ and sequential dot products.

A view is tests/surface_integrate_port.view's dict(rho, s_rho, Pose, Pos, K).  Every value is formed in float64 (get3DPos's Img2Hom part
in float32), one separately rounded operation at a time.  The arrays run over the hidder's rays (and over a block of target cells); the
arithmetic of one (cell, ray) test is written out as the reference has it.  What the reference recomputes in its inner loops but
depends on the hidder cell or the target cell alone is formed once, by the same operations.

The reference's quirk is kept: a ray's `dist` is norm(get3DPos(x, y)), not multiplied by the hidder's K, while the distance along the
ray it is compared with is in scaled units.  Comparisons with a NaN are false, as IEEE has them.  Visibility only falls: the loops'
early exits change no flag, and a cell that is hidden already needs no test.
"""
import numpy as np

from tests import depth_surface_port as dport
from tests.surface_integrate_port import camera, view  # noqa: F401  (the same views and camera)

F64 = np.float64
CHUNK = 16    # target cells per block of the (cells, rays) arrays


def transform_to(h, t, p):
    """h.transformTo(t, p) for points p (..., 3): t.Pose.T() * (h.Pose * p + h.Pos - t.Pos); a product is a dot product per row
    (of the transpose: per column), result = 0 and += in index order."""
    w = []
    with np.errstate(all="ignore"):
        for i in range(3):
            s = np.zeros(p.shape[:-1], F64)
            for j in range(3):
                s = s + h["Pose"][i, j] * p[..., j]
            w.append(s + h["Pos"][i] - t["Pos"][i])
        out = np.empty(p.shape, F64)
        for i in range(3):
            s = np.zeros(p.shape[:-1], F64)
            for j in range(3):
                s = s + t["Pose"][j, i] * w[j]
            out[..., i] = s
    return out


def rays(t, h, bw, bh, cam):
    """The hidder's rays in the target's frame -> (ray_orig (3,), ray_versor (G, 3), dist (G,))  (:89-91, depth_filler.cpp:175-177)."""
    P = dport.points(h["rho"], bw, bh, cam).reshape(-1, 3)
    ro = transform_to(h, t, np.zeros(3))
    with np.errstate(all="ignore"):
        rp = transform_to(h, t, P * h["K"])
        u = rp - ro
        v = u * (1.0 / np.sqrt(dport.dot(u, u)))[:, None]      # unit(v) = v * (1 / sqrt(v * v))
        dist = np.sqrt(dport.dot(P, P))                       # not scaled by K
    return ro, v, dist


def bubbles(t, bw, bh, cam):
    """buble_size of every target cell (:79, :95): util::norm(int, int) is sqrt of the int sum of squares."""
    with np.errstate(all="ignore"):
        norm_size = np.sqrt(F64(bw * bw + bh * bh)) / cam[2] * t["K"]
        return norm_size / t["rho"].reshape(-1)


def crossed_culled(d, bub, v, dist):
    """The same decisions as crossed()'s loop for tests that must stay quick on many pairs: a matrix product gives every (cell, ray)
    distance along the ray, a, and |d|^2 - a^2 estimates the squared distance to the ray (|v| = 1 to rounding).  The estimate is off
    by a few 1e-16 |d|^2 whatever order the product sums in; a pair is dropped only when the estimate is above the squared bubble by
    more than 1e-6 of it plus 1e-12 |d|^2.  Every other pair — those near the threshold, and every one with a NaN, an infinity or a
    |d|^2 outside [1e-100, 1e100] in it — goes through the reference's own operations, which alone decide a flag."""
    out = np.zeros(len(d), bool)
    with np.errstate(all="ignore"):
        dd = dport.dot(d, d)
        b2 = bub * bub
        for a0 in range(0, len(d), 256):
            sl = slice(a0, a0 + 256)
            a = d[sl] @ v.T
            est = dd[sl, None] - a * a
            far = est > (b2[sl] * (1.0 + 1e-6) + 1e-12 * dd[sl])[:, None]
            far &= ((dd[sl] > 1e-100) & (dd[sl] < 1e100))[:, None]
            i, j = np.nonzero(~far)
            d0, d1, d2 = d[sl][i, 0], d[sl][i, 1], d[sl][i, 2]
            vx, vy, vz = v[j, 0], v[j, 1], v[j, 2]
            cx, cy, cz = d1 * vz - d2 * vy, d2 * vx - d0 * vz, d0 * vy - d1 * vx
            near = np.sqrt(0.0 + cx * cx + cy * cy + cz * cz) < bub[sl][i]
            along = 0.0 + d0 * vx + d1 * vy + d2 * vz
            hit = near & (along > 0) & (along < dist[j])
            out[a0 + i[hit]] = True
    return out


def crossed(t, h, bw, bh, cam, cells=None, stats=None, cull=False):
    """checkDFRayCrossExaustive(t, h): which of the target's cells `cells` (flat indices; None: all) some ray of h crosses -> bool
    per cell.  stats (a dict) collects the branch populations: tests, inside the bubble, behind the origin, past the surface, hits.
    cull: decide through crossed_culled (the same flags, an order of magnitude fewer operations)."""
    G = t["rho"].size
    cells = np.arange(G) if cells is None else np.asarray(cells)
    ro, v, dist = rays(t, h, bw, bh, cam)
    point = (dport.points(t["rho"], bw, bh, cam).reshape(-1, 3) * t["K"])[cells]
    bub = bubbles(t, bw, bh, cam)[cells]
    out = np.zeros(len(cells), bool)
    vx, vy, vz = v[None, :, 0], v[None, :, 1], v[None, :, 2]
    with np.errstate(all="ignore"):
        d = point - ro
        if cull:
            return crossed_culled(d, bub, v, dist)
        for a in range(0, len(cells), CHUNK):
            d0, d1, d2 = (d[a:a + CHUNK, k, None] for k in range(3))
            cx, cy, cz = d1 * vz - d2 * vy, d2 * vx - d0 * vz, d0 * vy - d1 * vx       # operator^
            dist_p = np.sqrt(0.0 + cx * cx + cy * cy + cz * cz)
            near = dist_p < bub[a:a + CHUNK, None]
            i, j = np.nonzero(near)
            along = 0.0 + d0[i, 0] * v[j, 0] + d1[i, 0] * v[j, 1] + d2[i, 0] * v[j, 2]
            front, before = along > 0, along < dist[j]
            hit = front & before
            out[a + i[hit]] = True
            if stats is not None:
                for k, n in (("tests", near.size), ("near", len(i)), ("behind_origin", int((~front).sum())),
                             ("past_surface", int((front & ~before).sum())), ("hits", int(hit.sum()))):
                    stats[k] = stats.get(k, 0) + n
    return out


def all_pairs(views):
    return [(t, h) for t in range(len(views)) for h in range(len(views)) if t != h]


def ray_cross(views, pairs, bw, bh, cam, vis=None, stats=None, cull=False):
    """edgehip_surface_ray_cross: the ordered pairs (target, hidder) (None: every ordered pair), on top of `vis` (None: all visible).
    A pair that names an empty slot (None) is skipped.  -> list of (gh, gw) bool per view, None for an empty slot."""
    out = []
    for k, v in enumerate(views):
        if v is None:
            out.append(None)
        else:
            out.append(np.ones(v["rho"].shape, bool) if vis is None or vis[k] is None else np.array(vis[k], bool))
    for t, h in all_pairs(views) if pairs is None else pairs:
        assert t != h
        if views[t] is None or views[h] is None:
            continue
        flat = out[t].reshape(-1)
        cells = np.flatnonzero(flat)            # visibility only falls
        if len(cells):
            flat[cells[crossed(views[t], views[h], bw, bh, cam, cells, stats, cull)]] = False
    return out
