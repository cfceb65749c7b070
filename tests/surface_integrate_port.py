"""CPU restatement in numpy of REBVO's cross-view surface integration (src/visualizer/surface_integrator.cpp) with the reference's
own types: analizeSpaceSize (:32-68), OcGrid's geometry (:120-132, surface_integrator.h:66-69), fillKFList's sample walk (:167-229,
getImg3DPos: include/visualizer/depth_filler.h:133-163) and rayCutSurface (:235-266).

The reference keeps a list of cells per voxel and lets ray steps clear the visibility of other views' cells found there.  Visibility
only falls, so the order does not matter: cell c of view A ends hidden iff some voxel holds both a fill sample of c and a ray step of a
casting view B != A.  Here the ray steps of every casting view are collected as (voxel, view) pairs and every sample is looked up.

A view is a dict(rho, s_rho, Pose, Pos, K): (gh, gw) float64 grids, Pose 3x3, Pos 3, scale K; Local2WorldScaled(p) = Pose * p * K + Pos
(include/mtracklib/keyframe.h:101-103).  Every value is formed with explicit float32 / float64 types, one separately rounded operation
at a time.  The departures of include/edgehip.h's section are followed and counted: out-of-box samples and steps are dropped, a cell
with a non-finite or non-positive rho / K has no samples, a ray whose step count is no int takes no steps.
"""
import numpy as np

from tests import depth_surface_port as dport

F32, F64 = np.float32, np.float64
camera = dport.camera


def view(rho, s_rho, Pose=np.eye(3), Pos=(0, 0, 0), K=1.0):
    return dict(rho=np.asarray(rho, F64), s_rho=np.asarray(s_rho, F64), Pose=np.asarray(Pose, F64).reshape(3, 3),
                Pos=np.asarray(Pos, F64).reshape(3), K=F64(K))


def l2w(v, P):
    """Local2WorldScaled of points P (..., 3): TooN's Matrix * Vector is a dot product per row (0, += in index order), * K, + Pos."""
    out = np.empty(P.shape, F64)
    with np.errstate(all="ignore"):
        for a in range(3):
            s = np.zeros(P.shape[:-1], F64)
            for b in range(3):
                s = s + v["Pose"][a, b] * P[..., b]
            out[..., a] = s * v["K"] + v["Pos"][a]
    return out


def space(views, bw, bh, cam):
    """analizeSpaceSize -> (origin, size).  keep_min / keep_max never take a NaN; the maxima start at 1e-20."""
    mn, mx = np.full(3, 1e20), np.full(3, 1e-20)
    for v in views:
        if v is None:
            continue
        W = l2w(v, dport.points(v["rho"], bw, bh, cam)).reshape(-1, 3)
        for i in range(3):
            ok = ~np.isnan(W[:, i])
            if ok.any():
                mn[i] = min(mn[i], W[ok, i].min())
                mx[i] = max(mx[i], W[ok, i].max())
    return mn, mx - mn


def box(origin, size, n):
    """OcGrid's geometry: block = size / n per axis, min_block = the smallest."""
    n = np.asarray(n, np.int64).reshape(3)
    origin, size = np.asarray(origin, F64).reshape(3), np.asarray(size, F64).reshape(3)
    block = size / n.astype(F64)
    return dict(origin=origin, block=block, min_block=F64(block.min()), n=n)


def voxel(p, b):
    """wordl2Index of points p (m, 3) -> (inside, linear index): the quotient per axis, truncated; negative, non-finite or >= n is
    outside."""
    with np.errstate(all="ignore"):
        q = (p - b["origin"]) / b["block"]
        ok = (q >= 0.0) & (q < b["n"].astype(F64))
    inside = ok.all(-1)
    u = np.where(ok, q, 0.0).astype(np.int64)
    return inside, (u[:, 2] * b["n"][1] + u[:, 1]) * b["n"][0] + u[:, 0], q


def ray_voxels(v, b, bw, bh, cam):
    """rayCutSurface of one view -> (sorted unique voxel indices its steps fall in, steps outside the box)."""
    ro = l2w(v, np.zeros((1, 3)))
    with np.errstate(all="ignore"):
        rp = l2w(v, dport.points(v["rho"] + v["s_rho"], bw, bh, cam).reshape(-1, 3))
        d = rp - ro
        nrm = np.sqrt(dport.dot(d, d))
        step = d * (1.0 / nrm)[:, None] * b["min_block"]
        t = nrm / b["min_block"]
    steps = np.where(np.isfinite(t) & (t < 2147483648.0), np.trunc(np.where(np.isfinite(t), t, 0.0)), 0.0).astype(np.int64)
    pos = np.repeat(ro, len(d), 0)
    live = np.arange(len(d))
    found, outside, k = [], 0, 0
    while True:
        live = live[steps[live] > k]
        if not len(live):
            break
        inside, idx, q = voxel(pos[live], b)
        found.append(idx[inside])
        outside += int((~inside).sum())
        # a ray past the box on an axis in its own direction never comes back (adding one constant is monotone): its later steps are
        # all outside and are counted here at once
        s = step[live]
        gone = (np.isnan(q) | ((q >= b["n"]) & ~(s < 0)) | ((q < 0) & ~(s > 0))).any(-1) & ~inside
        outside += int((steps[live[gone]] - k - 1).sum())
        live = live[~gone]
        with np.errstate(all="ignore"):
            pos[live] = pos[live] + step[live]
        k += 1
    return (np.unique(np.concatenate(found)) if found else np.zeros(0, np.int64)), outside


def mark(views, cast, b, bw, bh, cam):
    """The plane: sorted voxel indices with the smallest and largest casting view id of each -> (idx, lo, hi, steps outside)."""
    idx, ids, outside = [], [], 0
    for k in cast:
        if views[k] is None:
            continue
        u, o = ray_voxels(views[k], b, bw, bh, cam)
        idx.append(u)
        ids.append(np.full(len(u), k, np.int64))
        outside += o
    if not idx or not sum(len(u) for u in idx):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), outside
    idx, ids = np.concatenate(idx), np.concatenate(ids)
    order = np.lexsort((ids, idx))
    idx, ids = idx[order], ids[order]
    first = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
    last = np.r_[first[1:] - 1, len(idx) - 1]
    return idx[first], ids[first], ids[last], outside


def crossed_by_other(plane, vox, me):
    """For voxel indices vox: do they hold a casting view other than `me`?"""
    pidx, lo, hi, _ = plane
    if not len(pidx):
        return np.zeros(len(vox), bool)
    j = np.minimum(np.searchsorted(pidx, vox), len(pidx) - 1)
    return (pidx[j] == vox) & ((lo[j] != me) | (hi[j] != me))


def hidden_cells(v, me, plane, b, bw, bh, cam):
    """fillKFList's walk over every cell of one view, looked up in the plane -> (hidden (gh, gw) bool, samples, samples outside).
    All cells advance together: float accumulators i_y, i_x with double increments, each cell with its own step and bounds."""
    ppx, ppy, zfm = cam
    gh, gw = v["rho"].shape
    G = gh * gw
    rho = v["rho"]
    g32 = rho.astype(F32)
    gy, gx = np.divmod(np.arange(G), gw)
    with np.errstate(all="ignore"):
        min_rho = rho.reshape(-1) / v["K"]
        rect_x, rect_y = F64(bw) / zfm / min_rho, F64(bh) / zfm / min_rho
        qx, qy = rect_x / b["min_block"], rect_y / b["min_block"]
        step_x = F64(bw) / np.where(qx < 1.0, 1.0, qx)   # std::max(q, 1.0)
        step_y = F64(bh) / np.where(qy < 1.0, 1.0, qy)
    walk = (min_rho > 0) & np.isfinite(min_rho) & (step_x > 0) & (step_y > 0)
    x0, x1 = (gx * bw).astype(F32), ((gx + 1) * bw).astype(F32)
    y1 = ((gy + 1) * bh).astype(F32)
    hidden = np.zeros(G, bool)
    samples = outside = 0
    iy = (gy * bh).astype(F32)
    rows = np.flatnonzero(walk)
    while True:
        rows = rows[iy[rows] < y1[rows]]
        if not len(rows):
            break
        yf, yc, dy = dport.terms(iy, bh, gh)
        ix = x0.copy()
        cols = rows
        stuck = np.zeros(G, bool)
        while True:
            cols = cols[ix[cols] < x1[cols]]
            if not len(cols):
                break
            xf, xc, dx = dport.terms(ix[cols], bw, gw)
            f, c, d = yf[cols], yc[cols], dy[cols]
            r00, r10, r01, r11 = g32[f, xf], g32[f, xc], g32[c, xf], g32[c, xc]
            one = F32(1)
            with np.errstate(all="ignore"):
                r = r00 * (one - dx) * (one - d) + r10 * dx * (one - d) + r01 * (one - dx) * d + r11 * dx * d   # depth_filler.h:156
                hx, hy = (ix[cols] - ppx).astype(F64), (iy[cols] - ppy).astype(F64)
                r = r.astype(F64)
                P = np.stack([hx / zfm / r, hy / zfm / r, 1.0 / r], -1)
            inside, idx, _ = voxel(l2w(v, P), b)
            samples += len(cols)
            outside += int((~inside).sum())
            hit = np.zeros(len(cols), bool)
            hit[inside] = crossed_by_other(plane, idx[inside], me)
            hidden[cols[hit]] = True
            nx = (ix[cols].astype(F64) + step_x[cols]).astype(F32)   # float i_x += double step
            adv = nx > ix[cols]
            stuck[cols[~adv]] = True        # an accumulator that no longer advances: the walk of that cell ends
            ix[cols] = nx
            cols = cols[adv]
        rows = rows[~stuck[rows]]
        ny = (iy[rows].astype(F64) + step_y[rows]).astype(F32)
        adv = ny > iy[rows]
        iy[rows] = ny
        rows = rows[adv]
    return hidden.reshape(gh, gw), samples, outside


def integrate(views, origin, size, n, bw, bh, cam, cast=None, vis=None):
    """edgehip_surface_integrate: rays of `cast` (None: all stored views), then every stored view's test.  vis: the visibilities to
    keep falling from (accumulate), None = all visible.  -> (list of (gh, gw) bool per view, None for an empty slot; dict of counts).
    Unlike the walk of the reference the test does not stop at a cell's first hit, so `samples` counts every sample."""
    b = box(origin, size, n)
    cast = [k for k in (range(len(views)) if cast is None else cast) if views[k] is not None]
    plane = mark(views, cast, b, bw, bh, cam)
    out, stats = [], dict(ray_steps_outside=plane[3], samples=0, samples_outside=0, voxels_marked=len(plane[0]))
    for k, v in enumerate(views):
        if v is None:
            out.append(None)
            continue
        hidden, s, o = hidden_cells(v, k, plane, b, bw, bh, cam)
        stats["samples"] += s
        stats["samples_outside"] += o
        prev = np.ones(hidden.shape, bool) if vis is None or vis[k] is None else np.asarray(vis[k], bool)
        out.append(prev & ~hidden)
    return out, stats
