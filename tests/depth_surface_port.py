"""CPU restatement in numpy of what depth_filler's callers take from its grid, with the reference's own types:
get3DPos (include/visualizer/depth_filler.h:115-122), computeDistance(Zeros) (src/visualizer/depth_filler.cpp:170-180),
calcSurfNormals (:358-373), calcSurfArea (:377-389), getImgRho (depth_filler.h:246-280) and getImgRhoTriInterp (:203-244).

Every value is formed with explicit float32 / float64 types, one separately rounded operation at a time, as the reference's x86-64
build (SSE, no FMA) forms it.  The grids come from tests/depth_fill_port.py (or the device); the camera is the context's
(cam_model: pp and zf as float, zfm = (double)((zfx + zfy) / 2) formed in float).
"""
import numpy as np

F32, F64 = np.float32, np.float64
BILINEAR, TRIANGLE = 1, 2


def camera(ppx, ppy, zfx, zfy):
    """(ppx, ppy, zfm) as cam_model keeps them (cam_model.h:47-57)."""
    zfm = F64((F32(zfx) + F32(zfy)) / F32(2))
    return F32(ppx), F32(ppy), zfm


def points(rho, bw, bh, cam):
    """get3DPos(x, y) of every cell -> (gh, gw, 3) float64.  Img2Hom<float> gets ((float)x + 0.5) * bw — a double product — as a
    float and subtracts pp in float; then x / zfm in double and TooN's Vector / rho element-wise."""
    ppx, ppy, zfm = cam
    gh, gw = rho.shape
    ix = (np.arange(gw).astype(F32).astype(F64) + 0.5) * F64(bw)
    iy = (np.arange(gh).astype(F32).astype(F64) + 0.5) * F64(bh)
    hx = (ix.astype(F32) - ppx).astype(F64) / zfm   # float - float, then double / double
    hy = (iy.astype(F32) - ppy).astype(F64) / zfm
    r = np.asarray(rho, F64)
    with np.errstate(all="ignore"):
        return np.stack([hx[None, :] / r, hy[:, None] / r, 1.0 / r], axis=-1)


def dot(u, v):
    """TooN's Vector * Vector: result = 0, then += u[i] * v[i] in index order."""
    s = np.zeros(u.shape[:-1], F64)
    for i in range(3):
        s = s + u[..., i] * v[..., i]
    return s


def cross(u, v):
    """TooN's operator^."""
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def distance(P):
    """computeDistance(Zeros): dist = norm(P) = sqrt(P * P) per cell, and current_min_dist: 1e20 lowered by keep_min (never to a
    NaN).  dist >= 0, so the minimum does not depend on the order."""
    with np.errstate(all="ignore"):
        d = np.sqrt(dot(P, P))
    ok = ~np.isnan(d)
    m = min(1e20, float(d[ok].min())) if ok.any() else 1e20
    return d, F64(m)


def _quad(P):
    """The step of calcSurfNormals / calcSurfArea at every (x, y) of [0, gw-2] x [0, gh-2]: the two cross products."""
    P00, P01, P10, P11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]   # P01 = (x+1, y), P10 = (x, y+1)
    return cross(P01 - P00, P10 - P00), cross(P01 - P11, P10 - P11)


def step_normals(P):
    """(-unit(a) + unit(b)) / 2 with unit(v) = v * (1 / sqrt(v * v)) -> (gh-1, gw-1, 3)."""
    a, b = _quad(P)
    with np.errstate(all="ignore"):
        ua = a * (1.0 / np.sqrt(dot(a, a)))[..., None]
        ub = b * (1.0 / np.sqrt(dot(b, b)))[..., None]
        return (-ua + ub) / 2.0


def normals(P):
    """calcSurfNormals' result: the cell's own step for x <= gw-2, y <= gh-2, else the step of (x-1, y-1) (the raster loop runs x
    outer, y inner and writes (x, y) then (x+1, y+1)); NaN where the loop never writes."""
    gh, gw = P.shape[:2]
    out = np.full((gh, gw, 3), np.nan)
    if gw < 2 or gh < 2:
        return out
    n = step_normals(P)
    out[1:, gw - 1] = n[:, gw - 2]   # the last column and row: from (x-1, y-1)
    out[gh - 1, 1:] = n[gh - 2, :]
    out[:-1, :-1] = n
    return out


def raster_normals(P):
    """calcSurfNormals as the reference loops it, one cell at a time: the check of normals()' owner rule."""
    gh, gw = P.shape[:2]
    out = np.full((gh, gw, 3), np.nan)
    n = step_normals(P) if gw > 1 and gh > 1 else None
    for x in range(gw - 1):
        for y in range(gh - 1):
            out[y, x] = n[y, x]
            out[y + 1, x + 1] = out[y, x]
    return out


def areas(P):
    """calcSurfArea: (norm(a) + norm(b)) / 2 in double, stored as float (df_point::area); NaN in the last row and column."""
    gh, gw = P.shape[:2]
    out = np.full((gh, gw), np.nan, F32)
    if gw < 2 or gh < 2:
        return out
    a, b = _quad(P)
    with np.errstate(all="ignore"):
        out[:-1, :-1] = ((np.sqrt(dot(a, a)) + np.sqrt(dot(b, b))) / 2.0).astype(F32)
    return out


def surface(rho, bw, bh, cam):
    """-> dict(point, dist, min_dist, normal, area) of one grid."""
    P = points(rho, bw, bh, cam)
    d, m = distance(P)
    return dict(point=P, dist=d, min_dist=m, normal=normals(P), area=areas(P))


def terms(x, b, n):
    """getImgRho's index terms of integer coordinates x: float x_histo = x / (float)b - 0.5 (float division, double subtraction,
    back to float); f, c = floor / ceil clamped to [0, n-1] in double, then int; d = x_histo - f in float."""
    xh = (np.asarray(x).astype(F32) / F32(b)).astype(F64) - 0.5
    xh = xh.astype(F32)
    f = np.minimum(np.maximum(np.floor(xh).astype(F64), 0.0), n - 1.0).astype(np.int64)
    c = np.minimum(np.maximum(np.ceil(xh).astype(F64), 0.0), n - 1.0).astype(np.int64)
    return f, c, xh - f.astype(F32)


def image_at(rho, s_rho, bw, bh, px, py, mode):
    """getImgRho (mode 1) or getImgRhoTriInterp (mode 2) with s_rho at integer pixels (px, py) (broadcast) -> (rho, s_rho) float32."""
    gh, gw = rho.shape
    xf, xc, dx = terms(px, bw, gw)
    yf, yc, dy = terms(py, bh, gh)
    xf, xc, dx, yf, yc, dy = np.broadcast_arrays(xf, xc, dx, yf, yc, dy)
    g = np.asarray(rho, F64).astype(F32)
    s = np.asarray(s_rho, F64).astype(F32)
    r00, r10, r01, r11 = g[yf, xf], g[yf, xc], g[yc, xf], g[yc, xc]
    s00, s10, s01, s11 = s[yf, xf], s[yf, xc], s[yc, xf], s[yc, xc]
    one = F32(1)
    with np.errstate(all="ignore"):
        if mode == BILINEAR:
            r = r00 * (one - dx) * (one - dy) + r10 * dx * (one - dy) + r01 * (one - dx) * dy + r11 * dx * dy
            sr = s00 * (one - dx) * (one - dy) + s10 * dx * (one - dy) + s01 * (one - dx) * dy + s11 * dx * dy
        elif mode == TRIANGLE:
            up = dx > dy
            r = np.where(up, r00 + dx * (r10 - r00) + dy * (r11 - r10), r00 + dy * (r01 - r00) + dx * (r11 - r01))
            sr = np.where(up, s00 + dx * (s10 - s11) + dy * (s11 - s10), s00 + dy * (s01 - s11) + dx * (s11 - s01))
        else:
            raise ValueError(mode)
    return r.astype(F32), sr.astype(F32)


def image(rho, s_rho, w, h, bw, bh, mode):
    """The whole (h, w) depth image of one grid -> (rho, s_rho) float32."""
    return image_at(rho, s_rho, bw, bh, np.arange(w)[None, :], np.arange(h)[:, None], mode)
