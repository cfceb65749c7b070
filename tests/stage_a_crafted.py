"""Crafted images, parameter sets and a plain numpy restatement of stage A's decisions (edge_finder.cpp:67-365).

The restatement is not a third implementation to trust: the CPU test holds it to the compiled reference on every case, and then
uses it for two things the reference cannot give — WHICH gate decided each pixel (the population conditions), and what a one-line
mistake would change (DEFECTS).  It is fed the reference's own dx / dy / DoG planes; the scale space is not restated here.

    crafted_images(w, h)                      name -> (h, w, 3) uint8, r = g = b
    restate_build_mask(dx, dy, dog, p, tresh) gates, mask, KeyLines of build_mask
    restate_stage_a(planes, p, tresh, lkl)    UpdateThresh + build_mask + join_edges + reEstimateThresh
    param_sets(name)                          the parameter sets of one group, found by search where a value has to sit exactly on a threshold
    ref_case(over, image)                     the reference's result, computed once per (parameters, image) and shared
"""
import functools

import numpy as np

from oracle import oracle

W, H = 104, 50          # multiple of 4, not of 16 / 64, spans the 63 / 64 lane seam; height no multiple of 4 or 12
MAX_IMG = 765           # max_img_value = 255 * 3 (rebvo.cpp:300)
KL = oracle.KEYLINE_DTYPE
STAGE_A_FIELDS = ["p_inx", "m_m", "u_m", "n_m", "c_p", "rho", "s_rho", "rho_nr", "s_rho_nr", "rho0", "s_rho0",
                  "p_m", "p_m_0", "m_id", "m_id_f", "m_id_kf", "m_num", "p_id", "n_id", "net_id"]
F = np.float32

# gate codes of restate_build_mask()["gate"]
UNSCANNED, G_GRAD, G_SIGN, G_POS, G_DOGGRAD, KEYLINE = 0, 1, 2, 3, 4, 5
GATE_NAMES = {G_GRAD: "gradient", G_SIGN: "sign balance", G_POS: "position", G_DOGGRAD: "DoG gradient"}

BASE = dict(auto_gain=0.0, detector_thresh=0.002, min_thresh=1e-4)

DEFECTS = {
    "grad_gate_le": "gradient gate rejects n2g <= thr_g",
    "sign_gate_ge": "sign gate rejects |pn| >= 25 * PosNegThresh",
    "dog_zero_positive": "DoG >= 0 counted positive",
    "pos_gate_ge": "position gate rejects |xs| >= 0.5 or |ys| >= 0.5",
    "dog_grad_gate_le": "DoG-gradient gate rejects n2_m <= thr_d",
    "fit_float": "plane-fit sums in float",
    "join_first_writer": "p_id keeps its first writer",
    "round_no_half": "int(c) without the 0.5",
    "next_ty_ge": "NextPoint: ty >= 0 picks the upper half",
    "next_tx_ge": "NextPoint: tx >= 0 picks the right quadrant of the upper half",
    "next_tx_gt_lower": "NextPoint: tx > 0 picks the right quadrant of the lower half",
    "cut_late": "kl_max cut one KeyLine late",
    "tail_not_cleared": "mask tail not cleared after the cut",
    "clamp_before_gain": "clamp applied before the gain step",
    "gain_at_zero": "gain step (and clamp) taken at gain == 0",
}


# ---- images ---------------------------------------------------------------------------------------------------------------------
def _rgb(a):
    return np.ascontiguousarray(np.repeat(np.asarray(a).astype(np.uint8)[:, :, None], 3, axis=2))


IMAGE_NAMES = (
    ["ramp_h", "ramp_v", "ramp_d", "checker4", "dot3", "cross", "step3", "blocks_sat", "y_junction", "x_crossing", "noise8"]
    + [f"vstep_{pol}" for pol in ("up", "down")] + [f"hstep_{pol}" for pol in ("up", "down")]
    + [f"{d}_{pol}" for d in ("diag", "anti") for pol in ("up", "down")]
    + [f"vstep_c{c}" for c in (2, 3, 4, W - 4, W - 3, W - 2)]
    + [f"hstep_r{r}" for r in (2, 3, 4, 12, 13, H - 4, H - 3, H - 2)]
    + ["diag_corner_tl", "diag_corner_br", "anti_corner_tr", "anti_corner_bl"]
    + [f"stripes{n}_{o}" for n in (1, 2, 3) for o in ("v", "h")]
)


def crafted_images(w=W, h=H):
    """Named frames.  A step `*_cN` / `*_rN` has its first bright column / row at N, so its zero crossing lies between N - 1 and N and
    its KeyLines fall on one of the two: N in 2..4 and dim - 4..dim - 2 covers the first and last scanned positions (2, dim - 3) and
    the unscanned border next to them; rows 12 / 13 are the band seam, row 4 the tick seam."""
    y, x = np.mgrid[0:h, 0:w]
    lo, hi = 60, 190
    im = {}
    im["ramp_h"] = x * 255 // (w - 1)
    im["ramp_v"] = y * 255 // (h - 1)
    im["ramp_d"] = (x + y) * 255 // (w + h - 2)
    im["checker4"] = np.where(((x // 4) + (y // 4)) % 2 == 0, lo, hi)
    im["dot3"] = np.where((abs(x - w // 2) <= 1) & (abs(y - h // 2) <= 1), hi, lo)
    im["cross"] = np.where((abs(x - w // 2) <= 1) | (abs(y - h // 2) <= 1), hi, lo)
    im["step3"] = np.where(x < w // 3, 40, np.where(x < 2 * w // 3, 120, 230))
    im["blocks_sat"] = np.where(((x // 13) + (y // 7)) % 2 == 0, 0, 255)
    cx, cy = w // 2, h // 2                                                  # three sectors meeting in one point
    im["y_junction"] = np.where((y >= cy), 125, np.where(x - cx < -(cy - y) // 2, 50, np.where(x - cx > (cy - y) // 2, 200, 50)))
    im["x_crossing"] = np.where(((x - cx) - (y - cy)) * ((x - cx) + (y - cy)) > 0, hi, lo)
    im["noise8"] = np.random.default_rng(11).integers(0, 8, (h, w)) * 32
    for pol, (a, b) in (("up", (lo, hi)), ("down", (hi, lo))):
        im[f"vstep_{pol}"] = np.where(x < w // 2, a, b)
        im[f"hstep_{pol}"] = np.where(y < h // 2, a, b)
        im[f"diag_{pol}"] = np.where(x - y < (w - h) // 2, a, b)
        im[f"anti_{pol}"] = np.where(x + y < (w + h) // 2, a, b)
    for c in (2, 3, 4, w - 4, w - 3, w - 2):
        im[f"vstep_c{c}"] = np.where(x < c, lo, hi)
    for r in (2, 3, 4, 12, 13, h - 4, h - 3, h - 2):
        im[f"hstep_r{r}"] = np.where(y < r, lo, hi)
    im["diag_corner_tl"] = np.where(x - y < 0, lo, hi)                       # through (0, 0): rows and columns 2, 3
    im["diag_corner_br"] = np.where(x - y < w - h, lo, hi)                   # through (w - 1, h - 1)
    im["anti_corner_tr"] = np.where(x + y < w - 1, lo, hi)                   # through (w - 1, 0)
    im["anti_corner_bl"] = np.where(x + y < h - 1, lo, hi)                   # through (0, h - 1)
    for n in (1, 2, 3):
        im[f"stripes{n}_v"] = np.where((x // n) % 2 == 0, lo, hi)
        im[f"stripes{n}_h"] = np.where((y // n) % 2 == 0, lo, hi)
    assert sorted(im) == sorted(IMAGE_NAMES)
    return {k: _rgb(im[k]) for k in IMAGE_NAMES}


def blank(w=W, h=H, v=77):
    return np.full((h, w, 3), v, np.uint8)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _pinv(ws):
    """PInv = Matrix3x3Inv(Phi^T Phi) * Phi^T as edge_finder.cpp:89-98 evaluates it; for the 5x5 window its rows are
    {-2u, -u, 0, u, 2u} (u = fl(1/50)) along x, along y, and the constant 2u."""
    i, j = np.mgrid[-ws:ws + 1, -ws:ws + 1]
    phi = np.stack([j.ravel(), i.ravel(), np.ones(j.size)], 1).astype(np.float64)
    a = phi.T @ phi                                                          # small integers: exact
    det = a[0, 0] * a[1, 1] * a[2, 2]
    b = np.diag([a[2, 2] * a[1, 1] / det, a[2, 2] * a[0, 0] / det, a[1, 1] * a[0, 0] / det])
    return np.stack([b[r, 0] * phi[:, 0] + b[r, 1] * phi[:, 1] + b[r, 2] * phi[:, 2] for r in range(3)])


def thr_g_of(tresh):
    g = F(F(tresh) * F(MAX_IMG))
    return F(g * g)


def thr_d_of(tresh, dog_thresh):
    g = F(F(F(tresh) * F(MAX_IMG)) * F(dog_thresh))
    return F(g * g)


def restate_build_mask(dx, dy, dog, p, tresh, defect=None):
    """build_mask on given planes.  -> dict(gate, mask, kl, kn, uncut, and the per-pixel quantities n2g, pn, xs, ys, n2m)."""
    h, w = dog.shape
    ws = int(p.plane_fit_size)
    nn = (2 * ws + 1) ** 2
    ys_, xs_ = slice(ws, h - ws), slice(ws, w - ws)
    sh = (h - 2 * ws, w - 2 * ws)
    with np.errstate(all="ignore"):
        gx, gy = dx[ys_, xs_], dy[ys_, xs_]
        n2g = F(gx * gx) + F(gy * gy)
        thr_g = thr_g_of(tresh)
        rej_g = n2g <= thr_g if defect == "grad_gate_le" else n2g < thr_g
        win = [dog[ws + i:h - ws + i, ws + j:w - ws + j] for i in range(-ws, ws + 1) for j in range(-ws, ws + 1)]
        pos = sum(((v >= 0) if defect == "dog_zero_positive" else (v > 0)).astype(np.int32) for v in win)
        pn = 2 * pos - nn
        pn_thr = F(F(nn) * F(p.pos_neg_thresh))
        apn = np.abs(pn).astype(np.float64)
        rej_s = apn >= np.float64(pn_thr) if defect == "sign_gate_ge" else apn > np.float64(pn_thr)
        pinv = _pinv(ws)
        acc = np.float32 if defect == "fit_float" else np.float64
        th = [np.zeros(sh, acc) for _ in range(3)]
        for r in range(3):
            for k in range(nn):                                              # sums from +0, in window order
                th[r] = th[r] + acc(pinv[r, k]) * win[k].astype(acc)
        t0, t1, t2 = (t.astype(np.float64) for t in th)
        den = t0 * t0 + t1 * t1
        xs = (-t0 * t2 / den).astype(F)
        ys = (-t1 * t2 / den).astype(F)
        if defect == "pos_gate_ge":
            rej_p = (np.abs(xs) >= 0.5) | (np.abs(ys) >= 0.5)
        else:
            rej_p = (np.abs(xs) > 0.5) | (np.abs(ys) > 0.5)                  # a NaN offset passes
        mx, my = t0.astype(F), t1.astype(F)
        n2m = F(mx * mx) + F(my * my)
        thr_d = thr_d_of(tresh, p.dog_thresh)
        rej_d = n2m <= thr_d if defect == "dog_grad_gate_le" else n2m < thr_d
    gate_in = np.select([rej_g, rej_s, rej_p, rej_d], [G_GRAD, G_SIGN, G_POS, G_DOGGRAD], KEYLINE).astype(np.int8)
    gate = np.zeros((h, w), np.int8)
    gate[ys_, xs_] = gate_in
    yy, xx = np.nonzero(gate == KEYLINE)                                     # raster order
    uncut = len(yy)
    kl_max = int(p.max_points) + (1 if defect == "cut_late" else 0)
    kn = min(uncut, kl_max)
    mask = np.full((h, w), -1, np.int32)
    keep = uncut if defect == "tail_not_cleared" else kn
    mask[yy[:keep], xx[:keep]] = np.arange(keep, dtype=np.int32)
    yy, xx = yy[:kn], xx[:kn]
    kl = np.zeros(kn, KL)
    sel = (yy - ws, xx - ws)
    with np.errstate(all="ignore"):
        kl["p_inx"] = yy * w + xx
        kl["m_m"][:, 0], kl["m_m"][:, 1] = mx[sel], my[sel]
        kl["n_m"] = np.sqrt(n2m[sel])
        kl["u_m"] = kl["m_m"] / kl["n_m"][:, None]
        kl["c_p"][:, 0] = xx.astype(F) + xs[sel]
        kl["c_p"][:, 1] = yy.astype(F) + ys[sel]
        kl["p_m"][:, 0] = kl["c_p"][:, 0] - F(p.ppx)                          # cam_model keeps pp as float (cam_model.h:45)
        kl["p_m"][:, 1] = kl["c_p"][:, 1] - F(p.ppy)
    kl["p_m_0"] = kl["p_m"]
    for f in ("rho", "rho0", "rho_nr"):
        kl[f] = 1.0                                                          # RhoInit
    for f in ("s_rho", "s_rho0", "s_rho_nr"):
        kl[f] = 20.0                                                         # RHO_MAX
    for f in ("n_id", "p_id", "net_id", "m_id", "m_id_f", "m_id_kf"):
        kl[f] = -1
    full = lambda a: np.pad(a, ws)
    return dict(gate=gate, mask=mask, kl=kl, kn=kn, uncut=uncut, n2g=full(n2g), pn=full(pn), xs=full(xs), ys=full(ys), n2m=full(n2m),
                thr_g=thr_g, thr_d=thr_d, pn_thr=pn_thr, pos=full(pos), win_has_zero=full(sum((v == 0).astype(np.int32) for v in win) > 0))


def restate_join(kl, mask, defect=None):
    """join_edges in place: raster order, the last writer of p_id wins.  -> (quadrant, probe) per KeyLine; quadrants are numbered
    in the order NextPoint lists them (0: ty>0,tx>0; 1: ty>0,tx<=0; 2: ty<=0,tx<0; 3: ty<=0,tx>=0), probe -1 = no successor."""
    kn = len(kl)
    half = 0.0 if defect == "round_no_half" else 0.5
    x = (kl["c_p"][:, 0].astype(np.float64) + half).astype(np.int64)
    y = (kl["c_p"][:, 1].astype(np.float64) + half).astype(np.int64)
    tx, ty = -kl["m_m"][:, 1], kl["m_m"][:, 0]
    up = ty >= 0 if defect == "next_ty_ge" else ty > 0
    right_up = tx >= 0 if defect == "next_tx_ge" else tx > 0
    left_lo = tx <= 0 if defect == "next_tx_gt_lower" else tx < 0
    quad = np.where(up, np.where(right_up, 0, 1), np.where(left_lo, 2, 3))
    sx = np.array([1, -1, -1, 1])[quad]
    sy = np.array([1, 1, -1, -1])[quad]
    succ = np.full(kn, -1, np.int64)
    probe = np.full(kn, -1, np.int64)
    for n, (ox, oy) in enumerate(((1, 0), (0, 1), (1, 1))):
        v = mask[y + oy * sy, x + ox * sx]
        take = (succ < 0) & (v >= 0)
        succ[take], probe[take] = v[take], n
    has = np.nonzero(succ >= 0)[0]
    kl["n_id"][has] = succ[has]
    order = has[::-1] if defect == "join_first_writer" else has
    for i in order:                                                          # sequential on purpose: this IS the statement
        if succ[i] < kn:                                                     # (an id past the cut exists only under tail_not_cleared)
            kl["p_id"][succ[i]] = i
    return quad, probe


def restate_update_thresh(p, tresh, lkl, defect=None):
    con = lambda v: p.max_thresh if v > p.max_thresh else (p.min_thresh if v < p.min_thresh else v)   # util::Constrain
    if p.auto_gain > 0 or defect == "gain_at_zero":
        if defect == "clamp_before_gain":
            return con(tresh) - p.auto_gain * float(p.reference_points - lkl)
        return con(tresh - p.auto_gain * float(p.reference_points - lkl))
    return tresh


def restate_retuned(kl, knum, n):
    """reEstimateThresh (edge_finder.cpp:373-405) in float, with its loop as written: bin 0 is never counted.  With
    max_dog == min_dog the bin index is (int)NaN, which is undefined — but the index is clamped into the histogram whatever it
    is, and the result is max_dog - i * 0 / n = max_dog for every i, so the value does not hang on the conversion."""
    nm = kl["n_m"]
    mx, mn = nm.max(), nm.min()
    if mx == mn:
        return F(mx)
    with np.errstate(all="ignore"):
        i = (F(n) * (mx - nm) / (mx - mn)).astype(np.int64)
    histo = np.bincount(np.clip(i, 0, n - 1), minlength=n + 1)
    i, a = 0, 0
    while i < n and a < knum:
        i += 1
        a += histo[i] if i < n else 0
    return F(mx - F(i) * (mx - mn) / F(n))


def restate_stage_a(planes, p, tresh, lkl, defect=None):
    """detect() + reEstimateThresh on the reference's planes.  -> dict(build_mask's fields + tresh, lkl, retuned, quad, probe)."""
    tresh = restate_update_thresh(p, tresh, lkl, defect)
    r = restate_build_mask(planes["dx"], planes["dy"], planes["dog"], p, tresh, defect)
    r["quad"], r["probe"] = restate_join(r["kl"], r["mask"], defect)
    r["tresh"], r["lkl"] = tresh, r["kn"]
    r["retuned"] = restate_retuned(r["kl"], p.track_points, p.qcut_nbins) if r["kn"] > 0 else None
    return r


# ---- the reference, once per (parameters, image) -----------------------------------------------------------------------------------
def _key(over):
    return tuple(sorted(over.items()))


@functools.lru_cache(maxsize=None)
def images():
    return crafted_images(W, H)


def run_oracle(kind, over, frames, tresh=None, lkl=0):
    """Stage A of `frames` one after the other -> list of dict(planes, mask, kl, kn, tresh, lkl, retuned, tresh_in, lkl_in)."""
    orc = oracle.Oracle(kind, oracle.euroc_params(W, H, **over), nslots=1)
    tresh = orc.p.detector_thresh if tresh is None else tresh
    out = []
    for f in frames:
        t_in, l_in = tresh, lkl
        kn, tresh, lkl = orc.stage_a(0, f, tresh, lkl)
        out.append(dict(planes={n: orc.plane(0, n) for n in ("img0", "img1", "dog", "dx", "dy")}, mask=orc.mask(0), kl=orc.keylines(0),
                        kn=kn, tresh=tresh, lkl=lkl, retuned=F(orc.retuned(0)), tresh_in=t_in, lkl_in=l_in))
    orc.close()
    return out


_REF = {}


def ref_case(over, image, kind="ref"):
    """The reference on one image from the first-frame state (tresh = detector_thresh, l_kl_num = 0); cached, read-only."""
    k = (kind, _key(over), image)
    if k not in _REF:
        r = run_oracle(kind, over, [images()[image]])[0]
        for a in list(r["planes"].values()) + [r["mask"], r["kl"]]:
            a.setflags(write=False)
        _REF[k] = r
    return _REF[k]


def params_of(over):
    return oracle.euroc_params(W, H, **over)


def restated(over, image, defect=None):
    r = ref_case(over, image)
    return restate_stage_a(r["planes"], params_of(over), r["tresh_in"], r["lkl_in"], defect)


# ---- parameter sets ----------------------------------------------------------------------------------------------------------------
POS_NEG = (0.0, 0.2, 0.28, 0.36, 1.0)
CUT_IMAGES = ("vstep_up", "checker4", "noise8")
GROUPS = (["euroc", "base", "gain0_outside_clamp", "low_thresh", "low_thresh_pos_neg_1.0"] + [f"pos_neg_{v}" for v in POS_NEG]
          + [f"thr_g:{n}" for n in IMAGE_NAMES] + [f"thr_d:{n}" for n in IMAGE_NAMES] + [f"cut:{n}" for n in CUT_IMAGES])


# thr_d = thr_g * dog_thresh^2 rises with the detector threshold: at the shipped dog_thresh an edge whose gradient sits on thr_g fails the
# DoG-gradient gate anyway (a step: n2g 21 706, n2_m 58, thr_d 197), and the first gate would decide nothing that shows
THR_G_BASE = dict(BASE, dog_thresh=0.01)


def _f32_neighbours(v, n):
    out = [F(v)]
    for _ in range(n):
        out = [np.nextafter(out[0], F(-np.inf))] + out + [np.nextafter(out[-1], F(np.inf))]
    return out


def _median_first(vals):
    """The distinct values, the median first and outwards from it: a threshold on the median of an edge whose pixels differ only in
    their last bits leaves ragged chains (KeyLines with a rejected neighbour), a threshold on the minimum leaves the chains whole."""
    return vals[np.argsort(np.abs(np.arange(len(vals)) - len(vals) // 2), kind="stable")]


def search_thr_g(image):
    """A detector_thresh whose thr_g = fl(fl(t * 765)^2) equals the squared gradient of a pixel that is a KeyLine at BASE, so that
    `<` against `<=` decides that pixel: for each distinct value, the float nearest sqrt(v) / 765 and three ulps either way.
    -> (t, value, tried, hit) or None."""
    r = restated(BASE, image)
    vals = _median_first(np.unique(r["n2g"][r["gate"] == KEYLINE]))
    hit, first, decides = 0, None, None
    planes, p = ref_case(BASE, image)["planes"], params_of(THR_G_BASE)
    for v in vals:
        for t in _f32_neighbours(np.sqrt(np.float64(v)) / MAX_IMG, 3):
            if thr_g_of(t) == v:
                hit += 1
                first = first or (float(t), v)
                if decides is None and hit <= 8:      # prefer a value at which the pixel survives the later gates too
                    a, b = (restate_build_mask(planes["dx"], planes["dy"], planes["dog"], p, float(t), d)["mask"] for d in (None, "grad_gate_le"))
                    if not np.array_equal(a, b):
                        decides = (float(t), v)
                break
    first = decides or first
    return None if first is None else first + (len(vals), hit)


def search_thr_d(image):
    """A dog_thresh (detector_thresh as BASE) whose thr_d equals a KeyLine's n2_m.  -> (dog_thresh, value, tried, hit) or None."""
    r = restated(BASE, image)
    vals = _median_first(np.unique(r["n2m"][r["gate"] == KEYLINE]))
    g = np.float64(F(F(BASE["detector_thresh"]) * F(MAX_IMG)))
    hit, first = 0, None
    for v in vals:
        for d in _f32_neighbours(np.sqrt(np.float64(v)) / g, 3):
            if thr_d_of(BASE["detector_thresh"], d) == v:
                hit += 1
                first = first or (float(d), v)
                break
    return None if first is None else first + (len(vals), hit)


def _others(image):
    """Two more images, so that a per-image parameter set still runs as a batch."""
    i = IMAGE_NAMES.index(image)
    return [image, IMAGE_NAMES[(i + 7) % len(IMAGE_NAMES)], IMAGE_NAMES[(i + 19) % len(IMAGE_NAMES)]]


def cut_points(image):
    """max_points values for one image: {1, T-1, T, T+1}, the last KeyLine of an image row and the first of the next, and either
    side of row 12 (the first band seam).  -> {label: max_points}"""
    r = restated(BASE, image)
    T = r["kn"]
    rows = r["kl"]["p_inx"] // W
    out = {"one": 1, "T-1": T - 1, "T": T, "T+1": T + 1}
    mid = rows[T // 2]
    last = int(np.nonzero(rows == mid)[0][-1])                               # index of the last KeyLine of a middle row
    if last + 2 < T:
        out["row_last"], out["row_next_first"] = last + 1, last + 2
    below = np.nonzero(rows < 12)[0]
    if len(below) and len(below) + 1 < T:
        out["band_last"], out["band_next_first"] = len(below), len(below) + 1
    return out


@functools.lru_cache(maxsize=None)
def param_sets(group):
    """-> list of (label, over, image names).  Empty where a search found nothing (the CPU test counts those)."""
    if group == "euroc":
        return [("euroc", dict(auto_gain=0.0), list(IMAGE_NAMES))]
    if group == "base":
        return [("base", dict(BASE), list(IMAGE_NAMES))]
    if group == "gain0_outside_clamp":      # auto_gain = 0 leaves a threshold below min_thresh alone
        return [(group, dict(auto_gain=0.0, detector_thresh=0.002), list(IMAGE_NAMES))]
    if group.startswith("low_thresh"):      # thr_d so low that pixels exactly on the half-pixel position gate become KeyLines
        return [(group, dict(BASE, detector_thresh=1e-4, dog_thresh=1e-3, **({"pos_neg_thresh": 1.0} if group.endswith("1.0") else {})),
                 list(IMAGE_NAMES))]
    if group.startswith("pos_neg_"):
        return [(group, dict(BASE, pos_neg_thresh=float(group[8:])), list(IMAGE_NAMES))]
    kind, image = group.split(":")
    if kind == "thr_g":
        s = search_thr_g(image)
        if s is None:
            return []
        lo, t, hi = _f32_neighbours(s[0], 1)
        return [(f"{group}:{n}", dict(THR_G_BASE, detector_thresh=float(v)), _others(image)) for n, v in (("below", lo), ("on", t), ("above", hi))]
    if kind == "thr_d":
        s = search_thr_d(image)
        if s is None:
            return []
        lo, d, hi = _f32_neighbours(s[0], 1)
        return [(f"{group}:{n}", dict(BASE, dog_thresh=float(v)), _others(image)) for n, v in (("below", lo), ("on", d), ("above", hi))]
    if kind == "cut":
        return [(f"{group}:{n}", dict(BASE, max_points=int(v), reference_points=max(1, int(v) * 3 // 4), track_points=max(1, int(v) * 3 // 4)),
                 _others(image)) for n, v in cut_points(image).items()]
    raise KeyError(group)


# ---- threshold-law sequences (auto_gain > 0) ----------------------------------------------------------------------------------------
def sequences():
    """name -> (over, frames).  tresh_k = Constrain(tresh_{k-1} - gain * (reference_points - l_kl_num_{k-1})); a blank frame has no
    KeyLines, the checkerboard has far more than reference_points."""
    im = images()
    b = blank()
    law = dict(detector_thresh=0.002, min_thresh=1e-4, max_thresh=0.004, reference_points=200, track_points=200)
    return {
        # min (0.002 - 200 g < min), then far above max, held there by a second rich frame, then blank frames bring it back down
        "clamp_both_ways": (dict(law, auto_gain=1e-5), [im["checker4"], im["checker4"], im["checker4"], b, b, b, b, im["vstep_up"]]),
        # a small gain: the threshold moves strictly inside [min, max] on every frame
        "inside": (dict(law, auto_gain=1e-7), [im["checker4"], im["vstep_up"], b, im["checker4"], im["noise8"]]),
    }


def clamp_state(p, tresh):
    return "max" if tresh == p.max_thresh else "min" if tresh == p.min_thresh else "inside"
