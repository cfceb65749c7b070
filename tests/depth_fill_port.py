"""CPU restatement of the reference's depth_filler (src/visualizer/depth_filler.cpp) in numpy, in the reference's own order of
operations: ResetData -> FillEdgeData(edge_tracker&, ...) -> InitCoarseFine -> Integrate(iter_num).

What the GPU tests compare against where the inputs are too large for fixtures.  Every fp64 sum is formed in the reference's
order (np.add.accumulate is a sequential loop, unlike np.sum); the Gauss-Seidel sweeps of Integrate1Step run on the skewed
wavefront t = x + 2 y + 4 k that rebvo_amd/csrc/depth_fill.hip runs (raster_sweeps() below is the plain raster loop it must equal).
"""
import numpy as np

RHO_MAX = 20.0                      # include/mtracklib/edge_finder.h:38
I_RHO0 = 1.0 / ((RHO_MAX * 2) ** 2)  # ResetData (depth_filler.cpp:41-56)
S_RHO0 = RHO_MAX * 2
I_WEAK = 1.0 / (RHO_MAX * RHO_MAX)   # FillEdgeData's weight of a KeyLine that fails the match test (discart == false)

BOUND_NONE, BOUND_CORNERS, BOUND_FULL = 0, 1, 2
FIELDS = ("c_p", "rho", "s_rho", "rho0", "m_num", "p_id", "n_id")   # what the fill reads of a KeyLine


def grid_size(w, h, bw, bh):
    return w // bw, h // bh


def _f2u32(q):
    """(uint) of a float as the reference's x86-64 build converts it: cvttss2si to 64 bits, low 32 bits kept (0 for NaN / overflow)."""
    q = np.asarray(q, np.float32).astype(np.float64)
    ok = np.isfinite(q) & (np.abs(q) < 9.2e18)
    t = np.where(ok, np.trunc(np.where(ok, q, 0.0)), 0.0).astype(np.int64)
    return (t & 0xFFFFFFFF).astype(np.uint64)


def cell_index(c_p, gw, gh, bw, bh):
    """GetIndex((uint)(c_p.x / bw), (uint)(c_p.y / bh)) = y * gw + x in 32-bit unsigned arithmetic (Image::GetIndex,
    include/VideoLib/image.h:113); -1 where that lands past the grid (the reference writes out of bounds there)."""
    c_p = np.asarray(c_p, np.float32).reshape(-1, 2)
    x = _f2u32(c_p[:, 0] / np.float32(bw))
    y = _f2u32(c_p[:, 1] / np.float32(bh))
    idx = (y * np.uint64(gw) + x) & np.uint64(0xFFFFFFFF)
    return np.where(idx < np.uint64(gw * gh), idx.astype(np.int64), -1)


def inboundary(x, y, gw, gh, mode):
    x, y = np.asarray(x), np.asarray(y)
    if mode == BOUND_NONE:
        return np.zeros(np.broadcast(x, y).shape, bool)
    if mode == BOUND_CORNERS:
        return ((x == 0) | (x == gw - 1)) & ((y == 0) | (y == gh - 1))
    return (x == 0) | (x == gw - 1) | (y == 0) | (y == gh - 1)


def fill_edge_data(kl, gw, gh, bw, bh, thresh_rel_rho, thresh_match_num, discard):
    """ResetData + FillEdgeData(edge_tracker&, v_thresh, m_num_t, discart) (depth_filler.cpp:113-163) -> rho, s_rho, fixed (flat).
    The KeyLines of one cell are folded in list order; the cells are independent, so the r-th KeyLine of every cell is folded at once.
    Nothing is written back into `kl` (the reference sets kl.rho = kl.rho0 for a negative rho it accepts)."""
    G = gw * gh
    rho = np.ones(G)
    s_rho = np.full(G, S_RHO0)
    I = np.full(G, I_RHO0)
    fixed = np.zeros(G, bool)
    kn = len(kl["rho"])
    if kn == 0:
        return rho, s_rho, fixed
    k_rho = np.asarray(kl["rho"], np.float64)
    k_srho = np.asarray(kl["s_rho"], np.float64)
    with np.errstate(all="ignore"):
        keep = ~(k_srho / k_rho > thresh_rel_rho)
        k_I = 1.0 / (k_srho * k_srho)
    # kl.rho <= 0 is false for a NaN rho (IEEE), as in the reference
    bad = (np.asarray(kl["m_num"]) < thresh_match_num) | (np.asarray(kl["p_id"]) < 0) | (np.asarray(kl["n_id"]) < 0) | (k_rho <= 0)
    if discard:
        keep &= ~bad
    k_I = np.where(bad, I_WEAK, k_I)
    k_rho = np.where(bad & (k_rho < 0), np.asarray(kl["rho0"], np.float64), k_rho)
    cell = cell_index(kl["c_p"], gw, gh, bw, bh)
    keep &= cell >= 0
    ids = np.nonzero(keep)[0]
    if len(ids) == 0:
        return rho, s_rho, fixed
    cells = cell[ids]
    order = np.argsort(cells, kind="stable")
    ids, cells = ids[order], cells[order]
    start = np.r_[0, np.nonzero(np.diff(cells))[0] + 1]
    rank = np.arange(len(ids)) - np.repeat(start, np.diff(np.r_[start, len(ids)]))
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1):
            sel = rank == r
            c, i = cells[sel], ids[sel]
            i_rho = I[c] * rho[c]
            i_rho = i_rho + k_rho[i] * k_I[i]
            I[c] = I[c] + k_I[i]
            v = np.where(I[c] > 0, 1.0 / I[c], 1e20)
            rho[c] = i_rho * v
            s_rho[c] = np.sqrt(v)
            fixed[c] = True
    return rho, s_rho, fixed


def levels(gw, gh):
    """InitCoarseFine's tile sizes (depth_filler.cpp:236): (sx, sy) = (gw, gh), (gw/2, gh/2), ... while both are > 1."""
    out = []
    sx, sy = gw, gh
    while sx > 1 and sy > 1:
        out.append((sx, sy))
        sx //= 2
        sy //= 2
    return out


def init_coarse_fine(rho, s_rho, fixed, gw, gh, mode):
    """InitCoarseFine (depth_filler.cpp:233-278), on (gh, gw) arrays in place.  A level reads only fixed cells and the s_rho of
    boundary cells, which no level writes, so each level is computed from the same input and applied coarse to fine."""
    bnd = inboundary(np.arange(gw)[None, :], np.arange(gh)[:, None], gw, gh, mode)
    src_rho, src_srho = rho.copy(), s_rho.copy()
    for sx, sy in levels(gw, gh):
        ntx, nty = (gw - sx) // sx + 1, (gh - sy) // sy + 1
        sl = (slice(0, nty * sy), slice(0, ntx * sx))
        f = fixed[sl].reshape(nty, sy, ntx, sx).transpose(0, 2, 3, 1).reshape(nty, ntx, sx * sy)   # [ty, tx, dx * sy + dy]
        b = bnd[sl].reshape(nty, sy, ntx, sx).transpose(0, 2, 3, 1).reshape(nty, ntx, sx * sy)
        r = src_rho[sl].reshape(nty, sy, ntx, sx).transpose(0, 2, 3, 1).reshape(nty, ntx, sx * sy)
        s = src_srho[sl].reshape(nty, sy, ntx, sx).transpose(0, 2, 3, 1).reshape(nty, ntx, sx * sy)
        n = f.sum(-1)
        nr = (f | b).sum(-1)
        # skipped terms add +0.0: exact, the running sums start at +0.0 and never become -0.0
        with np.errstate(all="ignore"):
            mr = np.add.accumulate(np.where(f, r, 0.0), axis=-1)[..., -1]
            ms = np.add.accumulate(np.where(f | b, s, 0.0), axis=-1)[..., -1]
            mr = mr / np.maximum(n, 1)
            ms = ms / np.maximum(nr, 1)
        has = n > 0
        cell_has = np.repeat(np.repeat(has, sy, axis=0), sx, axis=1)
        wr = cell_has & ~fixed[sl]
        rho[sl][wr] = np.repeat(np.repeat(mr, sy, axis=0), sx, axis=1)[wr]
        ws = wr & ~bnd[sl]
        s_rho[sl][ws] = np.repeat(np.repeat(ms, sy, axis=0), sx, axis=1)[ws]


_NB = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]   # (dy, dx) in Integrate1Step's loop order


def sweeps(rho, s_rho, fixed, gw, gh, mode, iter_num):
    """iter_num x Integrate1Step (depth_filler.cpp:301-355) in place, as the skewed wavefront: at step t the cells (x, y) of sweep k
    with x + 2 y + 4 k = t update together.  Their upper / left neighbours were updated by sweep k at steps t-3 .. t-1, their lower /
    right ones by sweep k-1 at steps t-3 .. t-1 and not yet by sweep k (steps t+1 .. t+3): exactly what the raster loop reads."""
    if iter_num <= 0:
        return
    bnd = inboundary(np.arange(gw)[None, :], np.arange(gh)[:, None], gw, gh, mode)
    K = np.repeat(np.arange(iter_num), gh)
    Y = np.tile(np.arange(gh), iter_num)
    T = (gw - 1) + 2 * (gh - 1) + 4 * (iter_num - 1) + 1
    with np.errstate(all="ignore"):
        for t in range(T):
            X = t - 4 * K - 2 * Y
            on = (X >= 0) & (X < gw)
            x, y = X[on], Y[on]
            live = ~fixed[y, x]
            x, y = x[live], y[live]
            if len(x) == 0:
                continue
            r = np.zeros(len(x))
            sr = np.zeros(len(x))
            n = np.zeros(len(x), np.int64)
            for dy, dx in _NB:
                px, py = x + dx, y + dy
                ok = (px >= 0) & (px < gw) & (py >= 0) & (py < gh)
                pxc, pyc = np.clip(px, 0, gw - 1), np.clip(py, 0, gh - 1)
                r = np.where(ok, r + rho[pyc, pxc], r)
                sr = np.where(ok, sr + s_rho[pyc, pxc], sr)
                n += ok
            w = 1.0
            rho[y, x] = (1 - w) * rho[y, x] + w * r / n
            nb = ~bnd[y, x]
            s_rho[y[nb], x[nb]] = (sr / n)[nb]


def raster_sweeps(rho, s_rho, fixed, gw, gh, mode, iter_num):
    """Integrate1Step as the reference loops (y outer, x inner, in place): the scalar check of sweeps()."""
    import math
    for _ in range(iter_num):
        for y in range(gh):
            for x in range(gw):
                if fixed[y, x]:
                    continue
                r = sr = 0.0
                n = 0
                for dy, dx in _NB:
                    px, py = x + dx, y + dy
                    if px < 0 or px >= gw or py < 0 or py >= gh:
                        continue
                    r += float(rho[py, px])
                    sr += float(s_rho[py, px])
                    n += 1
                w = 1.0
                rho[y, x] = (1 - w) * float(rho[y, x]) + w * r / n if n else math.nan
                if not inboundary(x, y, gw, gh, mode):
                    s_rho[y, x] = sr / n if n else math.nan


def depth_fill(kl, w, h, bw, bh, iter_num=10, thresh_rel_rho=1.0, thresh_match_num=5, bound_mode=0, discard=1):
    """The whole chain of both reference callers -> (rho, s_rho, fixed) as (gh, gw) arrays.  `kl`: a mapping with the FIELDS
    (a KeyLine record array from edgehip / the oracle works as is)."""
    gw, gh = grid_size(w, h, bw, bh)
    rho, s_rho, fixed = fill_edge_data(kl, gw, gh, bw, bh, thresh_rel_rho, thresh_match_num, discard)
    rho, s_rho, fixed = rho.reshape(gh, gw), s_rho.reshape(gh, gw), fixed.reshape(gh, gw)
    init_coarse_fine(rho, s_rho, fixed, gw, gh, bound_mode)
    sweeps(rho, s_rho, fixed, gw, gh, bound_mode, iter_num)
    return rho, s_rho, fixed
