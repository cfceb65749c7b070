"""CPU restatement of the reference's depth_filler fed from wire records (src/visualizer/depth_filler.cpp:59-104), in numpy, in the
reference's own order of operations: ResetData -> FillEdgeData(net_keyline*, kn, p_off, ...) -> InitCoarseFine -> Integrate(iter_num),
the chain its visualizer runs per received frame (visualizer.cpp:436-439).  Everything behind FillEdgeData is tests/depth_fill_port.py's.

Against the edge_tracker overload: rho and s_rho come back from 16-bit quanta of 1 / NET_RHO_SCALING, the cell from the quantised
position plus p_off, a record that fails the match-count test folds with s_rho = RHO_MAX, and there is no p_id / n_id / rho <= 0 gate
and no rho0.
"""
import numpy as np

from tests import depth_fill_port as dfp

NET_RHO_SCALING = 10000.0   # include/CommLib/net_keypoint.h:32
NET_DTYPE = np.dtype({"names": ["qx", "qy", "rho", "s_rho", "n_kl", "m_num", "flow"],
                      "formats": ["<u2", "<u2", "<u2", "<u2", "<i4", "u1", ("u1", (2,))],
                      "offsets": [0, 2, 4, 6, 8, 12, 13], "itemsize": 15})   # rebvo::net_keyline, packed


def as_records(rec):
    """A NET_DTYPE view of records given as such, or as raw bytes of shape (kn, 15)."""
    rec = np.ascontiguousarray(rec)
    if rec.dtype.names is None:
        rec = np.ascontiguousarray(rec, np.uint8).reshape(-1, 15).view(NET_DTYPE).reshape(-1)
    return rec


def cell_index(qx, qy, p_off, gw, gh, bw, bh):
    """GetIndex((qx + p_off.x) / bl_size.w, (qy + p_off.y) / bl_size.h): u_short -> int -> float, float sum, float quotient by the
    u_int block size, then (uint) as the x86-64 build converts; -1 where the index lands past the grid (dropped)."""
    x = dfp._f2u32((qx.astype(np.float32) + np.float32(p_off[0])) / np.float32(bw))
    y = dfp._f2u32((qy.astype(np.float32) + np.float32(p_off[1])) / np.float32(bh))
    idx = (y * np.uint64(gw) + x) & np.uint64(0xFFFFFFFF)
    return np.where(idx < np.uint64(gw * gh), idx.astype(np.int64), -1)


def fill_edge_data_net(rec, p_off, gw, gh, bw, bh, thresh_rel_rho, thresh_match_num, discard):
    """ResetData + FillEdgeData(net_keyline*, ...) -> rho, s_rho, fixed (flat).  The records of one cell fold in list order; the cells
    are independent, so the r-th record of every cell is folded at once."""
    rec = as_records(rec)
    G = gw * gh
    rho = np.ones(G)
    s_rho = np.full(G, dfp.S_RHO0)
    I = np.full(G, dfp.I_RHO0)
    fixed = np.zeros(G, bool)
    if len(rec) == 0:
        return rho, s_rho, fixed
    k_rho = rec["rho"].astype(np.float64) / NET_RHO_SCALING
    k_srho = rec["s_rho"].astype(np.float64) / NET_RHO_SCALING
    with np.errstate(all="ignore"):
        keep = ~(k_srho / k_rho > thresh_rel_rho)
    weak = rec["m_num"].astype(np.int64) < thresh_match_num
    if discard:
        keep &= ~weak
    k_srho = np.where(weak, dfp.RHO_MAX, k_srho)
    with np.errstate(all="ignore"):
        k_I = 1 / (k_srho * k_srho)
    cell = cell_index(rec["qx"], rec["qy"], p_off, gw, gh, bw, bh)
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


def depth_fill_net(rec, w, h, bw, bh, iter_num=10, thresh_rel_rho=1.0, thresh_match_num=5, bound_mode=0, discard=1, p_off=(0.0, 0.0)):
    """The visualizer's chain -> (rho, s_rho, fixed) as (gh, gw) arrays."""
    gw, gh = dfp.grid_size(w, h, bw, bh)
    rho, s_rho, fixed = fill_edge_data_net(rec, p_off, gw, gh, bw, bh, thresh_rel_rho, thresh_match_num, discard)
    rho, s_rho, fixed = rho.reshape(gh, gw), s_rho.reshape(gh, gw), fixed.reshape(gh, gw)
    dfp.init_coarse_fine(rho, s_rho, fixed, gw, gh, bound_mode)
    dfp.sweeps(rho, s_rho, fixed, gw, gh, bound_mode, iter_num)
    return rho, s_rho, fixed
