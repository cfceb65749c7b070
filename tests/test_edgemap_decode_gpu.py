"""GPU: the receiving side of the compressed edge map on the device — edgehip_upload_edgemap, edgehip_edgemap_decode (k_em_decode),
edgehip_edgemap_hide_visible (k_em_hide) and edgehip_depth_fill_segments (k_em_items + the segment source of k_depth_fill) — against
the compiled reference's fixtures (tests/golden/edgemap_decode/*.npz) and the numpy port (tests/edgemap_decode_port.py), bit for bit.
Fails, not skips, when the library lacks the entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import edgemap_crafted
from tests import edgemap_decode_crafted as crafted
from tests import edgemap_decode_port as port

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
PCAM = (crafted.CAM[0], crafted.CAM[1], crafted.CAM[4], crafted.W, crafted.H)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_grid(got, want, what):
    """rho and s_rho in their bits, fixed as it is.  (No input creates a NaN: nothing is exempt.)"""
    for name, g, w in zip(("rho", "s_rho"), got[:2], want[:2]):
        g, w = bits(g).reshape(-1), bits(w).reshape(-1)
        assert g.shape == w.shape and np.array_equal(g, w), (what, name, int((g != w).sum()))
    assert np.array_equal(np.asarray(got[2], bool).reshape(-1), np.asarray(want[2], bool).reshape(-1)), (what, "fixed")


def small_ctx(nseq, cap_records=crafted.CAP_RECORDS, cap_segments=crafted.CAP_SEGMENTS, cap_items=crafted.CAP_ITEMS, iter_num=crafted.ITER_NUM):
    p = edgehip.euroc_params(crafted.W, crafted.H, ppx=crafted.CAM[0], ppy=crafted.CAM[1], zfx=crafted.CAM[2], zfy=crafted.CAM[3], max_points=512)
    eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2)
    eh.edgemap_enable(cap_records)
    eh.edgemap_decode_enable(cap_segments, cap_items)
    eh.depth_fill_enable(crafted.BW, iter_num, bound_mode=crafted.BOUND_MODE, block_h=crafted.BH)
    return eh


def records_of(c):
    return np.frombuffer(np.ascontiguousarray(c["records"]).tobytes(), edgehip.COMPRESSED_KL_DTYPE)


def views_of(meta, v, nseq):
    DPose, DPos, _ = port.update_pos(meta["em_nav"], meta["views"][v])
    return [(DPose, DPos, float(meta["em_nav"][12]), float(meta["views"][v][12]))] * nseq


def check_against_fixture(eh, seq, c, meta, what):
    segs, flags, status = eh.download_edgemap_segments(seq)
    assert status == 0, what
    assert segs.tobytes() == c["segments"].tobytes() and flags.all(), what
    return segs


def test_crafted_fixtures():
    """Every crafted list as a sequence of one batch (thresholds differ between lists: one fill per pair of thresholds)."""
    meta, cases = crafted.load("crafted")
    names = crafted.names()
    eh = small_ctx(len(names))
    try:
        for s, name in enumerate(names):
            eh.upload_edgemap(s, records_of(cases[name]), float(cases[name]["params"][0]))
        eh.edgemap_decode()
        for s, name in enumerate(names):
            check_against_fixture(eh, s, cases[name], meta, name)
        for thr in sorted({(float(c["params"][1]), float(c["params"][2])) for c in cases.values()}):
            eh.depth_fill_segments(*thr)
            for s, name in enumerate(names):
                c = cases[name]
                if (float(c["params"][1]), float(c["params"][2])) == thr:
                    assert_grid(eh.download_depth_grid(s), (c["chain_rho"], c["chain_s_rho"], c["chain_fixed"]), name)
                    assert eh.download_edgemap_segments(s)[2] == 0
        # the views in order: flags are sticky, s_num counts what was visible and stays visible
        for v in range(len(meta["views"])):
            s_num = eh.edgemap_hide_visible(views_of(meta, v, len(names)))
            for s, name in enumerate(names):
                _, flags, _ = eh.download_edgemap_segments(s)
                assert np.array_equal(flags, cases[name]["flags"][v]), (name, v)
                assert s_num[s] == cases[name]["s_num"][v], (name, v)
    finally:
        eh.close()


@pytest.mark.parametrize("tag", ["frame3", "frame5", "frame6"])
def test_billboard_fixtures(tag):
    """The billboard frames' records: grid in LDS (8-px blocks), in HBM (3-px blocks: 85 x 64 cells) and with a boundary (8 x 4)."""
    meta, cases = crafted.load("billboard")
    c = cases[tag]
    w, h, bw, bh, iters, mode = (int(v) for v in c["geometry"])
    g = np.load(os.path.join(crafted.ROOT, "tests", "golden", "billboard_256x192.npz"))
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h, **dict(eval(str(g["over"])))), nseq=2, nslots=2)
    try:
        rec = records_of(c)
        eh.edgemap_enable(len(rec))
        eh.edgemap_decode_enable(len(rec), 40000)
        eh.depth_fill_enable(bw, iters, bound_mode=mode, block_h=bh)
        eh.upload_edgemap(1, rec, float(c["params"][0]))
        eh.edgemap_decode()
        check_against_fixture(eh, 1, c, meta, tag)
        assert len(eh.download_edgemap_segments(0)[0]) == 0
        eh.depth_fill_segments(float(c["params"][1]), float(c["params"][2]))
        assert_grid(eh.download_depth_grid(1), (c["chain_rho"], c["chain_s_rho"], c["chain_fixed"]), tag)
        empty = eh.download_depth_grid(0)
        assert not empty[2].any()
        for v in range(len(meta["views"])):
            s_num = eh.edgemap_hide_visible([None, views_of(meta, v, 1)[0]])
            assert s_num.tolist() == [-1, int(c["s_num"][v])]
            assert np.array_equal(eh.download_edgemap_segments(1)[1], c["flags"][v]), v
    finally:
        eh.close()


def _alone(records, rho_scale, thr, use_visibility=False, views=(), **caps):
    eh = small_ctx(1, **caps)
    try:
        eh.upload_edgemap(0, records, rho_scale)
        eh.edgemap_decode()
        for v in views:
            eh.edgemap_hide_visible([v])
        eh.depth_fill_segments(thr[0], thr[1], use_visibility)
        return eh.download_edgemap_segments(0), eh.download_depth_grid(0)
    finally:
        eh.close()


def test_ragged_batch_equals_each_alone():
    """A billboard list cut to the store, a crafted list and an empty one in one launch: each equals its own result alone."""
    _, bb = crafted.load("billboard")
    lists = [(records_of(bb["frame3"])[:crafted.CAP_RECORDS], float(bb["frame3"]["params"][0])), (crafted.case("mixed")["records"], 1.0),
             (crafted.case("empty")["records"], 1.0)]
    thr = (1.0, 60.0)
    eh = small_ctx(3, cap_segments=64)
    try:
        for s, (rec, scale) in enumerate(lists):
            eh.upload_edgemap(s, rec, scale)
        eh.edgemap_decode()
        eh.depth_fill_segments(*thr)
        got = [(eh.download_edgemap_segments(s), eh.download_depth_grid(s)) for s in range(3)]
    finally:
        eh.close()
    assert len(got[0][0][0]) > 10 and got[0][1][2].sum() > 5
    for s, (rec, scale) in enumerate(lists):
        (segs, flags, status), grid = _alone(rec, scale, thr, cap_segments=64)
        assert got[s][0][0].tobytes() == segs.tobytes() and np.array_equal(got[s][0][1], flags) and got[s][0][2] == status == 0
        assert_grid(got[s][1], grid, s)


def test_capacities_exceeded_by_one():
    """cap_segments: the list is cut in order and flagged, the fill folds the cut list.  cap_items: flagged, nothing of the sequence is
    folded (its grid is the chain behind ResetData).  The neighbours are unchanged."""
    c = crafted.case("mixed")
    full_segs, _ = port.decode(c["records"], 1.0)
    thr = (c["v_thresh"], c["a_thresh"])
    rho, s_rho, fixed, gates = port.fill_depth_map(full_segs, None, crafted.W, crafted.H, crafted.BW, crafted.BH, PCAM, *thr)
    n_items = sum(int(np.ceil(np.hypot(float(s[4]) - float(s[0]), float(s[5]) - float(s[1])))) for s, g in zip(full_segs, gates) if g == 0)
    want_full = port.chain(rho, s_rho, fixed, crafted.W, crafted.H, crafted.BW, crafted.BH, crafted.ITER_NUM, crafted.BOUND_MODE)
    reset = port.chain(np.ones(48), np.full(48, 40.0), np.zeros(48, bool), crafted.W, crafted.H, crafted.BW, crafted.BH, crafted.ITER_NUM, crafted.BOUND_MODE)
    nb = crafted.case("shared_vertex")
    (nb_segs, _, _), nb_grid = _alone(nb["records"], 1.0, thr)

    for cap_segments, cap_items in ((len(full_segs) - 1, crafted.CAP_ITEMS), (crafted.CAP_SEGMENTS, n_items - 1), (crafted.CAP_SEGMENTS, n_items)):
        eh = small_ctx(3, cap_segments=cap_segments, cap_items=cap_items)
        try:
            for s, rec in enumerate((nb["records"], c["records"], nb["records"])):
                eh.upload_edgemap(s, rec, 1.0)
            eh.edgemap_decode()
            eh.depth_fill_segments(*thr)
            segs, flags, status = eh.download_edgemap_segments(1)
            grid = eh.download_depth_grid(1)
            if cap_segments < len(full_segs):
                assert status == edgehip.EDGEMAP_SEGMENT_OVERFLOW
                assert segs.tobytes() == full_segs[:cap_segments].tobytes()
                r2, s2, f2, _ = port.fill_depth_map(full_segs[:cap_segments], None, crafted.W, crafted.H, crafted.BW, crafted.BH, PCAM, *thr)
                assert_grid(grid, port.chain(r2, s2, f2, crafted.W, crafted.H, crafted.BW, crafted.BH, crafted.ITER_NUM, crafted.BOUND_MODE), "cut")
            elif cap_items < n_items:
                assert status == edgehip.EDGEMAP_ITEM_OVERFLOW and segs.tobytes() == full_segs.tobytes()
                assert_grid(grid, reset, "items over")
            else:                                   # exactly cap_items items fit
                assert status == 0
                assert_grid(grid, want_full, "items fit")
            for s in (0, 2):
                got = eh.download_edgemap_segments(s)
                assert got[0].tobytes() == nb_segs.tobytes() and got[2] == 0
                assert_grid(eh.download_depth_grid(s), nb_grid, ("neighbour", s))
        finally:
            eh.close()


def test_compress_decode_fill_on_the_device_equals_the_round_trip():
    """edgehip_edgemap_compress leaves records and rho_scale in the store: decode + fill from there equals download -> upload_edgemap ->
    decode -> fill in a second context."""
    W, H = edgemap_crafted.W, edgemap_crafted.H
    kl, p = edgemap_crafted.case("mixed")
    p = dict(p, scale=1.7)
    thr = (0.5, 60.0)

    def ctx():
        eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=edgemap_crafted.MAX_POINTS), nseq=2, nslots=2)
        eh.edgemap_enable(2 * edgemap_crafted.MAX_POINTS)
        eh.edgemap_decode_enable(2 * edgemap_crafted.MAX_POINTS, 20000)
        eh.depth_fill_enable(10, 4)
        return eh

    a, b = ctx(), ctx()
    try:
        a.upload_keylines(1, 0, kl)
        a.edgemap_compress(0, edgemap_crafted.params_struct(p), [1.0, p["scale"]])
        a.edgemap_decode()
        a.depth_fill_segments(*thr)
        rec, status = a.download_edgemap(1)
        assert status == 0 and len(rec) > 4
        b.upload_edgemap(1, rec, float(np.float32(p["scale"])))
        b.edgemap_decode()
        b.depth_fill_segments(*thr)
        sa, sb = a.download_edgemap_segments(1), b.download_edgemap_segments(1)
        assert len(sa[0]) > 2 and sa[0].tobytes() == sb[0].tobytes()
        want, _ = port.decode(rec, np.float32(p["scale"]))
        assert sa[0].tobytes() == want.tobytes()
        ga, gb = a.download_depth_grid(1), b.download_depth_grid(1)
        assert ga[2].any()
        assert_grid(ga, gb, "round trip")
        # edgehip_depth_fill afterwards gives its own grid exactly as before: outputs are shared, state is not
        fresh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=edgemap_crafted.MAX_POINTS), nseq=2, nslots=2)
        try:
            fresh.upload_keylines(1, 0, kl)
            fresh.depth_fill_enable(10, 4)
            fresh.depth_fill(0)
            want_kl = fresh.download_depth_grid(1)
        finally:
            fresh.close()
        a.depth_fill(0)
        assert_grid(a.download_depth_grid(1), want_kl, "depth_fill after depth_fill_segments")
        assert want_kl[2].any() and not np.array_equal(bits(want_kl[0]), bits(ga[0]))
    finally:
        a.close()
        b.close()


def test_hide_visible_twice_and_use_visibility():
    """Two views one after the other: a flag that is 0 stays 0.  Then the fill with use_visibility against the port."""
    meta, _ = crafted.load("crafted")
    c = crafted.case("mixed")
    thr = (c["v_thresh"], c["a_thresh"])
    segs, flags = port.decode(c["records"], 1.0)
    eh = small_ctx(2)
    try:
        eh.upload_edgemap(0, c["records"], 1.0)
        eh.upload_edgemap(1, c["records"], 1.0)
        eh.edgemap_decode()
        history = []
        all_visible = port.chain(*port.fill_depth_map(segs, None, crafted.W, crafted.H, crafted.BW, crafted.BH, PCAM, *thr)[:3],
                                 crafted.W, crafted.H, crafted.BW, crafted.BH, crafted.ITER_NUM, crafted.BOUND_MODE)
        for v in (1, 0):
            view = views_of(meta, v, 1)[0]
            s_num = eh.edgemap_hide_visible([view, None])
            want = port.hide_visible(segs, flags, view[0], view[1], view[2], view[3], PCAM)
            got = eh.download_edgemap_segments(0)[1]
            assert np.array_equal(got, flags) and s_num.tolist() == [want, -1]
            history.append(got.copy())
            assert eh.download_edgemap_segments(1)[1].all()          # the NULL row: left alone
            for use in (False, True):
                eh.depth_fill_segments(thr[0], thr[1], use)
                r, s, f, gates = port.fill_depth_map(segs, flags, crafted.W, crafted.H, crafted.BW, crafted.BH, PCAM, thr[0], thr[1], use)
                want_grid = port.chain(r, s, f, crafted.W, crafted.H, crafted.BW, crafted.BH, crafted.ITER_NUM, crafted.BOUND_MODE)
                assert_grid(eh.download_depth_grid(0), want_grid, ("use_visibility", use, v))
                assert_grid(eh.download_depth_grid(1), all_visible, "all visible")
                if use and v == 1:    # some folded segments are hidden, some are not: the grid is neither the full one nor empty
                    assert f.any() and not np.array_equal(bits(want_grid[0]), bits(all_visible[0]))
        assert not (history[1] & ~history[0]).any() and 0 < history[1].sum() < history[0].sum() < len(flags)
        assert (gates == -1).any()
    finally:
        eh.close()


def test_other_scalings_against_the_port():
    """x_scaling / y_scaling other than 0.5 and 1 (this library's extension)."""
    c = crafted.case("mixed")
    eh = small_ctx(1)
    try:
        eh.upload_edgemap(0, c["records"], 1.0)
        eh.edgemap_decode(1.0, 2.0)
        want, _ = port.decode(c["records"], 1.0, x_scaling=1.0, y_scaling=2.0)
        assert eh.download_edgemap_segments(0)[0].tobytes() == want.tobytes()
    finally:
        eh.close()


def test_state_errors():
    p = edgehip.euroc_params(crafted.W, crafted.H, max_points=512)
    eh = edgehip.EdgeHip(p, nseq=2, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    rec = crafted.case("diagonal")["records"]
    ptr = C.c_void_p(rec.ctypes.data)
    d = C.c_double
    try:
        assert lib.edgehip_upload_edgemap(ctx, 0, ptr, len(rec), C.c_float(1)) == ERR_STATE          # no store
        assert lib.edgehip_edgemap_decode(ctx, d(0), d(0)) == ERR_STATE                               # no decoder
        assert lib.edgehip_depth_fill_segments(ctx, d(1), d(45), 0) == ERR_STATE                      # no fill
        eh.depth_fill_enable(8, 2)
        assert lib.edgehip_depth_fill_segments(ctx, d(1), d(45), 0) == ERR_STATE                      # no decoder
        eh.edgemap_decode_enable(8, 64)
        assert lib.edgehip_edgemap_decode(ctx, d(0), d(0)) == ERR_STATE                               # decoder, but no store
        eh.edgemap_enable(4)
        assert lib.edgehip_depth_fill_segments(ctx, d(1), d(45), 0) == ERR_STATE                      # nothing decoded yet
        assert lib.edgehip_edgemap_hide_visible(ctx, None, None, None, None, None) == ERR_STATE
        for count in (-1, 5):
            assert lib.edgehip_upload_edgemap(ctx, 0, ptr, count, C.c_float(1)) == ERR_ARG           # outside [0, cap_records]
        for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-37):     # 1e-37: (32767 / 20) / rho_scale overflows a float
            assert lib.edgehip_upload_edgemap(ctx, 0, ptr, 2, C.c_float(bad)) == ERR_ARG, bad         # getPair divides by it
        assert lib.edgehip_upload_edgemap(ctx, 2, ptr, 2, C.c_float(1)) == ERR_ARG                    # sequence out of range
        assert lib.edgehip_upload_edgemap(ctx, 0, None, 2, C.c_float(1)) == ERR_ARG
        assert lib.edgehip_upload_edgemap(None, 0, ptr, 2, C.c_float(1)) == ERR_ARG
        assert lib.edgehip_edgemap_decode(ctx, d(-1), d(0)) == ERR_ARG
        assert lib.edgehip_edgemap_decode_enable(ctx, -1, 0) == ERR_ARG
        assert lib.edgehip_upload_edgemap(ctx, 0, ptr, 2, C.c_float(1)) == 0
        assert lib.edgehip_upload_edgemap(ctx, 1, None, 0, C.c_float(1)) == 0                         # an empty list
        eh.edgemap_decode()
        assert lib.edgehip_edgemap_hide_visible(ctx, None, None, None, None, None) == ERR_ARG
        assert lib.edgehip_depth_fill_segments(ctx, d(float("nan")), d(45), 0) == ERR_ARG
        eh.depth_fill_segments(2.0, 10.0)
        segs, flags, status = eh.download_edgemap_segments(0)
        assert len(segs) == 1 and status == 0
        assert eh.download_depth_grid(0)[2].any() and not eh.download_depth_grid(1)[2].any()
        eh.edgemap_decode_enable(0)                                                                   # 0 frees
        assert lib.edgehip_edgemap_decode(ctx, d(0), d(0)) == ERR_STATE
        assert lib.edgehip_depth_fill_segments(ctx, d(1), d(45), 0) == ERR_STATE
        eh.depth_fill_enable(None)
    finally:
        eh.close()
