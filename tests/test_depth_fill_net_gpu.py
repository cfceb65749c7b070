"""GPU: the visualizer's depth fill from wire records (edgehip_depth_fill_net, the NET instantiation of k_depth_fill in
rebvo_amd/csrc/depth_fill.hip) against the reference's own grids (tests/golden/depth_fill_net/*.npz) and the numpy restatement
(tests/depth_fill_net_port.py), bit for bit.  Fails, not skips, when the library lacks the entry points."""
import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import depth_fill_net_port as port
from tests import depth_fill_port
from tests.test_depth_fill_net_cpu import NAMES, load

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_grid(got, want, what):
    """Bit for bit.  (No fixture and no real frame creates a NaN: nothing is exempt.)"""
    assert got[0].shape == want[0].shape, what
    assert np.array_equal(bits(got[0]), bits(want[0])), (what, "rho", int((bits(got[0]) != bits(want[0])).sum()))
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "s_rho", int((bits(got[1]) != bits(want[1])).sum()))
    assert np.array_equal(got[2], np.asarray(want[2], bool)), (what, "fixed")


def enable(eh, f):
    return eh.depth_fill_enable(f["bw"], f["iter_num"], f["thresh_rel_rho"], f["thresh_match_num"], f["bound_mode"], f["discard"], block_h=f["bh"])


@pytest.mark.parametrize("name", NAMES)
def test_fixture(name):
    """Two sequences: the fixture's records and none.  kl_size is the records' number, or 100 for the empty fixture."""
    f = load(name)
    kn = len(f["records"])
    eh = edgehip.EdgeHip(edgehip.euroc_params(f["w"], f["h"]), nseq=2, nslots=2)
    try:
        eh.net_enable(max(kn, 100))
        eh.upload_net_keylines(0, f["records"])
        assert enable(eh, f) == (f["w"] // f["bw"], f["h"] // f["bh"])
        eh.depth_fill_net(f["p_off"])
        assert_grid(eh.download_depth_grid(0), f["want"], name)
        empty = eh.download_depth_grid(1)
        assert (empty[0] == 1.0).all() and (empty[1] == 40.0).all() and not empty[2].any()
    finally:
        eh.close()


def test_ragged_batch():
    """Three different fixtures of one geometry in one launch (8437, 8437 and 0 records; fixture 3's p_off is the launch's, so its
    neighbours are checked against the port with that offset and their own records), and more records than KeyLines fit."""
    fs = [load(NAMES[0]), load(NAMES[2]), load(NAMES[4])]
    f3 = fs[1]
    eh = edgehip.EdgeHip(edgehip.euroc_params(376, 240, max_points=4000), nseq=3, nslots=2)
    try:
        eh.net_enable(9000)   # > max_points: the fill bins in scratch of its own
        for s, f in enumerate(fs):
            eh.upload_net_keylines(s, f["records"])
        enable(eh, f3)
        eh.depth_fill_net(f3["p_off"])
        grids = eh.download_depth_grids([0, 1, 2])
        assert_grid(grids[1], f3["want"], "fixture 3")
        for s in (0, 2):
            want = port.depth_fill_net(fs[s]["records"], 376, 240, f3["bw"], f3["bh"], f3["iter_num"], f3["thresh_rel_rho"],
                                       f3["thresh_match_num"], f3["bound_mode"], f3["discard"], f3["p_off"])
            assert_grid(grids[s], want, ("port", s))
        enable(eh, fs[0])     # ... and with fixture 1's parameters and no offset: sequences 0 and 2 equal their own fixtures
        eh.depth_fill_net()
        grids = eh.download_depth_grids([0, 1, 2])
        assert_grid(grids[0], fs[0]["want"], "fixture 1")
        assert_grid(grids[2], fs[2]["want"], "fixture 5")
    finally:
        eh.close()


def test_pack_then_fill_then_the_other_fill():
    """net_pack + depth_fill_net on real frames equals the port on the downloaded records; depth_surface runs on it; depth_fill on the
    same slot then gives the tracker-list grids exactly as without any net call: shared outputs, no shared state."""
    w, h, nseq, frames_n = 376, 240, 2, 6
    frames = [f for f, _, _ in synth.billboard_sequence(w, h, frames_n + nseq)]
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
    try:
        eh.net_enable(eh.cap)
        eh.depth_fill_enable(10, 10, 1.0, 2, 0, 1)
        eh.depth_surface_enable(True, 1)
        for k in range(frames_n):
            eh.upload_rgb(eh.next_slot(), np.stack([frames[k + s] for s in range(nseq)]))
            eh.process_frame(np.full(nseq, 0.05 * k))
        cur = eh.cur_slot()
        eh.depth_fill(cur)
        before = eh.download_depth_grids([0, 1])
        eh.net_pack(cur)
        eh.depth_fill_net()
        got = eh.download_depth_grids([0, 1])
        for s in range(nseq):
            rec, hdr = eh.net_keylines(s)
            assert hdr["kline_num"] == len(rec) > 3000
            assert_grid(got[s], port.depth_fill_net(rec, w, h, 10, 10, 10, 1.0, 2, 0, 1), ("net", s))
            assert got[s][2].sum() > 50
            assert not np.array_equal(bits(got[s][0]), bits(before[s][0]))   # quantised depths: another grid than the tracker list's
        eh.depth_surface()
        surf = eh.download_depth_surface(0)
        assert np.isfinite(surf["dist"]).all() and surf["min_dist"] > 0
        eh.depth_fill(cur)
        after = eh.download_depth_grids([0, 1])
        for s in range(nseq):
            assert_grid(after[s], before[s], ("restored", s))
            kl, _ = eh.download_keylines(s, cur, want_mask=False)
            assert_grid(after[s], depth_fill_port.depth_fill(kl, w, h, 10, 10, 10, 1.0, 2, 0, 1), ("port", s))
    finally:
        eh.close()


def test_state_errors():
    eh = edgehip.EdgeHip(edgehip.euroc_params(64, 48), nseq=2, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        import ctypes as C
        z = C.c_float(0)
        assert lib.edgehip_depth_fill_net(ctx, z, z) == ERR_STATE    # neither
        eh.depth_fill_enable(8, 2)
        assert lib.edgehip_depth_fill_net(ctx, z, z) == ERR_STATE    # before net_enable
        eh.net_enable(16)
        eh.depth_fill_enable(None)
        assert lib.edgehip_depth_fill_net(ctx, z, z) == ERR_STATE    # the fill off
        assert lib.edgehip_depth_fill_net(None, z, z) == ERR_ARG
        eh.depth_fill_enable(8, 2)
        eh.depth_fill_net()                                          # usable afterwards: no records, ResetData's grid
        rho, s_rho, fixed = eh.download_depth_grid(1)
        assert (rho == 1.0).all() and (s_rho == 40.0).all() and not fixed.any()
    finally:
        eh.close()
