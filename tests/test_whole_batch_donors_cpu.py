"""CPU: the preconditions of tests/test_whole_batch_vs_ref_gpu.py, wherever the reference oracle (oracle/_ref) exists.

The ragged batch is only a test of per-sequence indexing if its donors really differ: lists from a few hundred KeyLines to the cap,
at the small cap at least two lists cut at exactly `cap` beside at least two shorter than cap / 4, an empty new list, an empty old
list, and a deal that puts four different donors at sequences 0, 63, 64 and B - 1 and every empty donor between two full ones.  And
the input of the skipped-KeyLine test (s_rho = 0, skipped by match count) must leave the reference itself finite, in both of its
instantiations: only then is a NaN on the device the device's own."""
import numpy as np
import pytest

from helpers import check_donor_preconditions, deal_donors, skipped_keyline_pair, whole_batch_donors


def _need_ref():
    from oracle import oracle
    if not oracle.available("ref"):
        pytest.skip("oracle/_ref not built on this machine (the reference tree is absent)")


@pytest.mark.parametrize("w,h,B,cap,small", [(376, 240, 200, 16000, False), (376, 240, 200, 2048, True),
                                              (752, 480, 72, 16000, False), (752, 480, 72, 4096, True)])
def test_donors_and_deal(w, h, B, cap, small):
    _need_ref()
    donors = whole_batch_donors(w, h, cap)
    check_donor_preconditions(donors, deal_donors(donors, B), cap, small)
    for d in donors:
        d["orc"].close()


@pytest.mark.parametrize("f32", [False, True])
def test_the_reference_stays_finite_on_skipped_keylines_with_zero_s_rho(f32):
    _need_ref()
    orc, so, sn, nav, idx = skipped_keyline_pair()
    assert len(idx) >= 10
    orc.set_tracker_f32(int(f32))
    orc.build_field(sn, 40, orc.retuned(sn))
    orc.set_framecount(sn, 3)
    q = orc.quantile(so)
    ref = orc.minimizer_rv(sn, so, nav.V[:], nav.W[:], 0.5, 5, 2, 2.0, q, 2, 2)
    for k in ("F", "V", "W", "RVel", "RW0"):
        assert np.all(np.isfinite(ref[k])), (k, ref[k])
    assert np.linalg.norm(ref["V"]) > 1e-4          # a real estimate, not an early return
    orc.close()


def test_the_reference_divides_a_skipped_keylines_zero_row_by_its_s_rho():
    """Why the fp64 cases of test_skipped_keylines_with_zero_s_rho part from the reference: its un-reweighted TryVelRot is NaN on this
    input (0 / 0 for the skipped KeyLines, global_tracker.cpp:456-461), its reweighted one (q_rho = 1) is finite."""
    _need_ref()
    orc, so, sn, nav, idx = skipped_keyline_pair()
    orc.build_field(sn, 40, orc.retuned(sn))
    orc.set_framecount(sn, 3)
    q = orc.quantile(so)
    X = np.r_[np.array(nav.V[:]), np.array(nav.W[:])]
    F, JtJ, JtF, _ = orc.try_velrot(sn, so, X, False, True, 0.5, q, 2, 2.0)
    assert np.isnan(F) and np.all(np.isnan(JtJ)) and np.all(np.isnan(JtF))
    F, JtJ, JtF, _ = orc.try_velrot(sn, so, X, True, True, 0.5, q, 2, 2.0)
    assert np.isfinite(F) and np.all(np.isfinite(JtJ)) and np.all(np.isfinite(JtF))
    orc.close()
