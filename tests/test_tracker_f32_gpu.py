"""GPU: the tracker's float instantiation as a second configuration.

The reference has two instantiations of its tracker: global_tracker::Minimizer_RV<double> (x86, rebvo_second_t.cpp:346) and
Minimizer_RV<float> with TryVelRot<float, ...> (global_tracker.cpp:824; what USE_NE10 builds run, rebvo_second_t.cpp:339-343).
edgehip_set_tracker_precision(ctx, 32) runs the second one on the device (k_try_velrot_f32, the step kernel rounding JtJ / JtF / h / X
to float where the reference's assignments do).  The oracle here is the reference's OWN float instantiation, compiled from
global_tracker.cpp into oracle/_ref and switched on with ref_set_tracker_f32.

Tolerance, stated: float sums of ~8-14 k products added in different (fixed) trees agree to ~1e-6 relative, and the minimiser's state
inherits that through six 6x6 solves: |dV|, |dW| <= 2e-4 |X| + 2e-7 per frame pair (the reference's float and double instantiations
differ from EACH OTHER by 1e-5 relative on the same pair), the score 1e-4 relative.  Discrete results: the forward
matches (m_id_f) must be the float reference's on at least 99.5 % of the KeyLines (a projection that lands within a float ulp of a
pixel boundary may round either way), exactly equal KeyLine / match counts are required of whole sequences only through the pose
tolerance below.  The headline configuration stays fp64 and keeps its own (1e-7 / exact) bounds: tests/test_stage_b_gpu.py."""
import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from helpers import inject_pair, oracle_pair, rel_err, require_ref

pytestmark = pytest.mark.gpu

F32_REL, F32_ABS = 2e-4, 2e-7


def _pair(w, h):
    orc, so, sn, nav, frames = oracle_pair(w, h, 4)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=1, nslots=2)
    inject_pair(eh, orc, so, sn)
    return orc, so, sn, nav, eh


@pytest.mark.parametrize("w,h,init_type", [(376, 240, 2), (752, 480, 2), (376, 240, 0), (376, 240, 1)])
def test_minimizer_rv_float_against_the_reference_float_instantiation(w, h, init_type):
    require_ref()
    orc, so, sn, nav, eh = _pair(w, h)
    orc.set_tracker_f32(1)
    eh.set_tracker_precision(32)
    p = edgehip.euroc_params(w, h, tracker_init_type=init_type)
    eh2 = edgehip.EdgeHip(p, nseq=1, nslots=2)
    inject_pair(eh2, orc, so, sn)
    eh2.set_tracker_precision(32)
    orc.build_field(sn, 40, orc.retuned(sn))
    eh2.build_field(1, 40, -1.0)
    s_rho_q = orc.quantile(so)
    eh2.quantile(0)
    st = eh2.get_state(0)
    st.V[:] = nav.V[:]
    st.W[:] = nav.W[:]
    eh2.set_state(0, st)
    ref = orc.minimizer_rv(sn, so, nav.V[:], nav.W[:], 0.5, 5, init_type, 2.0, s_rho_q, 0, 2)
    eh2.minimizer_rv(1, 0)
    g = eh2.get_state(0)
    X, Xr = np.r_[np.array(g.V[:]), np.array(g.W[:])], np.r_[ref["V"], ref["W"]]
    tol = F32_REL * np.linalg.norm(Xr) + F32_ABS
    assert np.max(np.abs(X - Xr)) <= tol, (X, Xr, tol)
    assert rel_err(g.score, ref["F"]) < 1e-4
    assert rel_err(np.array(g.P_V[:]).reshape(3, 3), ref["RVel"]) < 1e-3 and rel_err(np.array(g.P_W[:]).reshape(3, 3), ref["RW0"]) < 1e-3
    assert g.minimizer_evals == (12 if init_type == 2 else 6)      # (init type 2: six of the twelve in three two-chain launches, k_try_velrot2_f32)
    # what the float tracker returns IS float: V, W are float values exactly (X is a Vector<6, float> in the reference)
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
    kl_ref = orc.keylines(so)
    kl_gpu, _ = eh2.download_keylines(0, 0, want_mask=False)
    same = float(np.mean(kl_ref["m_id_f"] == kl_gpu["m_id_f"]))
    assert same >= 0.995, same
    # ... and the float result is NOT the double one: the configuration really computes in float
    orc.set_tracker_f32(0)
    inject_pair(eh2, orc, so, sn)
    ref64 = orc.minimizer_rv(sn, so, nav.V[:], nav.W[:], 0.5, 5, init_type, 2.0, s_rho_q, 0, 2)
    assert np.max(np.abs(X - np.r_[ref64["V"], ref64["W"]])) > 1e-9
    # back to 64 bits: the fp64 bounds again
    eh2.set_tracker_precision(64)
    eh2.build_field(1, 40, -1.0)
    eh2.set_state(0, st)
    eh2.quantile(0)
    eh2.minimizer_rv(1, 0)
    g = eh2.get_state(0)
    assert np.allclose(np.r_[np.array(g.V[:]), np.array(g.W[:])], np.r_[ref64["V"], ref64["W"]], rtol=1e-7, atol=1e-9)
    eh.close()
    eh2.close()
    orc.close()


def test_whole_sequences_with_the_float_tracker_follow_the_float_reference():
    """The full path with the float tracker (stage A, field, Minimizer_RV<float>, matching, EKF, rescaling, pose) over 24 frames, three
    sequences, against the reference with ITS float tracker on the same frames.

    (i) Teacher-forced (oracle/teacher.py: the reference's state injected before every frame): EVERY frame of every sequence within
    2e-5 |X| + 2e-8 of the float reference (observed: <= 4e-6, i.e. a few float ulps through six solves) with identical KeyLine,
    match and EstimationOK counts.  This is the parity statement: given the same input, the device's float tracker is the reference's.
    (ii) Free-running, a batch of three: a float trajectory is a chain of decisions (which LM step is accepted, which initialisation
    chain wins) fed by float sums, and two correct float implementations that add in different orders part ways at the first decision
    that hangs on the sum's last bits — the reference's own float and double instantiations part on these very sequences
    (tools/experiments/exp_f32_sequence.py: sequence 0, frames 14-16).  So: inside 1e-4 |X| on every frame up to a sequence's first
    departure, at least two of the three sequences inside it to the end, every frame EstimationOK, KeyLine counts equal throughout
    (the detector does not depend on the tracker's precision)."""
    oracle = require_ref()
    from oracle import teacher
    w, h, n, B = 376, 240, 24, 3
    frames = [f for f, _, _ in synth.billboard_sequence(w, h, n + B)]
    for s in range(B):
        orc = oracle.Oracle("ref", oracle.euroc_params(w, h))
        orc.set_tracker_f32(1)
        e1 = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=1, nslots=3)
        e1.set_tracker_precision(32)
        tf = teacher.teacher_forced_replay(e1, orc, lambda k, s=s: frames[k + s], n, tol_rel=2e-5, tol_abs=2e-8)
        e1.close()
        orc.close()
        assert tf["outside_tolerance"] == [], (s, tf["outside_tolerance"][:3])
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=B, nslots=3)
    eh.set_tracker_precision(32)
    eh.set_nav_log(n)
    for k in range(n):
        eh.upload_rgb(eh.next_slot(), np.stack([frames[k + s] for s in range(B)]))
        eh.process_frame(np.full(B, 0.05 * k))
    log = eh.read_nav_log_array(0, n)
    eh.close()
    stayed = 0
    for s in range(B):
        orc = oracle.Oracle("ref", oracle.euroc_params(w, h))
        orc.set_tracker_f32(1)
        departed = None
        for k in range(n):
            _, nr = orc.process_frame(frames[k + s], 0.05 * k)
            g = log[k, s]
            if k == 0:
                assert int(g["kn"]) == nr.kn
                continue
            assert int(g["estimation_ok"]) == 1 and nr.estimation_ok == 1, (s, k)
            Xg, Xr = np.r_[g["V"], g["W"]], np.r_[np.array(nr.V[:]), np.array(nr.W[:])]
            inside = np.max(np.abs(Xg - Xr)) <= 1e-4 * np.linalg.norm(Xr) + 1e-7
            if departed is None and not inside:
                departed = k
            if departed is None:
                assert int(g["kn"]) == nr.kn and abs(int(g["klm_num"]) - nr.klm_num) <= 2, (s, k)
        orc.close()
        stayed += departed is None
        print(f"sequence {s}: first frame outside 1e-4 |X| of the float reference: {departed}")
    assert stayed >= 2


def test_precision_switch_rules():
    eh = edgehip.EdgeHip(edgehip.euroc_params(376, 240), nseq=1, nslots=3)
    import ctypes as C
    assert eh.lib.edgehip_set_tracker_precision(eh.ctx, 16) != 0
    eh.imu_enable(edgehip.euroc_imu_params())
    assert eh.lib.edgehip_set_tracker_precision(eh.ctx, 32) != 0      # Minimizer_RV<float> is the ImuMode 0 tracker
    assert eh.lib.edgehip_set_tracker_precision(eh.ctx, 64) == 0
    eh.close()
    # the reverse order: the float tracker first, then the IMU branch or a stereo rig — refused, and nothing changes
    eh = edgehip.EdgeHip(edgehip.euroc_params(376, 240, stereo_available=1), nseq=1, nslots=4)
    eh.set_tracker_precision(32)
    ip = edgehip.euroc_imu_params()
    assert eh.lib.edgehip_imu_enable(eh.ctx, C.byref(ip)) != 0
    assert b"float tracker" in eh.lib.edgehip_last_error()
    t, R = np.array([0.11, 0.0, 0.0]), np.eye(3).ravel().copy()
    dp = C.POINTER(C.c_double)
    assert eh.lib.edgehip_set_stereo_rig(eh.ctx, 3, t.ctypes.data_as(dp), R.ctypes.data_as(dp), C.c_double(100.0)) != 0
    assert b"float tracker" in eh.lib.edgehip_last_error()
    assert eh.lib.edgehip_set_tracker_precision(eh.ctx, 32) == 0       # still neither IMU nor rig: 32 stays legal
    eh.set_tracker_precision(64)                                       # back to 64 bits: both are accepted
    eh.set_stereo_rig(3, t, R)
    assert eh.lib.edgehip_set_tracker_precision(eh.ctx, 32) != 0
    eh.set_stereo_rig(-1)
    eh.imu_enable(ip)
    assert eh.lib.edgehip_set_tracker_precision(eh.ctx, 32) != 0
    eh.close()
