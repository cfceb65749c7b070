"""k_try_velrot, k_try_velrot2, k_try_vel and the LM steps against the reference on crafted KeyLine lists (GPU).

The lists are those of tests/tracker_crafted.py; what they reach in the reference — runs of unmatched KeyLines of 1, 63, 64, 65, 255, 256,
257 and 513 KeyLines from multiples of 256 and from odd offsets, a run from KeyLine 0, a tail, two match-free blocks, a list without a
match, every gate on its threshold, a new list that needs the 32-byte gather record, the exact grid — is asserted on the CPU, in
tests/test_tracker_crafted_cpu.py.

Single evaluations (edgehip_try_velrot, which stores m_id_f): pass 1 unweighted at X / 2 into residual buffer 1, pass 2 under test for
(reweight, procjf) in MODES reading buffer 1 and writing buffer 2.  Three different lists share every launch and the one in sequence 0
changes from launch to launch; the cuts come in the order 513, 1, full, 256, 255, 257, 511, 512 in ONE context per family, so that a short
list follows a long one and stale partials / block_last / resid_carry entries of the blocks it no longer has would show.  For every sequence,
against the reference on that sequence's list and request:
  m_id_f of every KeyLine equal; the residual memory bit-equal on every KeyLine the gate does not skip (include/edgehip.h promises it);
  |F - F_ref| <= 1e-13 |F_ref|; |d JtJ_ij| <= 1e-13 sqrt(JtJ_ii JtJ_jj) and |d JtF_i| <= 1e-13 sqrt(JtJ_ii F), scales from the reference:
  both sides add 2 048 to 16 000 products in log-depth trees, log2(n) 2^-53 sum|terms| <= 1.6e-15 of that Cauchy-Schwarz scale, so 1e-13
  leaves about 60 x; where the reference's scale is 0 the device's value must be exactly 0.  Nothing is excluded.
The Huber requests of family B put k_huber on |r0[i]| and on the doubles either side of it.  What that can show: every KeyLine whose first-pass
residual exceeds such a small k is weighted by k / |r|, and inside the carry run the device holds a marker where the reference holds the
inherited value — a weight taken from the marker instead of carry_in_prev moves the sums by percents.  What it cannot show: the weight of KeyLine i
itself on the threshold differs from 1 by 2^-53, far below any bound on a sum.

Minimisers (family A; full length and the 257 cut): Minimizer_RV with TrackerInitType 0, 1 and 2 in batches of three and once in a batch of 200 (the
size of test_whole_batch_vs_ref_gpu.py at 376 x 240, where the whole-batch launch chain runs); Minimizer_V with iter_max 0 and 3, two starts, a
min_mod that drops 698 KeyLines by n_m and a list with 360 KeyLines behind the camera.  Bounds: those of test_stage_b_gpu.py::test_minimizer_rv and
::test_minimizer_v; non-finite reference entries (a list without a match has J^T J = 0) must be non-finite on the device.  The reference's results
are stable on every one of these requests (test_tracker_crafted_cpu.py).  Seeds replaced: the start of Minimizer_RV on (`none`, cut 257) takes seed 1 — with
seed 0 the reference ends on a pose with one chance match and its covariance is 1e25 from one start and NaN from a start 1e-12 away (tracker_crafted.RV_SEED).
"""
import time

import numpy as np
import pytest

import tracker_crafted as tc
from helpers import require_ref, to_edgehip_kl
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu
NSEQ = 3
TOL = 1e-13
WHOLE_BATCH = 200


@pytest.fixture(scope="module")
def world():
    oracle = require_ref()
    fam = tc.family_a()
    w = dict(fam=fam, orc_b=tc.make_reference_b(oracle), eh={})
    try:
        w["eh"]["a"] = edgehip.EdgeHip(edgehip.euroc_params(tc.W_A, tc.H_A), nseq=NSEQ, nslots=2)
        w["eh"]["b"] = edgehip.EdgeHip(edgehip.euroc_params(tc.W_B, tc.H_B, max_points=tc.CAP_B, ppx=tc.PP_B[0], ppy=tc.PP_B[1], zfx=tc.ZF_B,
                                                            zfy=tc.ZF_B), nseq=NSEQ, nslots=2)
        w["eh"]["r"] = edgehip.EdgeHip(edgehip.euroc_params(tc.W_A, tc.H_A), nseq=1, nslots=2)
        upload_new_a(w["eh"]["a"], fam)
        yield w
    finally:
        for e in w["eh"].values():
            e.close()
        w["orc_b"].close()


def upload_new_a(eh, fam, new=None):
    for s in range(eh.nseq):
        eh.upload_keylines(s, 1, to_edgehip_kl(fam["new"] if new is None else new), fam["new_mask"], fam["new_retuned"])
    eh.build_field(1, tc.MAX_R, -1.0)


def compare_evaluation(bad, tag, got, ref, kl, gate, mnt, fc, procjf):
    """got = (F, JtJ, JtF, residual buffer 2, m_id_f) of one sequence; ref = the reference's pass 2."""
    F, JtJ, JtF, r, mid = got
    k = len(kl)
    if not np.array_equal(mid, ref["mid"]):
        i = np.nonzero(mid != ref["mid"])[0]
        bad.append(f"{tag}: m_id_f differs in {len(i)} KeyLines, first {i[:4]}: {mid[i[:4]]} vs {ref['mid'][i[:4]]}")
    ev = ~tc.gate_skips(kl, gate, mnt, fc)
    a, b = r[:k][ev], ref["r"][:k][ev]
    if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        i = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
        bad.append(f"{tag}: residual memory differs in {len(i)} KeyLines, first {np.nonzero(ev)[0][i[:4]]}: {a[i[:4]]} vs {b[i[:4]]}")
    if not abs(F - ref["F"]) <= TOL * abs(ref["F"]):
        bad.append(f"{tag}: F {F!r} vs {ref['F']!r}")
    if procjf:
        d = np.sqrt(np.abs(np.diag(ref["JtJ"])))
        sj, sf = TOL * np.outer(d, d), TOL * d * np.sqrt(abs(ref["F"]))
        if not np.all(np.abs(JtJ - ref["JtJ"]) <= sj):
            bad.append(f"{tag}: JtJ off by {np.max(np.abs(JtJ - ref['JtJ']) / np.where(sj > 0, sj / TOL, 1)):.2e} of its scale")
        if not np.all(np.abs(JtF - ref["JtF"]) <= sf):
            bad.append(f"{tag}: JtF off by {np.max(np.abs(JtF - ref['JtF']) / np.where(sf > 0, sf / TOL, 1)):.2e} of its scale")


def run_launch(bad, tag, eh, refs, X, gates, mnt, fcs, modes, k_huber=tc.K_HUBER):
    """One uploaded set of lists through both passes in every mode.  refs[s] = (reference context, slot_new, slot_old, list)."""
    X = np.asarray(X, np.float64)
    for s, fc in enumerate(fcs):
        eh.set_framecount(s, 1, fc)
    for rw, jf in modes:
        eh.try_velrot(1, 0, X * 0.5, False, True, tc.MATCH_THRESH, gates, mnt, k_huber, resid_in=-1, resid_out=1)
        F, JtJ, JtF = eh.try_velrot(1, 0, X, rw, jf, tc.MATCH_THRESH, gates, mnt, k_huber, resid_in=1, resid_out=2)
        r = eh.download_resid(2)
        for s, (orc, sn, so, kl, load) in enumerate(refs):
            load()
            orc.set_framecount(sn, fcs[s])
            _, p2 = tc.two_pass(orc, sn, so, X, gates[s], mnt, rw, jf, k_huber=k_huber)
            kg, _ = eh.download_keylines(s, 0, want_mask=False)
            compare_evaluation(bad, f"{tag} seq {s} rw={int(rw)} jf={int(jf)}", (F[s], JtJ[s], JtF[s], r[s], kg["m_id_f"]), p2, kl, gates[s], mnt,
                               fcs[s], jf)
            orc.set_framecount(sn, 0)


def ref_a(fam, name, n):
    kl, m = tc.cut(fam["variants"][name], fam["old_mask"], n)
    return (fam["orc"], fam["sn"], fam["so"], kl, lambda: fam["orc"].set_keylines(fam["so"], kl, m, fam["old_retuned"])), m


def report(bad, t0, what):
    print(f"{what}: {time.perf_counter() - t0:.1f} s, {len(bad)} mismatches")
    assert not bad, f"{len(bad)} mismatches, first:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_runs_of_unmatched_keylines(world, pose):
    """runs, head, tail, hole, none and the donor itself: every cut, all four modes, X = 0 / the donor's nav pose / a seeded small pose."""
    fam, eh = world["fam"], world["eh"]["a"]
    bad, t0 = [], time.perf_counter()
    gates = np.full(NSEQ, fam["gate"])
    for n, names in tc.jobs_a():
        refs = []
        for s, name in enumerate(names):
            ref, m = ref_a(fam, name, n)
            eh.upload_keylines(s, 0, to_edgehip_kl(ref[3]), m, fam["old_retuned"])
            refs.append(ref)
        run_launch(bad, f"pose {pose} cut {n} {names}", eh, refs, fam["poses"][pose], gates, 0, [0] * NSEQ, tc.MODES)
    report(bad, t0, f"runs, pose {pose}")


@pytest.mark.parametrize("pose", [0, 1, 2])
def test_gates_on_their_thresholds(world, pose):
    """s_rho on the gate and either side; m_num -1 .. 3 against min(MatchNumThresh = 2, FrameCount) with FrameCount 0, 1 and 5 in the three
    sequences of one launch (which sequence has which rotates)."""
    fam, eh = world["fam"], world["eh"]["a"]
    bad, t0 = [], time.perf_counter()
    gates = np.full(NSEQ, fam["gate"])
    for k, n in enumerate(tc.CUTS):
        ref, m = ref_a(fam, "gates", n)
        for s in range(NSEQ):
            eh.upload_keylines(s, 0, to_edgehip_kl(ref[3]), m, fam["old_retuned"])
        fcs = [tc.GATES_FC[(s + k) % 3] for s in range(NSEQ)]
        run_launch(bad, f"pose {pose} cut {n} gates FrameCount {fcs}", eh, [ref] * NSEQ, fam["poses"][pose], gates, tc.GATES_MNT, fcs, tc.MODES)
    report(bad, t0, f"gates, pose {pose}")


def test_the_upload_chooses_the_gather_record(world):
    """One sequence: the new list with one u_m[0] a float ulp off (edgehip_upload_keylines must fall back to the 32-byte record with the stored
    u_m, which is what the reference reads), then the same list unedited (back to the 16-byte record), then the edited one again."""
    fam, eh = world["fam"], world["eh"]["r"]
    orc, sn = fam["orc"], fam["sn"]
    bad, t0 = [], time.perf_counter()
    gates = np.full(1, fam["gate"])
    try:
        for which, new in (("record", fam["record"]["new"]), ("plain", fam["new"]), ("record again", fam["record"]["new"])):
            upload_new_a(eh, fam, new)
            orc.set_keylines(sn, new, fam["new_mask"], fam["new_retuned"])
            orc.build_field(sn, tc.MAX_R, fam["new_retuned"])
            for n in tc.CUTS:
                ref, m = ref_a(fam, "plain", n)
                eh.upload_keylines(0, 0, to_edgehip_kl(ref[3]), m, fam["old_retuned"])
                for pose in range(3):
                    run_launch(bad, f"{which} pose {pose} cut {n}", eh, [ref], fam["poses"][pose], gates, 0, [0], tc.MODES)
    finally:
        orc.set_keylines(sn, fam["new"], fam["new_mask"], fam["new_retuned"])
        orc.build_field(sn, tc.MAX_R, fam["new_retuned"])
    report(bad, t0, "gather record")


def test_exact_grid(world):
    """Family B at X = 0: the image border with p + 0.5 an integer on both sides of each limit, Test_f_k on its threshold, empty field entries
    against entries that fail the test, KeyLines behind the camera, a carry over two block boundaries; then the Huber requests."""
    eh, orc = world["eh"]["b"], world["orc_b"]
    fams = [tc.family_b(s) for s in range(3)]
    bad, t0 = [], time.perf_counter()
    gates = np.full(NSEQ, tc.GATE_B)
    for s in range(NSEQ):
        eh.upload_keylines(s, 1, to_edgehip_kl(fams[0]["new"]), fams[0]["new_mask"], 0.0)
    eh.build_field(1, tc.MAX_R_B, 0.0)

    def launch(k, n, modes, k_huber, tag):
        refs = []
        for s in range(NSEQ):
            f = fams[(s + k) % 3]
            kl, m = tc.cut(f["old"], f["old_mask"], n)
            eh.upload_keylines(s, 0, to_edgehip_kl(kl), m, 0.0)
            refs.append((orc, 1, 0, kl, lambda f=f, n=n: tc.load_b(orc, f, n)))
        run_launch(bad, tag, eh, refs, np.zeros(6), gates, 0, [0] * NSEQ, modes, k_huber)

    for k, n in enumerate(tc.CUTS):
        launch(k, n, tc.MODES, tc.K_HUBER, f"grid cut {n}")
    for k, (kh, i, kind) in enumerate(tc.huber_requests(orc, fams[0])):
        launch(k, None, ((True, True), (True, False)), kh, f"grid k_huber {kh!r} ({kind} residual of KeyLine {i})")
    report(bad, t0, "exact grid")


def _set_start(eh, s, start, gate, fc):
    st = eh.get_state(s)
    st.V[:], st.W[:] = list(start[:3]), list(start[3:])
    st.s_rho_q = gate
    eh.set_state(s, st)
    eh.set_framecount(s, 1, fc)


def _compare_rv(bad, tag, eh, s, ref):
    g = eh.get_state(s)
    got = dict(V=np.array(g.V[:]), W=np.array(g.W[:]), RVel=np.array(g.P_V[:]).reshape(3, 3), RW0=np.array(g.P_W[:]).reshape(3, 3), F=g.score)
    bad += [f"{tag}: {b}" for b in tc.rv_agree(got, ref)]
    kg, _ = eh.download_keylines(s, 0, want_mask=False)
    if not np.array_equal(kg["m_id_f"], ref["mid"]):
        bad.append(f"{tag}: m_id_f differs in {(kg['m_id_f'] != ref['mid']).sum()} KeyLines")
    if eh.get_framecount(s, 1) != ref["fc"]:
        bad.append(f"{tag}: FrameCount {eh.get_framecount(s, 1)} vs {ref['fc']}")


@pytest.mark.parametrize("init_type", [0, 1, 2])
def test_minimizer_rv(world, init_type):
    """Minimizer_RV on runs, head, hole, none and gates (FrameCount 1 and 5, MatchNumThresh 2), full length and the 257 cut, three per launch."""
    fam = world["fam"]
    bad, t0 = [], time.perf_counter()
    eh = edgehip.EdgeHip(edgehip.euroc_params(tc.W_A, tc.H_A, tracker_init_type=init_type, match_num_thresh=tc.GATES_MNT), nseq=NSEQ, nslots=2)
    try:
        upload_new_a(eh, fam)
        jobs = tc.rv_jobs()
        for k0 in range(0, len(jobs), NSEQ):
            starts = []
            for s, job in enumerate(jobs[k0:k0 + NSEQ]):
                kl, m = tc.cut(fam["variants"][job[0]], fam["old_mask"], job[2])
                eh.upload_keylines(s, 0, to_edgehip_kl(kl), m, fam["old_retuned"])
                starts.append(tc.rv_start(fam, job, k0 + s))
                _set_start(eh, s, starts[s], fam["gate"], job[1])
            eh.minimizer_rv(1, 0)
            for s, job in enumerate(jobs[k0:k0 + NSEQ]):
                _compare_rv(bad, f"init {init_type} {job} seq {s}", eh, s, tc.ref_minimizer_rv(fam, job, starts[s], init_type))
    finally:
        eh.close()
    report(bad, t0, f"Minimizer_RV, TrackerInitType {init_type}")


def test_minimizer_rv_whole_batch(world):
    """`runs` and `hole`, full and cut to 257, two starts each, dealt round-robin over a batch of 200: the whole-batch launch chain
    (k_try_velrot2 / k_lm_step2 with a carry per chain, the LM step's carry resolution over up to 34 blocks)."""
    fam = world["fam"]
    bad, t0 = [], time.perf_counter()
    combos = [(("runs", 0, None), 0), (("hole", 0, None), 1), (("runs", 0, 257), 2), (("hole", 0, 257), 3),
              (("runs", 0, None), 4), (("hole", 0, None), 5), (("runs", 0, 257), 6), (("hole", 0, 257), 7)]
    eh = edgehip.EdgeHip(edgehip.euroc_params(tc.W_A, tc.H_A), nseq=WHOLE_BATCH, nslots=2)
    try:
        upload_new_a(eh, fam)
        cuts = {job: tc.cut(fam["variants"][job[0]], fam["old_mask"], job[2]) for job, _ in combos}
        for s in range(WHOLE_BATCH):
            job, k = combos[s % len(combos)]
            eh.upload_keylines(s, 0, to_edgehip_kl(cuts[job][0]), cuts[job][1], fam["old_retuned"])
            _set_start(eh, s, tc.rv_start(fam, job, 100 + k), fam["gate"], 0)
        eh.minimizer_rv(1, 0)
        refs = [tc.ref_minimizer_rv(fam, job, tc.rv_start(fam, job, 100 + k), 2) for job, k in combos]
        for (job, k), a in zip(combos, refs):                     # (the reference's own stability on these starts)
            assert tc.rv_agree(tc.ref_minimizer_rv(fam, job, tc.rv_start(fam, job, 100 + k) + 1e-12, 2), a, 0.1) == [], job
        for s in range(WHOLE_BATCH):
            _compare_rv(bad, f"whole batch {combos[s % len(combos)][0]} seq {s}", eh, s, refs[s % len(combos)])
    finally:
        eh.close()
    report(bad, t0, f"Minimizer_RV, batch of {WHOLE_BATCH}")


def test_minimizer_v(world):
    """Minimizer_V (k_try_vel: fabs(fi), the in-place residual buffer, resolved / rkeep) on runs, head, hole, none, gates and `behind`."""
    fam, eh = world["fam"], world["eh"]["a"]
    bad, t0 = [], time.perf_counter()
    upload_new_a(eh, fam)
    jobs = tc.v_jobs()
    gates = np.full(NSEQ, fam["gate"])
    for k0 in range(0, len(jobs), NSEQ):
        grp = jobs[k0:k0 + NSEQ]
        for s, job in enumerate(grp):
            kl, m = tc.cut(fam["variants"][job[0]], fam["old_mask"], job[2])
            eh.upload_keylines(s, 0, to_edgehip_kl(kl), m, fam["old_retuned"])
        for iter_max, min_mod in tc.V_REQUESTS:
            for V0 in tc.V_STARTS:
                for s, job in enumerate(grp):
                    eh.set_framecount(s, 1, job[1])
                V, RV, F = eh.minimizer_v(1, 0, V0, gates, -1.0 if min_mod is None else min_mod, tc.MATCH_THRESH, iter_max, tc.GATES_MNT, tc.K_HUBER)
                for s, job in enumerate(grp):
                    ref = tc.ref_minimizer_v(fam, job, np.array(V0), iter_max, min_mod)
                    tag = f"Minimizer_V {job} seq {s} iter_max {iter_max} min_mod {min_mod} V0 {V0}"
                    bad += [f"{tag}: {b}" for b in tc.v_agree(dict(V=V[s], RVel=RV[s], F=F[s]), ref)]
                    kg, _ = eh.download_keylines(s, 0, want_mask=False)
                    if not np.array_equal(kg["m_id_f"], ref["mid"]):
                        bad.append(f"{tag}: m_id_f differs in {(kg['m_id_f'] != ref['mid']).sum()} KeyLines")
    for s in range(NSEQ):
        eh.set_framecount(s, 1, 0)
    report(bad, t0, "Minimizer_V")
