"""k_quantile<1024> / k_quantile<256>, the detector's retune (k_retune and the last wave of k_quantile) and k_ext_rotvel with the 6x6 solve of
edgehip_ext_rot_vel against the reference on crafted inputs (GPU).

The inputs are those of tests/stats_crafted.py; what they reach in the reference — the bin of every special s_rho, lists exactly on and one
KeyLine past pct * kn, the first and last KeyLine of every 4 * NT stride decisive, the retune walk landing on, one past and never at TrackPoints,
a single row that holds the rank of ExtRotVel's system at KeyLine 0 / the last KeyLine / a block boundary, the pole, lists without a match —
is asserted on the CPU, in tests/test_stats_crafted_cpu.py, together with the named defects each comparison catches.

Quantile: s_rho_q of every sequence == the reference's, for every nbins in (1, 4, 5, 100, 255, 256) and pct in (0, 0.5, 0.9, 1).  Three different lists
per launch in a 3-sequence context (k_quantile<1024>), rotated so that sequence 0 holds another list every time, lengths 1 .. 8193 and 0 in an order in which
a short list follows a long one in the same slot; 65 lists of lengths 1025, 1, 1024, 1023 per launch in a 65-sequence context (k_quantile<256>).
Retune (QCutOffNumBins 100 and 256): for every crafted TrackPoints one context pair: upload_rgb + stage_a (k_retune) and process_frame without overlap (frame 2 retunes in k_quantile's last
wave); reTunedThresh equal as float32 bits to the reference's and between the two paths.  A uniform grey frame (kn = 0) gives 0.f on both paths — a claim about the
device alone: the reference reads an uninitialised KeyLine there (tests/test_stage_a_gpu.py).
ExtRotVel: stats_crafted.erv_agree — ok equal; |dWx_ij| <= n_rows 2^-52 sqrt(Wx_ii Wx_jj), the worst case of two summation orders over n_rows products
(Cauchy-Schwarz; derived, not measured), exactly 0 where the scale is 0; X and Rx within cond (n_rows 2^-52 + 1e-11) of their largest entry, cond over the
singular values the reference keeps; non-finite where the reference's entry is.  Nothing is excluded.
"""
import ctypes as C
import time

import numpy as np
import pytest

import stats_crafted as sc
from helpers import require_ref, to_edgehip_kl
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu
NSEQ = 3
NSEQ_256 = 65                                          # nseq > 64 selects k_quantile<256>
COMBOS = [(n, pct) for n in sc.Q_NBINS for pct in sc.Q_PCTS]


@pytest.fixture(scope="module")
def world():
    oracle = require_ref()
    w = dict(oracle=oracle, ref=oracle.Oracle("ref", sc.params(oracle), nslots=2), eh={})
    try:
        w["eh"][NSEQ] = edgehip.EdgeHip(sc.params(edgehip), nseq=NSEQ, nslots=2)
        yield w
    finally:
        for e in w["eh"].values():
            e.close()
        w["ref"].close()


def report(bad, t0, what):
    print(f"{what}: {time.perf_counter() - t0:.1f} s, {len(bad)} mismatches")
    assert not bad, f"{len(bad)} mismatches, first:\n" + "\n".join(bad[:12])


def _bits(v):
    return np.float32(v).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# EstimateQuantile
# ---------------------------------------------------------------------------------------------------------------------------------
def _reference_answers(ref, cases):
    """{case name: {(nbins, pct): s_rho_q}} — computed once, shared by both contexts."""
    out = {}
    for name, s in cases:
        ref.set_keylines(0, sc.quantile_keylines(s))
        out[name] = {(n, pct): ref.quantile(0, sc.SMIN, sc.SMAX, pct, n) for n, pct in COMBOS}
    return out


def _quantile_launch(bad, tag, eh, lists, want):
    """lists[s] = (name, s_rho) of sequence s: upload, then every (nbins, pct)."""
    for s, (name, srho) in enumerate(lists):
        eh.upload_keylines(s, 0, to_edgehip_kl(sc.quantile_keylines(srho)), None, 0.0)
    for n, pct in COMBOS:
        eh.quantile(0, sc.SMIN, sc.SMAX, pct, n)
        for s, (name, srho) in enumerate(lists):
            got = eh.get_state(s).s_rho_q
            if not got == want[name][(n, pct)]:
                bad.append(f"{tag} seq {s} [{name}] nbins {n} pct {pct}: {got!r} vs {want[name][(n, pct)]!r}")


@pytest.fixture(scope="module")
def quantile_world(world):
    cases = sc.quantile_cases()
    return cases, _reference_answers(world["ref"], cases)


def test_quantile_three_sequences(world, quantile_world):
    cases, want = quantile_world
    eh = world["eh"][NSEQ]
    bad, t0 = [], time.perf_counter()
    for k, g in enumerate(range(0, len(cases), NSEQ)):
        grp = [cases[(g + j) % len(cases)] for j in range(NSEQ)]
        r = k % NSEQ
        _quantile_launch(bad, f"launch {k}", eh, grp[r:] + grp[:r], want)
    report(bad, t0, f"quantile, {NSEQ} sequences, {len(cases)} lists x {len(COMBOS)} (nbins, pct)")


def test_quantile_whole_batch_kernel(world, quantile_world):
    """65 sequences: k_quantile<256>, whose 4 * NT stride is 1024.  Sequence s of launch k holds a list of length Q_CUTS_256[(s + k) % 4]."""
    cases, want = quantile_world
    by_len = {L: [c for c in cases if len(c[1]) == L] for L in sc.Q_CUTS_256}
    bad, t0 = [], time.perf_counter()
    eh = edgehip.EdgeHip(sc.params(edgehip), nseq=NSEQ_256, nslots=2)
    try:
        for k in range(len(sc.Q_CUTS_256)):
            lists = []
            for s in range(NSEQ_256):
                pool = by_len[sc.Q_CUTS_256[(s + k) % len(sc.Q_CUTS_256)]]
                lists.append(pool[(s // len(sc.Q_CUTS_256) + 3 * k) % len(pool)])
            _quantile_launch(bad, f"launch {k}", eh, lists, want)
    finally:
        eh.close()
    report(bad, t0, f"quantile, {NSEQ_256} sequences")


def test_quantile_refuses_nbins_out_of_range(world, quantile_world):
    cases, want = quantile_world
    eh = world["eh"][NSEQ]
    grp = cases[:NSEQ]
    bad = []
    _quantile_launch(bad, "before", eh, grp, want)
    assert not bad, bad
    before = [eh.get_state(s).s_rho_q for s in range(NSEQ)]
    for nbins in (0, 257):
        rc = eh.lib.edgehip_quantile(eh.ctx, 0, C.c_double(sc.SMIN), C.c_double(sc.SMAX), C.c_double(0.5), nbins)
        assert rc == -1, (nbins, rc)                                   # EDGEHIP_ERR_ARG
        assert [eh.get_state(s).s_rho_q for s in range(NSEQ)] == before
    eh.quantile(0, sc.SMIN, sc.SMAX, 0.5, 256)                          # and the context goes on
    assert eh.get_state(0).s_rho_q == want[grp[0][0]][(256, 0.5)]


# ---------------------------------------------------------------------------------------------------------------------------------
# reEstimateThresh
# ---------------------------------------------------------------------------------------------------------------------------------
def _retuned(eh):
    return [eh.get_state(s).retuned_thresh for s in range(eh.nseq)]


@pytest.mark.parametrize("nbins", sc.RT_NBINS)
def test_retune_on_and_past_track_points(world, monkeypatch, nbins):
    oracle = world["oracle"]
    pairs = sc.retune_frames(NSEQ)
    f1, f2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    grey = np.full_like(f1, 90)
    bad, t0 = [], time.perf_counter()
    values = set()
    for p in pairs:                                                     # the histogram of the frame whose retune runs in k_quantile
        o = oracle.Oracle("ref", sc.retune_params(oracle, 12000, nbins), nslots=2)
        o.stage_a(0, p[1], o.p.detector_thresh, 0)
        values |= set(sc.retune_track_points(sc.modulus_histogram(o.keylines(0)["n_m"], nbins)[0]))
        o.close()
    monkeypatch.setenv("EDGEHIP_OVERLAP", "0")                          # one stream: the driver defers frame 2's retune to k_quantile
    for v in sorted(values):
        want_a, want_b = [], []
        for p in pairs:
            a = oracle.Oracle("ref", sc.retune_params(oracle, v, nbins), nslots=2)
            b = oracle.Oracle("ref", sc.retune_params(oracle, v, nbins), nslots=8)
            wa = []
            for k, f in enumerate(p):
                a.stage_a(k, f, a.p.detector_thresh, 0)
                wa.append(a.retuned(k))
                _, nav = b.process_frame(f, 0.05 * k)
            want_a.append(wa)
            want_b.append(nav.retuned_thresh)
            a.close()
            b.close()
        ea = edgehip.EdgeHip(sc.retune_params(edgehip, v, nbins), nseq=NSEQ, nslots=3)
        eb = edgehip.EdgeHip(sc.retune_params(edgehip, v, nbins), nseq=NSEQ, nslots=3)
        try:
            got_a = []
            for k, f in enumerate((f1, f2, grey, f2)):
                ea.upload_rgb(k % 3, f)
                ea.stage_a(k % 3)
                got_a.append(_retuned(ea))
                eb.upload_rgb(eb.next_slot(), f)
                eb.process_frame(0.05 * k)
                got_b = _retuned(eb)
                for s in range(NSEQ):
                    tag = f"TrackPoints {v} seq {s} frame {k}"
                    if k < 2 and _bits(got_a[k][s]) != _bits(want_a[s][k]):
                        bad.append(f"{tag}: stage_a {got_a[k][s]!r} vs {want_a[s][k]!r}")
                    if k == 1 and _bits(got_b[s]) != _bits(want_b[s]):
                        bad.append(f"{tag}: process_frame {got_b[s]!r} vs {want_b[s]!r}")
                    if k == 2 and not (_bits(got_a[k][s]) == _bits(got_b[s]) == _bits(0.0)):
                        bad.append(f"{tag} (grey, kn = 0): {got_a[k][s]!r}, {got_b[s]!r}, both must be 0.f")
                    if k == 3 and _bits(got_a[k][s]) != _bits(want_a[s][1]):
                        bad.append(f"{tag} (after the grey frame): stage_a {got_a[k][s]!r} vs {want_a[s][1]!r}")
                    if _bits(got_a[k][s]) != _bits(got_b[s]):
                        bad.append(f"{tag}: stage_a {got_a[k][s]!r} vs process_frame {got_b[s]!r}")
            assert list(ea.get_kn(2)) == [0] * NSEQ
        finally:
            ea.close()
            eb.close()
    report(bad, t0, f"retune, {nbins} bins, TrackPoints {sorted(values)}")


# ---------------------------------------------------------------------------------------------------------------------------------
# ExtRotVel
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ext_rot_vel(world):
    eh, ref = world["eh"][NSEQ], world["ref"]
    bad, t0, n_lists = [], time.perf_counter(), 0
    for k, (cut, names, vels) in enumerate(sc.erv_jobs(NSEQ)):
        lists = [sc.erv_list(name, cut, vel) for name, vel in zip(names, vels)]
        for s, kl in enumerate(lists):
            eh.upload_keylines(s, 1, to_edgehip_kl(kl), None, 0.0)
        X, Wx, Rx, ok = eh.ext_rot_vel(1, np.array(vels), sc.LOC_UNC, sc.HUB)
        for s, kl in enumerate(lists):
            ref.set_keylines(0, kl)
            want = ref.ext_rot_vel(0, vels[s], sc.LOC_UNC, sc.HUB)
            n_rows = int((kl["m_id"] >= 0).sum())
            got = dict(ok=bool(ok[s]), X=X[s], Wx=Wx[s], Rx=Rx[s])
            bad += [f"launch {k} seq {s} [{names[s]}, {len(kl)} KeyLines, vel {vels[s]}]: {b}" for b in sc.erv_agree(got, want, n_rows)]
            n_lists += 1
    report(bad, t0, f"ExtRotVel, {n_lists} lists")
