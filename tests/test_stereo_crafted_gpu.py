"""k_stereo_match and k_fuse_stereo against the reference on crafted KeyLine lists (GPU).

The lists are those of tests/stereo_crafted.py; what they reach in the reference — which class takes which branch and ends how — is asserted
on the CPU, in tests/test_stereo_crafted_cpu.py.  In short: NaN and infinite depth bounds (std::max / std::min pass a NaN first argument
on, edge_tracker.cpp:474-475), bounds exactly on RHO_MIN / RHO_MAX and on the two doubles either side of each, the no-displacement branch with finite,
infinite and NaN directions, pair KeyLines in row 0 and column 0 of the mask that only a probe with a NaN coordinate turned into 0 would
find (Image::GetIndexRC, image.h:121-126), a pole and a negative depth in the pair camera, the "exactly one candidate" rule at
loc_unc^2 and the float above it, both gates exactly on their thresholds and one float either side, the walk's first and last step and
one beyond each, walks leaving through each side of the image with coordinates exactly -0.5, w - 0.5 and h - 0.5, rho < 0, +-0.0,
div = 0, and a per-KeyLine sentinel (NaN payloads included) in stereo_rho / stereo_s_rho that an unmatched or ambiguous KeyLine must keep.

One context of three sequences, stereo_available = 1, 160 x 120, max_points = 2048.  Three different lists share every launch — lengths
0, 1, 63, 64, 65, 255, 256, 257, 1025 (upload_keylines accepts kn = 0, so the empty list is in), a different class mix and pair-list
variant per sequence, the mix in sequence 0 rotating from launch to launch — so a slip between the per-sequence slices shows as a
neighbour's ids.  Under each of the five rigs, against the reference:

  stereo_m_id of every KeyLine and the per-sequence count: exact; directed_matching_stereo is called twice on the same upload and the
  second count must equal the first (the counter is cleared per call);
  stereo_rho / stereo_s_rho: the uploaded bytes where the reference left them alone, else rtol 1e-12, atol 0, NaN equal to NaN, an
  infinity equal only to the same infinity (the bound of test_stereo_matches_reference);
  after fuse_stereo_depth — from the device's own post-match state, and from the reference's post-match state with the crafted fusion
  states (s_rho 0 / inf / NaN, stereo_s_rho inf / 1e-300, stereo_rho inf, on matched and unmatched KeyLines alike) — rho0 / s_rho0
  bit-equal, rho / s_rho rtol 1e-13, atol 0, NaN equal to NaN, and the bytes of rho / s_rho of a KeyLine without a match.

Then the detector lists of test_stereo_gpu.make_data() at 376 x 240 with 600 edited main KeyLines (rho NaN, rho = s_rho = inf, s_rho
NaN), once.  Nothing is excluded from any comparison; failures are collected and reported together.
"""
import time

import numpy as np
import pytest

import stereo_crafted as sc
from helpers import require_ref, to_edgehip_kl
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu
NSEQ = 3


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def match_mismatches(got, want, uploaded):
    """stereo_m_id exact; stereo_rho / stereo_s_rho: the uploaded bytes where the reference kept them, else rtol 1e-12."""
    if len(got) != len(want):
        return [f"list length {len(got)} vs {len(want)}"]
    bad = []
    if not np.array_equal(got["stereo_m_id"], want["stereo_m_id"]):
        i = np.nonzero(got["stereo_m_id"] != want["stereo_m_id"])[0]
        bad.append(f"stereo_m_id: {len(i)} differ, first {i[:6]}: {got['stereo_m_id'][i[:6]]} vs {want['stereo_m_id'][i[:6]]}")
    for f in ("stereo_rho", "stereo_s_rho"):
        kept = _bits(want[f]) == _bits(uploaded[f])
        ok = np.where(kept, _bits(got[f]) == _bits(want[f]), np.isclose(got[f], want[f], rtol=1e-12, atol=0, equal_nan=True))
        if not ok.all():
            i = np.nonzero(~ok)[0]
            bad.append(f"KeyLine.{f}: {len(i)} differ ({int((~ok & kept).sum())} of them lost the uploaded bytes), first {i[:4]}: {got[f][i[:4]]} vs {want[f][i[:4]]}")
    return bad


def fuse_mismatches(got, want, start):
    if len(got) != len(want):
        return [f"list length {len(got)} vs {len(want)}"]
    bad = []
    for f in ("rho0", "s_rho0"):
        if _bits(got[f]).tobytes() != _bits(want[f]).tobytes():
            bad.append(f"KeyLine.{f}: {int((_bits(got[f]) != _bits(want[f])).sum())} differ in bits")
    un = start["stereo_m_id"] < 0
    for f in ("rho", "s_rho"):
        ok = np.isclose(got[f], want[f], rtol=1e-13, atol=0, equal_nan=True)
        ok &= ~un | (_bits(got[f]) == _bits(start[f]))
        if not ok.all():
            i = np.nonzero(~ok)[0]
            bad.append(f"KeyLine.{f}: {len(i)} differ, first {i[:4]}: {got[f][i[:4]]} vs {want[f][i[:4]]}")
    return bad


def test_crafted_lists_follow_the_reference_under_every_rig():
    t_start = time.perf_counter()
    oracle = require_ref()
    orc = sc.make_reference(oracle)
    bad, launches, lists, eh = [], 0, 0, None
    pairs = [sc.pair_list(v) for v in (0, 1)]
    try:
        eh = edgehip.EdgeHip(edgehip.euroc_params(sc.W, sc.H, max_points=sc.CAP, stereo_available=1, ppx=sc.PP1[0], ppy=sc.PP1[1], zfx=sc.ZF, zfy=sc.ZF),
                             nseq=NSEQ, nslots=3)
        for slot in (0, 1):
            eh.set_slot_camera(slot, sc.PP1[0], sc.PP1[1], sc.ZF, sc.ZF)
        for ri, rig in enumerate(sc.RIGS):
            js = sc.jobs(ri)
            args = sc.args_tuple(rig)
            for k0 in range(0, len(js), NSEQ):
                case = js[k0:k0 + NSEQ]
                up, want, n_ref = [], [], []
                for s, (n, rot, v) in enumerate(case):
                    kl, _ = sc.main_list(n, rot)
                    pair, mask, _ = pairs[v]
                    w_, n_ = sc.reference_match(orc, kl, pair, mask, rig)
                    up.append(kl); want.append(w_); n_ref.append(n_)
                    eh.upload_keylines(s, 0, to_edgehip_kl(kl))
                    eh.upload_keylines(s, 1, to_edgehip_kl(pair), mask)
                    lists += 1
                n1 = eh.directed_matching_stereo(0, 1, *args)
                n2 = eh.directed_matching_stereo(0, 1, *args)
                launches += 2
                tags = [f"{rig}: sequence {s} ({n} KeyLines, mix {rot}, pair variant {v}): " for s, (n, rot, v) in enumerate(case)]
                if list(n1) != n_ref:
                    bad.append(f"{rig}: lengths {[c[0] for c in case]}: counts {list(n1)} vs {n_ref}")
                if list(n2) != list(n1):
                    bad.append(f"{rig}: lengths {[c[0] for c in case]}: the second call counts {list(n2)}, the first {list(n1)}")
                for s in range(NSEQ):
                    kg, _ = eh.download_keylines(s, 0, want_mask=False)
                    bad += [tags[s] + m for m in match_mismatches(kg, want[s], up[s])]
                # ---- fuse from the device's own post-match state ----
                eh.fuse_stereo_depth(0)
                launches += 1
                for s in range(NSEQ):
                    kg, _ = eh.download_keylines(s, 0, want_mask=False)
                    bad += [tags[s] + "fuse: " + m for m in fuse_mismatches(kg, sc.reference_fuse(orc, want[s]), want[s])]
                # ---- fuse from the reference's post-match state with the crafted states ----
                starts = [sc.fuse_states(want[s])[0] for s in range(NSEQ)]
                for s in range(NSEQ):
                    eh.upload_keylines(s, 0, to_edgehip_kl(starts[s]))
                eh.fuse_stereo_depth(0)
                launches += 1
                for s in range(NSEQ):
                    kg, _ = eh.download_keylines(s, 0, want_mask=False)
                    bad += [tags[s] + "fuse (crafted states): " + m for m in fuse_mismatches(kg, sc.reference_fuse(orc, starts[s]), starts[s])]
                    if kg["stereo_m_id"].tobytes() != starts[s]["stereo_m_id"].tobytes():
                        bad.append(tags[s] + "fuse changed stereo_m_id")
    finally:
        if eh is not None:
            eh.close()
        orc.close()
    print(f"crafted stereo lists: {len(sc.RIGS)} rigs, {lists} lists, {launches} launches of {NSEQ} sequences, {time.perf_counter() - t_start:.1f} s, {len(bad)} mismatches")
    assert not bad, f"{len(bad)} mismatches, first 25:\n" + "\n".join(bad[:25])


def test_detector_lists_with_nan_depth_bounds():
    """376 x 240, the detector's lists with 600 edited main KeyLines: none of the 600 may match, the rest as the reference."""
    oracle = require_ref()
    c = sc.detector_case(oracle)
    orc, s, ps = c["orc"], c["slot"], c["pair_slot"]
    pc = c["pair_cam"]
    bad, eh = [], None
    try:
        eh = edgehip.EdgeHip(edgehip.euroc_params(c["w"], c["h"], stereo_available=1), nseq=2, nslots=3)
        orc.set_keylines(ps, c["pair"], c["pair_mask"], c["pair_retuned"])
        orc.set_keylines(s, c["main"], c["main_mask"], c["main_retuned"])
        n_ref = orc.directed_matching_stereo(s, ps, *c["args"])
        want = orc.keylines(s).copy()
        for seq in range(2):
            eh.upload_keylines(seq, 0, to_edgehip_kl(c["main"]), c["main_mask"], c["main_retuned"])
            eh.upload_keylines(seq, 1, to_edgehip_kl(c["pair"]), c["pair_mask"], c["pair_retuned"])
        eh.set_slot_camera(1, pc["ppx"], pc["ppy"], pc["zfx"], pc["zfy"])
        n_gpu = eh.directed_matching_stereo(0, 1, *c["args"])
        assert np.all(want["stereo_m_id"][c["edited"]] == -1) and n_ref > 300
        if list(n_gpu) != [n_ref, n_ref]:
            bad.append(f"counts {list(n_gpu)} vs {n_ref}")
        for seq in range(2):
            kg, _ = eh.download_keylines(seq, 0, want_mask=False)
            bad += [f"sequence {seq}: " + m for m in match_mismatches(kg, want, c["main"])]
            hit = int((kg["stereo_m_id"][c["edited"]] >= 0).sum())
            if hit:
                by = {k: int((kg["stereo_m_id"][v] >= 0).sum()) for k, v in c["groups"].items()}
                bad.append(f"sequence {seq}: {hit} of the 600 KeyLines with NaN depth bounds matched: {by}")
        orc.fuse_stereo_depth(s)
        eh.fuse_stereo_depth(0)
        kg, _ = eh.download_keylines(1, 0, want_mask=False)
        bad += ["fuse: " + m for m in fuse_mismatches(kg, orc.keylines(s), want)]
    finally:
        if eh is not None:
            eh.close()
        orc.close()
    assert not bad, f"{len(bad)} mismatches:\n" + "\n".join(bad[:25])
