"""k_regularize, k_ekf and k_rescale<512,12,4> against the reference on crafted KeyLine lists (GPU).

The lists are those of helpers.crafted_mapping_lists (what they reach in the reference is asserted on the CPU, in
tests/test_mapping_crafted_cpu.py): an EKF variant (both clamps, the NaN / inf reset, n_m0 = 0, the prediction's pole 1 / rho + V[2] = 0,
rho = 0, NaN, s_rho = inf, values exactly at RHO_MAX and RHO_MIN, edited KeyLines without a match), a regularize variant (neighbours
with n_m = 0, one-sided, doubled and self neighbours, neighbour pairs exactly on the depth gate and one ulp either side, float alpha
exactly at thresh and its two float neighbours, alpha = 1, s_rho = 0 of a neighbour and of the KeyLine itself), a rescale variant
(s_rho0 = 0, < 0, -0.0, s_rho at 20 and its two neighbours, m_num = 0 and -1, in each of the kernel's three storage regions) and one in
which no KeyLine counts (tb = 0).  Each is cut to 1, 63, 64, 65, 1023, 1024, 1025, 12 287, 12 288, 12 289, 16 383, 16 384, 16 385
KeyLines and run whole: 376 x 240 with the default cap, 752 x 480 with max_points = 20 000, so that k_rescale's streamed region
(KeyLines from 16 384 on) runs and both region boundaries are a list's end.

One context of three sequences per resolution.  Three different lists share every launch and the variant in sequence 0 rotates from
launch to launch, so a slip between the per-sequence slices of the regularizer's scratch (seq * 2 * cap) shows as a neighbour's
values.  Every stage starts from the uploaded reference state:

  regularize          k_regularize alone, from the crafted list
  ekf_raw             k_ekf alone, from the crafted list (the edits reach the EKF as crafted)
  ekf                 k_ekf alone, from the reference's regularized list
  regularize_ekf      both
  rescale             k_rescale from the crafted list
  rescale_div         the same with do_rescaling = 1 (a second context: the switch is a creation parameter): rho, s_rho after the division
  rescale_after_ekf   k_rescale from the reference's regularized and updated list

Tolerances are the project's: rho, s_rho, rho0, s_rho0 of EVERY KeyLine rtol 1e-12, atol 0, NaN equal to NaN (test_stage_c_gpu.py, the
ragged-batch test); Kp and P_Kp 1e-10 relative, non-finite where the reference's is (the rescale's Newton reciprocal and summation
order).  Branch outcomes are sets: the KeyLines at RHO_MAX, at RHO_MIN, at (RhoInit, RHO_MAX) and NaN must be the reference's.  A
KeyLine without a match keeps the uploaded bits of all four fields through the EKF (of rho0 and s_rho0 where the regularizer ran first).
Nothing is excluded.

Two constructions are made so that a slip shows in rho and s_rho, the only thing read back here.  At alpha == thresh the neighbours'
weights are 0, so the centre KeyLines of "alpha on thresh" and "one float below" have s_rho = 0 themselves: regularized (alpha - thresh
< 0 is false, edge_tracker.cpp:117) is NaN, skipped keeps its bits.  And the EKF edits with an s_rho of 1e12 to 2e12 are chosen, with the
update's own arithmetic, where K * H rounds above 1 (edge_tracker.cpp:1024-1030): v_rho < 0, s_rho = NaN, rho finite and beyond a limit,
so the clamp arms must come before the NaN arm, and 1 - K * H must be rounded as written, not fused.
"""
import time

import numpy as np
import pytest

from rebvo_amd import edgehip
from helpers import (MAPPING_STAGES, crafted_mapping_lists, cut_list, depth_state_mismatches, mapping_lengths, mapping_stages, require_ref,
                     scalar_close, to_edgehip_kl)

pytestmark = pytest.mark.gpu

VARIANTS = ("ekf", "regularize", "rescale", "rescale_none")
NSEQ = 3


@pytest.fixture(scope="module")
def reference_sets():
    """One reference set-up per resolution for the module, made on first use."""
    require_ref()
    made = {}

    def get(w, h, cap):
        if (w, h, cap) not in made:
            made[(w, h, cap)] = crafted_mapping_lists(w, h, cap)
        return made[(w, h, cap)]

    yield get
    for c in made.values():
        c["orc"].close()


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("w,h,cap", [(376, 240, 16000), (752, 480, 20000)])
def test_crafted_lists_follow_the_reference_stage_by_stage(reference_sets, w, h, cap):
    t_start = time.perf_counter()
    c = reference_sets(w, h, cap)
    pose = (c["V"], c["RVel"], c["RW0"])
    jobs = [(v, n) for n in mapping_lengths(c["kn"]) for v in VARIANTS]        # neighbours in this order differ in variant
    assert c["kn"] <= cap and (w < 752 or c["kn"] > 16385)
    bad, launches = [], 0
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h, max_points=cap), nseq=NSEQ, nslots=2)
    eh_div = edgehip.EdgeHip(edgehip.euroc_params(w, h, max_points=cap, do_rescaling=1), nseq=NSEQ, nslots=2)
    try:
        for e in (eh, eh_div):
            for s in range(NSEQ):
                st = e.get_state(s)
                st.V[:] = c["V"]
                st.P_V[:] = c["RVel"].ravel()
                st.P_W[:] = c["RW0"].ravel()
                e.set_state(s, st)
        for k0 in range(0, len(jobs), NSEQ):
            case = [jobs[(k0 + s) % len(jobs)] for s in range(NSEQ)]              # (the last launch wraps round to the first lists)
            assert len({v for v, _ in case}) == NSEQ
            ref, masks = [], []
            for v, n in case:
                lst, mask = cut_list(c["variants"][v], c["mask"], n)
                ref.append(mapping_stages(c["orc"], c["slot"], lst, mask, c["retuned"], *pose))
                masks.append(mask)
            for stage in MAPPING_STAGES:
                dev = eh_div if stage == "rescale_div" else eh
                for s in range(NSEQ):
                    dev.upload_keylines(s, 1, to_edgehip_kl(ref[s][stage]["input"]), masks[s], c["retuned"])
                    if stage.startswith("rescale"):
                        st = dev.get_state(s)
                        st.Kp, st.P_Kp = -7.0, -7.0                               # what a launch that wrote nothing would leave
                        dev.set_state(s, st)
                if stage == "regularize":
                    dev.regularize_ekf(1, True, False)
                elif stage in ("ekf_raw", "ekf"):
                    dev.regularize_ekf(1, False, True)
                elif stage == "regularize_ekf":
                    dev.regularize_ekf(1)
                else:
                    dev.rescale(1)
                launches += 1
                for s in range(NSEQ):
                    want = ref[s][stage]
                    tag = f"{stage}: sequence {s} ({case[s][0]}, {case[s][1]} KeyLines): "
                    kg, _ = dev.download_keylines(s, 1, want_mask=False)
                    bad += [tag + m for m in depth_state_mismatches(kg, want["kl"])]
                    if len(kg) == len(want["kl"]) and "ekf" in stage:
                        un = want["input"]["m_id"] < 0
                        # (after a regularizer of its own rho and s_rho are computed values: a NaN's sign and payload may differ)
                        for f in ("rho0", "s_rho0") if stage == "regularize_ekf" else ("rho", "s_rho", "rho0", "s_rho0"):
                            if not _same_bits(kg[f][un], want["input"][f][un]):
                                bad.append(tag + f"KeyLine.{f} of a KeyLine without a match lost its bits")
                    if stage.startswith("rescale"):
                        g = dev.get_state(s)
                        if not scalar_close(g.Kp, want["Kp"]):
                            bad.append(tag + f"Kp {g.Kp} vs {want['Kp']}")
                        if not scalar_close(g.P_Kp, want["RKp"]):
                            bad.append(tag + f"P_Kp {g.P_Kp} vs {want['RKp']}")
    finally:
        eh.close()
        eh_div.close()
    print(f"crafted mapping lists {w}x{h} cap={cap}: {len(jobs)} lists, {launches} launches of {NSEQ} sequences, "
          f"{time.perf_counter() - t_start:.1f} s, {len(bad)} mismatches")
    assert not bad, f"{len(bad)} mismatches, first 25:\n" + "\n".join(bad[:25])
