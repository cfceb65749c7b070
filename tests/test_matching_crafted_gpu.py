"""k_fwd_key / k_fwd_win / k_fwd_apply, k_rotate and directed_body (k_directed and k_directed_fused<FILL>) against the reference on crafted
KeyLine lists (GPU).

The lists are those of tests/matching_crafted.py; what they reach in the reference — which class takes which branch of search_match and
ends how — is asserted on the CPU, in tests/test_matching_crafted_cpu.py.  In short: norm_t exactly 1e-6 and the doubles either side,
V = 0; the start of the walk on dq_max and one double above it, both bounds clamped and not, round2int_positive's argument on .5 and
either side, t_steps 0, 1, 255, 256, 257; two acceptable candidates where the order of the probes decides, a candidate at the last step
and one at step t_steps, candidates behind skipped probes; walks of up to 1e7 steps from a negative rho and from p3[2] < 0 whose tp run
alone sees the image, walks of 257 to 259 steps from a positive start (both runs of the segment code), arguments on and above 2^31 - 0.5; walks
that leave through each side of the image with coordinates exactly -0.5, w - 0.5 and h - 0.5; each gate on its threshold and either side,
n_m = 0 on either KeyLine; NaN and infinite rho / s_rho / p_m / m_m, p3[2] = 0, with old KeyLines all along row 0 and column 0 of the mask
that only a NaN coordinate turned into 0 would find; a sentinel of its own in every cloned field of every KeyLine; forward matches with
shared targets (rising, falling, mixed and equal rho, +-inf, +-0.0, NaN) and m_id_f of -1, kn_new - 1, kn_new and 2^30.

Two contexts of three sequences (search_range 40 and 255, the largest the library accepts; 160 x 120, max_points = 2048) and one with stereo_available = 1.  Every launch
carries three different lists — lengths 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025, a class mix that rotates from sequence to
sequence and from launch to launch — under every pose of matching_crafted.COMBOS.  There are no tolerances: every comparison is on
copied values and integers.

  launch chain: forward_match, rotate_keylines(R0), directed_matching against the same three calls of the reference; after each step
  every uploaded field of both lists is bit-equal, klm_num / kf_matchs are exact, klm_fwd is the number of distinct targets (<= the
  reference's return value, which counts every write); a second directed_matching on the result, against the reference's second;
  one-pass form (edgehip_match_one_pass: k_fwd_key, k_rotate<OUT, WIN>, k_directed_fused<FILL>) with fill = 0 and fill = 1 against the
  reference's chain: the back-rotation the device stores equals Rodrigues' to 1e-15 and its transpose is what the reference turns the
  old list by; the new list and the three counters are exact, with fill = 1 the ten fields are uploaded as garbage and come back as
  the match's, the forward match's or a fresh KeyLine's; the old slot, read back afterwards, is the reference's turned list.

The forward groups of matching_crafted.FWD_DEVICE_RULE (a NaN rho, +0.0 before -0.0: unreachable in the pipeline) are held to the
device's stated rule instead of :407: for their targets the expectation is the restatement's, forward_match(rule="device") followed by
the restated search; every other KeyLine is held to the reference.  Failures are collected and reported together.
"""
import time

import numpy as np
import pytest

import matching_crafted as mc
from helpers import require_ref, so3_exp, to_edgehip_kl
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu
NSEQ = 3
FIELDS = [f for f in mc.KEYLINE_DTYPE.names if f not in ("_pad0", "score", "net_id", "stereo_m_id", "stereo_rho", "stereo_s_rho")]


def diff(got, want, tag, fields=FIELDS):
    if len(got) != len(want):
        return [f"{tag}list length {len(got)} vs {len(want)}"]
    bad = []
    for f in () if len(got) == 0 else fields:
        a = np.ascontiguousarray(got[f]).view(np.uint8).reshape(len(got), -1)
        b = np.ascontiguousarray(want[f]).view(np.uint8).reshape(len(want), -1)
        i = np.nonzero((a != b).any(axis=1))[0]
        if len(i):
            bad.append(f"{tag}KeyLine.{f}: {len(i)} differ, first {i[:4]}: {got[f][i[:4]]} vs {want[f][i[:4]]}")
    return bad


@pytest.fixture(scope="module")
def world():
    oracle = require_ref()
    w = dict(orc={}, eh={}, old={})
    try:
        for ctx in mc.SEARCH_RANGE:
            w["orc"][ctx] = mc.make_reference(oracle, ctx)
            w["old"][ctx] = mc.old_list(ctx)
        w["orc"]["stereo"] = mc.make_reference(oracle, "near", stereo_mode=True)
        for name, ctx, stereo in (("near", "near", 0), ("far", "far", 0), ("stereo", "near", 1)):
            w["eh"][name] = edgehip.EdgeHip(edgehip.euroc_params(mc.W, mc.H, max_points=mc.CAP, stereo_available=stereo, ppx=mc.PP[0], ppy=mc.PP[1],
                                                                 zfx=mc.ZF, zfy=mc.ZF, search_range=mc.SEARCH_RANGE[ctx]), nseq=NSEQ, nslots=2)
        yield w
    finally:
        for e in w["eh"].values():
            e.close()
        for o in w["orc"].values():
            o.close()


def expected_chain(orc, old_f, mask, new, targets, R0, BR, V, RVel, ctx, stereo=False, second=False):
    """The reference's chain, with the KeyLines the FWD_DEVICE_RULE groups point at held to the device's stated rule (restatement)."""
    want = mc.reference_chain(orc, old_f, mask, new, R0, BR, V, RVel, ctx)
    if second:
        n2, kf2 = orc.directed_matching(1, 0, V, RVel, BR, mc.ARGS["min_thr_mod"], mc.ARGS["min_thr_ang"], float(mc.SEARCH_RANGE[ctx]), mc.ARGS["loc_unc"])
        want.update(new2=orc.keylines(1).copy(), nmatch2=n2, kf2=kf2)
    want["n_targets"] = len({f for tg in targets.values() for f, _ in tg})
    idx = sorted({f for name in mc.FWD_DEVICE_RULE for f, _ in targets.get(name, [])})
    if idx:
        dev_fwd, _ = mc.forward_match(old_f, new, rule="device")
        ref_src, dev_src = want["fwd"].copy(), want["fwd"]
        dev_src[idx] = dev_fwd[idx]
        kf_old = want["turned"]["m_id_kf"]
        for key, kn, kk in (("new", "nmatch", "kf"), ("new2", "nmatch2", "kf2"))[:2 if second else 1]:
            for src, sign in ((ref_src, -1), (dev_src, +1)):           # the reference's own count of these KeyLines out, the device rule's in
                got, _, _, infos = mc.directed_matching(src, want["turned"], mask, (V, RVel, BR), ctx, stereo_mode=stereo, only=idx)
                hit = [i for i in idx if infos[i]["step"] >= 0]
                want[kn] += sign * len(hit)
                want[kk] += sign * sum(int(kf_old[got["m_id"][i]] >= 0) for i in hit)
            ref_src = want[key].copy()
            want[key][idx] = got[idx]
            dev_src = want[key]
    return want


def set_pose(eh, V, RVel, R=None, Wv=None):
    for s in range(NSEQ):
        st = eh.get_state(s)
        st.V[:] = list(V)
        st.P_V[:] = list(np.asarray(RVel).ravel())
        if R is not None:
            st.R[:] = list(np.asarray(R).ravel())
        if Wv is not None:
            st.W[:] = list(Wv)
        st.klm_fwd = st.klm_num = st.kf_matchs = 0
        eh.set_state(s, st)


def counters(eh):
    st = [eh.get_state(s) for s in range(NSEQ)]
    return [s.klm_fwd for s in st], [s.klm_num for s in st], [s.kf_matchs for s in st]


def launches_of(ci, ctx, pose, place, fwd0, old, defaults=False):
    js = mc.jobs(ci)
    for k0 in range(0, len(js), NSEQ):
        case = []
        for s, (n, rot) in enumerate(js[k0:k0 + NSEQ]):
            new, _ = mc.new_list(n, rot, ctx, pose, place, defaults=defaults)
            old_f, targets = mc.with_forward(old, fwd0, n, salt=ci + s + k0)
            case.append((n, rot, new, old_f, targets))
        yield case


def run_chain(w, eh_name, ci, stereo=False):
    ctx, pose = mc.COMBOS[ci]
    eh, orc = w["eh"][eh_name], w["orc"]["stereo" if stereo else ctx]
    old, mask, first, trap0, fwd0, place = w["old"][ctx]
    R0, BR, V, RVel = mc.pose_matrices(pose)
    bad, lists, launches = [], 0, 0
    for case in launches_of(ci, ctx, pose, place, fwd0, old):
        wants = []
        for s, (n, rot, new, old_f, targets) in enumerate(case):
            wants.append(expected_chain(orc, old_f, mask, new, targets, R0, BR, V, RVel, ctx, stereo=stereo, second=True))
            eh.upload_keylines(s, 0, to_edgehip_kl(old_f), mask)
            eh.upload_keylines(s, 1, to_edgehip_kl(new))
            lists += 1
        tags = [f"{ctx}, {pose}{', stereo_mode' if stereo else ''}: sequence {s} ({c[0]} KeyLines, mix {c[1]}): " for s, c in enumerate(case)]
        set_pose(eh, V, RVel, R=BR)
        eh.forward_match(0, 1)
        for s in range(NSEQ):
            kg, _ = eh.download_keylines(s, 1, want_mask=False)
            bad += diff(kg, wants[s]["fwd"], tags[s] + "forward: ")
        fw, _, _ = counters(eh)
        for s in range(NSEQ):
            if fw[s] != wants[s]["n_targets"] or fw[s] > wants[s]["n_fwd"]:
                bad.append(tags[s] + f"klm_fwd {fw[s]}, distinct targets {wants[s]['n_targets']}, the reference wrote {wants[s]['n_fwd']} times")
        eh.rotate_keylines(0, R0)
        for s in range(NSEQ):
            kg, _ = eh.download_keylines(s, 0, want_mask=False)
            bad += diff(kg, wants[s]["turned"], tags[s] + "rotate: ")
        for key, kn, kk in (("new", "nmatch", "kf"), ("new2", "nmatch2", "kf2")):
            set_pose(eh, V, RVel, R=BR)
            eh.directed_matching(1, 0)
            _, num, kfm = counters(eh)
            for s in range(NSEQ):
                kg, _ = eh.download_keylines(s, 1, want_mask=False)
                bad += diff(kg, wants[s][key], tags[s] + f"directed ({key}): ")
                if (num[s], kfm[s]) != (wants[s][kn], wants[s][kk]):
                    bad.append(tags[s] + f"directed ({key}): klm_num, kf_matchs {(num[s], kfm[s])} vs {(wants[s][kn], wants[s][kk])}")
        launches += 4
    return bad, lists, launches


def run_one_pass(w, ci):
    ctx, pose = mc.COMBOS[ci]
    eh, orc = w["eh"][ctx], w["orc"][ctx]
    old, mask, first, trap0, fwd0, place = w["old"][ctx]
    _, _, V, RVel = mc.pose_matrices(pose)
    Wv = mc.POSES[pose]["W"]
    bad, lists, launches = [], 0, 0
    for fill in (0, 1):
        for case in launches_of(ci, ctx, pose, place, fwd0, old, defaults=bool(fill)):
            tags = [f"{ctx}, {pose}, one pass, fill {fill}: sequence {s} ({c[0]} KeyLines, mix {c[1]}): " for s, c in enumerate(case)]
            ups = []
            for s, (n, rot, new, old_f, targets) in enumerate(case):
                ups.append(mc.garbage_ten(new) if fill else new)
                eh.upload_keylines(s, 0, to_edgehip_kl(old_f), mask)
                eh.upload_keylines(s, 1, to_edgehip_kl(ups[s]))
                lists += 1
            set_pose(eh, V, RVel, Wv=Wv)
            eh.match_one_pass(1, 0, fill)
            launches += 3
            BRs = [np.array(eh.get_state(s).R[:]).reshape(3, 3) for s in range(NSEQ)]
            err = max(np.abs(b - so3_exp(np.array(Wv, np.float64)).T).max() for b in BRs)
            if err > 1e-15 or any(b.tobytes() != BRs[0].tobytes() for b in BRs):
                bad.append(tags[0] + f"the stored back-rotation is {err:.3g} from Rodrigues'")
            BR = BRs[0]
            fw, num, kfm = counters(eh)
            for s, (n, rot, new, old_f, targets) in enumerate(case):
                want = expected_chain(orc, old_f, mask, new, targets, BR.T.copy(), BR, V, RVel, ctx)
                kg, _ = eh.download_keylines(s, 1, want_mask=False)
                bad += diff(kg, want["new"], tags[s] + "new list: ", fields=mc.TEN)
                bad += diff(kg, ups[s], tags[s] + "new list, fields the matching does not write: ", fields=[f for f in FIELDS if f not in mc.TEN])
                if (fw[s], num[s], kfm[s]) != (want["n_targets"], want["nmatch"], want["kf"]) or fw[s] > want["n_fwd"]:
                    bad.append(tags[s] + f"klm_fwd, klm_num, kf_matchs {(fw[s], num[s], kfm[s])} vs {(want['n_targets'], want['nmatch'], want['kf'])}")
                ko, _ = eh.download_keylines(s, 0, want_mask=False)
                bad += diff(ko, want["turned"], tags[s] + "old list afterwards: ")
    return bad, lists, launches


def _report(name, t0, bad, lists, launches):
    print(f"{name}: {lists} lists, {launches} launches of {NSEQ} sequences, {time.perf_counter() - t0:.1f} s, {len(bad)} mismatches")
    assert not bad, f"{len(bad)} mismatches, first 25:\n" + "\n".join(bad[:25])


@pytest.mark.parametrize("ci", range(len(mc.COMBOS)), ids=[f"{c}-{p}" for c, p in mc.COMBOS])
def test_launch_chain_follows_the_reference(world, ci):
    t0 = time.perf_counter()
    _report("launch chain " + "-".join(mc.COMBOS[ci]), t0, *run_chain(world, mc.COMBOS[ci][0], ci))


@pytest.mark.parametrize("ci", [i for i, (c, p) in enumerate(mc.COMBOS) if c == "near" and p in ("x", "zero", "rot_a")], ids=lambda i: "-".join(mc.COMBOS[i]))
def test_launch_chain_with_stereo_available(world, ci):
    """stereo_mode: rho0 / s_rho0 of the match are cloned into rho / s_rho, rho_nr / s_rho_nr keep their sentinels."""
    t0 = time.perf_counter()
    _report("launch chain, stereo_available " + "-".join(mc.COMBOS[ci]), t0, *run_chain(world, "stereo", ci, stereo=True))


@pytest.mark.parametrize("ci", range(len(mc.COMBOS)), ids=[f"{c}-{p}" for c, p in mc.COMBOS])
def test_one_pass_form_follows_the_reference(world, ci):
    t0 = time.perf_counter()
    _report("one pass " + "-".join(mc.COMBOS[ci]), t0, *run_one_pass(world, ci))


def test_one_pass_entry_refuses_what_the_frame_would_not_do(world):
    eh = world["eh"]["stereo"]
    assert eh.lib.edgehip_match_one_pass(eh.ctx, 1, 0, 0) == -4          # EDGEHIP_ERR_STATE: stereo_available frames use the launch chain
    eh = world["eh"]["near"]
    assert eh.lib.edgehip_match_one_pass(eh.ctx, 1, 1, 0) == -1 and eh.lib.edgehip_match_one_pass(eh.ctx, 2, 0, 0) == -1
