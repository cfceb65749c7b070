"""Crafted KeyLine lists for the stereo path, reference and restatement only (no GPU).

tests/stereo_crafted.py builds a pair mask, a pair list and a main list in which every KeyLine belongs to a named class, and restates
search_match_stereo, getDepthFromStereo and fuseStereoDepth in Python.  Here the reference itself runs on those lists under every rig:

  * the restatement's stereo_m_id and count are the reference's, stereo_rho / stereo_s_rho are the reference's bit for bit (or NaN where
    the reference's is NaN) — which also says that unmatched and ambiguous KeyLines kept their per-KeyLine sentinel bits;
  * every class takes the branch it was built for (the restatement's label) and ends as it was built to end (read off the reference's
    record), with at least MIN_POP members in the 1025-long list, members in the first wave, in the last 65 KeyLines and in between, and
    a match names the pair KeyLine the class says it must;
  * fuseStereoDepth from the reference's post-match state and from the crafted states (s_rho 0 / inf / NaN, stereo_s_rho inf / 1e-300,
    stereo_rho inf, on matched and unmatched KeyLines of every class): rho0 / s_rho0 of every KeyLine, and the restatement agrees;
  * the detector lists of test_stereo_gpu.make_data() at 376 x 240 with 600 edited main KeyLines (rho NaN, rho = s_rho = inf, s_rho NaN):
    the reference matches none of them, and the restatement agrees on all.

The reference prints a line per no-displacement KeyLine; pytest's capture takes it.  Nothing is excluded from any comparison.
"""
import numpy as np
import pytest

import stereo_crafted as sc
from helpers import require_ref


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_or_both_nan(got, want, fields):
    """-> messages for the fields that are neither bit-equal nor NaN on both sides."""
    bad = []
    for f in fields:
        ne = (_bits(got[f]) != _bits(want[f])) & ~(np.isnan(got[f]) & np.isnan(want[f]))
        if ne.any():
            i = np.nonzero(ne)[0]
            bad.append(f"KeyLine.{f}: {len(i)} differ, first {i[:4]}: {got[f][i[:4]]} vs {want[f][i[:4]]}")
    return bad


@pytest.fixture(scope="module")
def ref():
    oracle = require_ref()
    orc = sc.make_reference(oracle)
    yield orc
    orc.close()


def test_restatement_follows_the_reference_and_every_class_is_populated(ref):
    bad, seen = [], set()
    for ri, rig in enumerate(sc.RIGS):
        for variant in (0, 1):
            pair, mask, first = sc.pair_list(variant)
            kl, which = sc.main_list(sc.FULL, 0)
            want, n_ref = sc.reference_match(ref, kl, pair, mask, rig)
            again, n_again = sc.reference_match(ref, kl, pair, mask, rig)
            assert n_again == n_ref and want.tobytes() == again.tobytes(), (rig, "the reference does not repeat itself")
            got, n_got, branch, outcome = sc.directed_matching_stereo(kl, pair, mask, sc.ZF, sc.ZF, sc.PP1, rig)
            tag = f"{rig}, pair variant {variant}: "
            if n_got != n_ref:
                bad.append(tag + f"count {n_got} vs {n_ref}")
            if not np.array_equal(got["stereo_m_id"], want["stereo_m_id"]):
                i = np.nonzero(got["stereo_m_id"] != want["stereo_m_id"])[0]
                bad.append(tag + f"stereo_m_id: {len(i)} differ, first {i[:4]}")
            bad += [tag + m for m in same_or_both_nan(got, want, ("stereo_rho", "stereo_s_rho"))]
            assert n_ref == int((want["stereo_m_id"] >= 0).sum())
            # ---- one outcome per KeyLine, the restatement's and the reference's agree ----
            ref_out = sc.reference_outcome(kl, want)
            assert "?" not in set(ref_out), (rig, "a KeyLine the reference changed without it being a match, a reset or a rejection")
            same = np.where(np.isin(outcome.astype(str), ("none", "ambiguous")), "untouched", outcome.astype(str))
            assert np.array_equal(same, ref_out.astype(str)), (rig, variant)
            # ---- the classes built for this rig ----
            for si, s in enumerate(sc.SUBS):
                if s["rig"] != rig:
                    continue
                idx = np.nonzero(which == si)[0]
                aimed = idx[(branch[idx] == s["branch"]) & (outcome[idx] == s["outcome"]) &
                            (ref_out[idx] == ("untouched" if s["outcome"] in ("none", "ambiguous") else s["outcome"]))]
                if s["hit"] is not None:
                    aimed = aimed[want["stereo_m_id"][aimed] == first[s["name"]] + s["hit"]]
                if len(aimed) != len(idx) or len(aimed) < sc.MIN_POP:
                    bad.append(tag + f"class {s['name']}: {len(aimed)} of {len(idx)} members reach ({s['branch']}, {s['outcome']}); "
                                     f"got {sorted(set(zip(branch[idx], outcome[idx], ref_out[idx])))}")
                if not ((idx < 64).any() and (idx >= sc.FULL - 65).any() and ((idx >= 64) & (idx < sc.FULL - 65)).any()):
                    bad.append(tag + f"class {s['name']}: no member in the first wave, the middle or the last 65 KeyLines")
                seen.add(s["name"])
            if rig == "baseline":                          # mul = 0: rho is +0.0 or -0.0, both accepted
                by = {s["name"]: np.nonzero(which == si)[0] for si, s in enumerate(sc.SUBS)}
                z, nz = want["stereo_rho"][by["g_zero"]], want["stereo_rho"][by["g_neg_zero"]]
                assert np.all(z == 0) and not np.signbit(z).any() and np.all(nz == 0) and np.signbit(nz).all(), (z, nz)
                assert np.all(want["stereo_m_id"][by["g_neg_zero"]] >= 0)
            # ---- fuseStereoDepth: the post-match state as it is, and with the crafted states ----
            states, edit = sc.fuse_states(want)
            for name, start in (("post-match", want), ("crafted", states)):
                fr = sc.reference_fuse(ref, start)
                fg = sc.fuse_stereo_depth(start)
                bad += [tag + f"fuse ({name}): " + m for m in same_or_both_nan(fg, fr, ("rho", "s_rho", "rho0", "s_rho0"))]
                if _bits(fr["rho0"]).tobytes() != _bits(start["rho"]).tobytes() or _bits(fr["s_rho0"]).tobytes() != _bits(start["s_rho"]).tobytes():
                    bad.append(tag + f"fuse ({name}): rho0 / s_rho0 are not the bits of rho / s_rho before the call")
                un = start["stereo_m_id"] < 0
                if _bits(fr["rho"][un]).tobytes() != _bits(start["rho"][un]).tobytes():
                    bad.append(tag + f"fuse ({name}): an unmatched KeyLine's rho changed")
            if variant == 0:
                for e, nm in enumerate(sc.FUSE_EDITS):           # every state on matched and on unmatched KeyLines
                    m = (edit == e)
                    pop = (int((states["stereo_m_id"][m] >= 0).sum()), int((states["stereo_m_id"][m] < 0).sum()))
                    if min(pop) < sc.MIN_POP and rig in ("baseline", "identity", "euroc"):
                        bad.append(tag + f"fusion state {nm}: (matched, unmatched) = {pop}")
            print(f"{tag}{n_ref} matches of {len(kl)}, outcomes {dict(zip(*np.unique(outcome.astype(str), return_counts=True)))}")
    missing = {s["name"] for s in sc.SUBS} - seen
    assert not missing, missing
    assert {s["cls"] for s in sc.SUBS} == set(sc.CLASSES)
    assert not bad, f"{len(bad)} mismatches, first 25:\n" + "\n".join(bad[:25])


def test_lists_are_what_the_gpu_test_assumes():
    """Every length and rotation the GPU test uploads is a list in which KeyLine i belongs to the class main_list says, the pair list
    fits the context and no two pair KeyLines share a pixel (pair_list asserts that)."""
    for v in (0, 1):
        pair, mask, first = sc.pair_list(v)
        assert len(pair) <= sc.CAP and int((mask >= 0).sum()) == len(pair)
        assert np.array_equal(mask.ravel()[pair["p_inx"]], np.arange(len(pair)))
        assert pair["n_m"][mask[0, 0]] == (0.0 if v else 1.0)
    for ri in range(len(sc.RIGS)):
        js = sc.jobs(ri)
        assert [n for n, _, _ in js] == list(sc.LENGTHS) and len(js) % 3 == 0
        for k0 in range(0, len(js), 3):
            assert len({r for _, r, _ in js[k0:k0 + 3]}) == 3 and len({v for _, _, v in js[k0:k0 + 3]}) == 2
        assert len({js[k0][1] for k0 in range(0, len(js), 3)}) == len(js) // 3          # sequence 0's mix rotates
    kl, which = sc.main_list(sc.FULL, 5)
    rho, s = kl["stereo_rho"], kl["stereo_s_rho"]
    assert len(set(_bits(rho).tolist())) == len(kl) and len(set(_bits(s).tolist())) == len(kl)      # a sentinel of its own per KeyLine
    assert np.isnan(rho).sum() > 300 and np.isnan(s).sum() > 200


def test_detector_lists_with_nan_depth_bounds():
    """376 x 240, the lists of test_stereo_gpu.make_data(), 600 edited main KeyLines: NaN depth bounds go through std::max / std::min
    (edge_tracker.cpp:474-475), the KeyLine takes the no-displacement branch with pi0 = NaN and matches nothing."""
    oracle = require_ref()
    c = sc.detector_case(oracle)
    orc, s, ps = c["orc"], c["slot"], c["pair_slot"]
    try:
        orc.set_keylines(ps, c["pair"], c["pair_mask"], c["pair_retuned"])
        orc.set_keylines(s, c["main"], c["main_mask"], c["main_retuned"])
        n_ref = orc.directed_matching_stereo(s, ps, *c["args"])
        want = orc.keylines(s).copy()
    finally:
        orc.close()
    assert all(len(g) == 200 for g in c["groups"].values()) and len(c["edited"]) == 600
    assert n_ref == int((want["stereo_m_id"] >= 0).sum()) > 300
    assert np.all(want["stereo_m_id"][c["edited"]] == -1)
    a = dict(zip(("min_thr_mod", "min_thr_ang", "max_radius", "loc_unc", "q_abs", "q_rel", "loc_unc_model"), c["args"][2:]))
    zfm = lambda zfx, zfy: float((np.float32(zfx) + np.float32(zfy)) / np.float32(2))
    p = oracle.euroc_params(c["w"], c["h"])
    pc = c["pair_cam"]
    got, _, branch, outcome = sc.directed_matching_stereo(c["main"], c["pair"], c["pair_mask"].reshape(c["h"], c["w"]), zfm(p.zfx, p.zfy), zfm(pc["zfx"], pc["zfy"]),
                                                          (pc["ppx"], pc["ppy"]), (c["args"][0], c["args"][1]), a, only=c["edited"])
    e = c["edited"]
    assert np.array_equal(got["stereo_m_id"][e], want["stereo_m_id"][e])
    assert set(branch[e]) == {"across"} and set(outcome[e]) == {"none"}
    assert not same_or_both_nan(got[e], want[e], ("stereo_rho", "stereo_s_rho"))
    # the restatement is the reference's on KeyLines that do match, too: a sample of the untouched ones
    others = np.setdiff1d(np.arange(len(want)), e)[::23]
    got2, _, _, _ = sc.directed_matching_stereo(c["main"], c["pair"], c["pair_mask"].reshape(c["h"], c["w"]), zfm(p.zfx, p.zfy), zfm(pc["zfx"], pc["zfy"]),
                                                (pc["ppx"], pc["ppy"]), (c["args"][0], c["args"][1]), a, only=others)
    assert np.array_equal(got2["stereo_m_id"][others], want["stereo_m_id"][others]) and (want["stereo_m_id"][others] >= 0).sum() > 10
    assert not same_or_both_nan(got2[others], want[others], ("stereo_rho", "stereo_s_rho"))
