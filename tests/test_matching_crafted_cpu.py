"""Crafted KeyLine lists for forward and directed matching, reference and restatement only (no GPU).

tests/matching_crafted.py builds, per context, an old list with its mask and new lists in which every KeyLine
belongs to a named class (search_range 40 and 255), and restates FordwardMatch, search_match and directed_matching in Python.  Here the reference itself runs on
the 1025-long list of every (context, pose) pair:

  * the restatement's new list equals the reference's bit for bit on every field, and both counts (nmatch, kf_matchs; FordwardMatch's
    return value) are the reference's — for directed_matching alone, for the chain FordwardMatch -> rotate_keylines ->
    directed_matching with the crafted forward matches, and with stereo_mode;
  * every class reaches, under the pose it was built for, the branch it was built for (its predicate on the restatement's record of
    the walk: branch, round2int_positive's argument, t_steps, bounds, step and direction of the match) and the outcome (the old
    KeyLine it must match, a trap of row / column 0, or none) with at least MIN_POP members; no KeyLine whose walk never produced a
    finite probe matched a trap;
  * cloned fields: matches whose old KeyLine has m_id_kf >= 0 and < 0, unmatched KeyLines that keep the bytes of all ten fields, and
    stereo_mode matches with rho0 / s_rho0 cloned and rho_nr / s_rho_nr kept, each at least MIN_POP times;
  * every forward group has the winner :407 gives it when read by hand, at least MIN_POP times;
  * the kernel's two step-index runs (segment_runs) never exist apart on any crafted KeyLine and no tn run is entered beyond step 0
    (matching_crafted.py says why), and each of "tp run alone, entered beyond step 0" and "both, merged" has at least MIN_POP members;
  * the reference executes at most 2e8 walk iterations over everything this file runs.

Nothing is excluded from any comparison; failures are collected and reported together.
"""
import numpy as np
import pytest

import matching_crafted as mc
from helpers import require_ref

ITER_CAP = 2e8


def diff(got, want, tag):
    """-> messages for the fields whose bytes differ."""
    if len(got) != len(want):
        return [f"{tag}list length {len(got)} vs {len(want)}"]
    bad = []
    for f in () if len(got) == 0 else got.dtype.names:
        a = np.ascontiguousarray(got[f]).view(np.uint8).reshape(len(got), -1)
        b = np.ascontiguousarray(want[f]).view(np.uint8).reshape(len(want), -1)
        i = np.nonzero((a != b).any(axis=1))[0]
        if len(i):
            bad.append(f"{tag}KeyLine.{f}: {len(i)} differ, first {i[:4]}: {got[f][i[:4]]} vs {want[f][i[:4]]}")
    return bad


@pytest.fixture(scope="module")
def refs():
    oracle = require_ref()
    r = {ctx: mc.make_reference(oracle, ctx) for ctx in mc.SEARCH_RANGE}
    r["stereo"] = mc.make_reference(oracle, "near", stereo_mode=True)
    yield r
    for o in r.values():
        o.close()


def test_restatement_follows_the_reference_and_every_class_is_populated(refs):
    bad, seen, iters = [], set(), 0
    runs = dict(both=0, tp_alone=0)
    fwd_seen = {}
    cloned = dict(matched_kf=0, matched_no_kf=0, unmatched_keeps_bytes=0, stereo_rho0_cloned=0)
    for ci, (ctx, pose) in enumerate(mc.COMBOS):
        orc = refs[ctx]
        old, mask, first, trap0, fwd0, place = mc.old_list(ctx)
        R0, BR, V, RVel = mc.pose_matrices(pose)
        new, which = mc.new_list(mc.FULL, 0, ctx, pose, place)
        tag = f"{ctx}, {pose}: "
        # ---- directed_matching alone ----
        want = mc.reference_chain(orc, old, mask, new, R0, BR, V, RVel, ctx)
        assert want["n_fwd"] == 0 and want["fwd"].tobytes() == new.tobytes()
        got, n, kf, infos = mc.directed_matching(new, want["turned"], mask, (V, RVel, BR), ctx)
        iters += sum(i["iters"] for i in infos)
        if (n, kf) != (want["nmatch"], want["kf"]):
            bad.append(tag + f"counts {(n, kf)} vs {(want['nmatch'], want['kf'])}")
        bad += diff(got, want["new"], tag)
        assert want["nmatch"] == int((want["new"]["m_id"] >= 0).sum())
        m_id = want["new"]["m_id"]
        # a walk without a single probe inside the image cannot have matched; a trap is matched only by a walk that reached it
        blind = np.array([i["probes"] == 0 for i in infos])
        if (m_id[blind] >= 0).any():
            bad.append(tag + f"{int((m_id[blind] >= 0).sum())} KeyLines without a probe inside the image matched")
        for si, s in enumerate(mc.SUBS):
            if not mc.home(s, ctx, pose):
                continue
            idx = np.nonzero(which == si)[0]
            y_, x_ = place[s["name"]]
            if s["expect"] == "trap":
                exp = trap0 + int(x_) if s["new"]["X0"] == "col" else trap0 + mc.W + int(y_) - 1
            elif s["expect"] is None:
                exp = -1
            elif s["expect"] == "any":
                exp = None
            else:
                exp = first[s["name"]] + s["expect"]
            ok = np.array([(exp is None or m_id[i] == exp) and (s["pred"] is None or bool(s["pred"](infos[i]))) for i in idx])
            if len(idx) < mc.MIN_POP or not ok.all():
                j = idx[~ok][:1]
                bad.append(tag + f"class {s['name']}: {int(ok.sum())} of {len(idx)} members as built (want match {exp}); "
                                 f"first other: m_id {m_id[j]}, {infos[j[0]] if len(j) else ''}")
            if not ((idx < 128).any() and (idx >= mc.FULL - 129).any()):
                bad.append(tag + f"class {s['name']}: no member in the first or in the last block")
            seen.add((s["name"], ctx))
        # ---- cloned fields: a match carries the old KeyLine's bytes (diff above), with and without a keyframe match; an unmatched
        # KeyLine keeps its sentinels in all ten fields ----
        if pose == "x":
            hit = m_id >= 0
            kf_old = want["turned"]["m_id_kf"][m_id[hit]]
            cloned["matched_kf"] += int((kf_old >= 0).sum())
            cloned["matched_no_kf"] += int((kf_old < 0).sum())
            if not np.array_equal(want["new"]["m_id_kf"][hit], kf_old) or want["kf"] != int((kf_old >= 0).sum()):
                bad.append(tag + "m_id_kf of a match is not the old KeyLine's, or kf_matchs is not their count")
            keeps = ~hit
            for f in mc.TEN:
                a_, b_ = (np.ascontiguousarray(x[f]).view(np.uint8).reshape(len(new), -1) for x in (want["new"], new))
                keeps &= (a_ == b_).all(axis=1)
            if not np.array_equal(keeps, ~hit):
                bad.append(tag + f"{int((~hit & ~keeps).sum())} unmatched KeyLines lost sentinel bytes")
            cloned["unmatched_keeps_bytes"] += int(keeps.sum())
        # ---- the displacement classes are poses: every KeyLine with finite fields is a member ----
        fin = np.isfinite(new["rho"]) & np.isfinite(new["p_m"]).all(axis=1)
        br = np.array([i["branch"] for i in infos])
        if pose in ("zero", "nt_on", "nt_below") and not (br[fin] == "across").all():
            bad.append(tag + "norm_t <= 1e-6 but a KeyLine took the displacement branch")
        if pose in ("x", "nt_above") and (br[fin] == "across").any():
            bad.append(tag + "norm_t > 1e-6 but a KeyLine took the no-displacement branch")
        if pose.startswith("nt_"):
            want_nt = dict(nt_on=mc.C_1EM6, nt_below=float(np.nextafter(mc.C_1EM6, 0)), nt_above=float(np.nextafter(mc.C_1EM6, 1)))[pose]
            nts = {i["norm_t"] for i, f in zip(infos, fin) if f}
            assert nts == ({1.0} if pose != "nt_above" else {want_nt}), (pose, sorted(nts)[:4])
        # ---- the kernel's step-index runs ----
        for i in infos:
            sr = mc.segment_runs(i, ctx)
            if sr is None:
                continue
            if sr["hn"] and sr["hp"]:
                if sr["n1"] < sr["p0"] or sr["p1"] < sr["n0"] or sr["n0"] != 0 or sr["p0"] != 0:
                    bad.append(tag + f"two runs apart: {sr}")
                runs["both"] += 1
            if sr["hn"] and sr["n0"] != 0:
                bad.append(tag + f"a tn run entered beyond step 0: {sr}")
            if sr["hp"] and not sr["hn"]:
                runs["tp_alone"] += sr["p0"] > 0
        # ---- the chain with forward matches (and once with stereo_mode) ----
        if pose in ("x", "rot_a", "flip"):
            for orc2, stereo, n_new in ((orc, False, 257),) + (((refs["stereo"], True, 129),) if (ctx, pose) == ("near", "x") else ()):
                new2, _ = mc.new_list(n_new, 5 + ci, ctx, pose, place)
                old_f, targets = mc.with_forward(old, fwd0, n_new, ci)
                want = mc.reference_chain(orc2, old_f, mask, new2, R0, BR, V, RVel, ctx)
                gf, nf = mc.forward_match(old_f, new2)
                if nf != want["n_fwd"]:
                    bad.append(tag + f"FordwardMatch returns {want['n_fwd']}, the restatement {nf}")
                bad += diff(gf, want["fwd"], tag + "forward: ")
                got, n, kf, infos2 = mc.directed_matching(want["fwd"], want["turned"], mask, (V, RVel, BR), ctx, stereo_mode=stereo)
                iters += sum(i["iters"] for i in infos2)
                if (n, kf) != (want["nmatch"], want["kf"]):
                    bad.append(tag + f"chain{' (stereo_mode)' if stereo else ''}: counts {(n, kf)} vs {(want['nmatch'], want['kf'])}")
                bad += diff(got, want["new"], tag + f"chain{' (stereo_mode)' if stereo else ''}: ")
                if stereo:                                    # rho0 / s_rho0 cloned, rho_nr / s_rho_nr kept (a match is an old KeyLine on the mask)
                    on = np.nonzero(want["new"]["m_id"] != want["fwd"]["m_id"])[0]
                    j = want["new"]["m_id"][on]
                    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
                    ok = (bits(want["new"]["rho"][on]) == bits(want["turned"]["rho0"][j])) & (bits(want["new"]["s_rho"][on]) == bits(want["turned"]["s_rho0"][j])) & \
                        (bits(want["new"]["rho_nr"][on]) == bits(want["fwd"]["rho_nr"][on])) & (bits(want["new"]["s_rho_nr"][on]) == bits(want["fwd"]["s_rho_nr"][on]))
                    if not ok.all():
                        bad.append(tag + f"stereo_mode: {int((~ok).sum())} matches without rho0 / s_rho0 cloned or with rho_nr / s_rho_nr changed")
                    cloned["stereo_rho0_cloned"] += int(ok.sum())
                for name, tg in targets.items():
                    for f, i0 in tg:
                        win = want["fwd"]["m_id"][f]
                        exp = fwd0 + mc.N_FWD - 4 if name == "last" else i0 + mc.FWD_WINNER[name]      # "last": rho rises from repeat to repeat
                        if win != exp:
                            bad.append(tag + f"forward group {name} at target {f}: winner {win}, by hand {exp}")
                        fwd_seen[name] = fwd_seen.get(name, 0) + 1
                untouched = np.setdiff1d(np.arange(n_new), [f for tg in targets.values() for f, _ in tg])
                if want["fwd"][untouched].tobytes() != new2[untouched].tobytes():
                    bad.append(tag + "a new KeyLine nobody points at lost its detector fields in FordwardMatch")
        print(f"{tag}{want['nmatch']} matches, iterations so far {iters:.3g}")
    for s in mc.SUBS:
        for ctx in mc.SEARCH_RANGE:
            if s["ctx"] in ("*", ctx) and (ctx, s["poses"][0]) in mc.COMBOS and (s["name"], ctx) not in seen:
                bad.append(f"class {s['name']} was never checked in context {ctx}")
    assert {s["cls"] for s in mc.SUBS} == set(mc.CLASSES)
    for name, _ in mc.FWD_GROUPS:
        if fwd_seen.get(name, 0) < mc.MIN_POP:
            bad.append(f"forward group {name}: {fwd_seen.get(name, 0)} targets")
    for k, v in runs.items():
        if v < mc.MIN_POP:
            bad.append(f"step-index runs '{k}': {v} members")
    for k, v in cloned.items():
        if v < mc.MIN_POP:
            bad.append(f"cloned fields '{k}': {v} members")
    print(f"cloned {cloned}, runs {runs}, forward groups {fwd_seen}, reference iterations {iters:.3g}")
    assert iters <= ITER_CAP, f"the reference executes {iters:.3g} walk iterations"
    assert not bad, f"{len(bad)} mismatches, first 30:\n" + "\n".join(bad[:30])


def test_lists_are_what_the_gpu_test_assumes():
    """Lengths, rotations, sentinels and forward targets of the lists the GPU test uploads."""
    for ci, (ctx, pose) in enumerate(mc.COMBOS):
        old, mask, first, trap0, fwd0, place = mc.old_list(ctx)
        assert len(old) <= mc.CAP and fwd0 + mc.N_FWD == len(old)
        on = np.nonzero(mask.ravel() >= 0)[0]
        assert np.array_equal(mask.ravel()[old["p_inx"][:fwd0]], np.arange(fwd0)) and len(on) == fwd0
        assert (mask[0] >= trap0).all() and (mask[:, 0] >= trap0).all()
        js = mc.jobs(ci)
        assert [n for n, _ in js] == list(mc.LENGTHS) and len(js) % 3 == 0
        pool = len(mc.subs_of(ctx, pose))
        for k0 in range(0, len(js), 3):
            assert len({r % pool for _, r in js[k0:k0 + 3]}) == 3
        assert len({js[k0][1] % pool for k0 in range(0, len(js), 3)}) >= 3          # sequence 0's mix rotates
    old, mask, first, trap0, fwd0, place = mc.old_list("near")
    kl, _ = mc.new_list(mc.FULL, 5, "near", "x", place)
    for f in ("rho_nr", "s_rho_nr", "n_m0"):
        assert len(set(np.ascontiguousarray(kl[f]).view(np.uint64).tolist())) == len(kl), f
    assert np.isnan(kl["rho_nr"]).sum() > 300 and (kl["m_id"] == -1).all() and (kl["m_num"] == 0).all()
    g = mc.garbage_ten(kl)
    for f in mc.TEN:
        assert (np.ascontiguousarray(g[f]).view(np.uint8).reshape(len(g), -1) != np.ascontiguousarray(kl[f]).view(np.uint8).reshape(len(g), -1)).any(axis=1).all(), f
    o, targets = mc.with_forward(old, fwd0, 1025)
    assert all(len(targets[name]) == mc._FWD_REPEAT for name, _ in mc.FWD_GROUPS)
    o, targets = mc.with_forward(old, fwd0, 1)
    assert (o["m_id_f"][fwd0:fwd0 + mc.N_FWD - 4 * mc._FWD_REPEAT] == -1).all() and targets == {"last": [(0, len(o) - 4)]}


def test_segment_runs_is_a_copy_of_the_kernels_expressions():
    """matching_crafted.segment_runs restates four expressions of directed_body by hand; the statements proved with it (no two runs
    apart, no tn run entered beyond step 0) are about the kernel only while the kernel still reads like this."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rebvo_amd", "csrc", "stage_c.hip")).read()
    for line in ("const double Tmax = (double)(a.w + a.h) + fabs((double)pi0x) + fabs((double)pi0y) + 4.0;",
                 "if (t_steps > 256 && fabs(dq_rho) < 1e15 && Tmax < 1e15) {",
                 "const double n0 = fmax(0.0, floor(dq_rho - Tmax) - 2.0), n1 = fmin((double)t_steps, ceil(fmin(dq_rho + Tmax, dq_rho - dq_min)) + 2.0);",
                 "const double p0 = fmax(0.0, floor(-Tmax - dq_rho - 1.0) - 2.0), p1 = fmin((double)t_steps, ceil(fmin(Tmax - dq_rho - 1.0, dq_max - dq_rho - 1.0)) + 2.0);",
                 "if (hn && hp && !(n1 < p0 || p1 < n0)) {"):
        assert src.count(line) == 1, f"directed_body no longer has `{line}`: bring matching_crafted.segment_runs up to date"
