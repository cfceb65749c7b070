"""Crafted KeyLine lists for the mapping stages, reference and port only (no GPU).

Regularize_1_iter, UpdateInverseDepthKalman (ARLU) and EstimateReScalingOpt are otherwise compared only on lists the detector and the
matcher made from the synthetic scenes, which never reach the EKF's RHO_MAX clamp or its NaN reset, a NaN out of the regularizer, the
rescale's s_rho0 <= 0 gate, or a list longer than 16 000 KeyLines.  helpers.crafted_mapping_lists edits the reference's own matched
list so that every one of those branches is taken by 50 KeyLines or more, and cuts it at the lengths where k_rescale<512,12,4>
changes storage (12 288: registers -> LDS, 16 384: LDS -> streamed) and where a virtual thread gains a KeyLine (1024).  This module
checks, without a device, that the lists do what they are meant to:

  * the reference run twice from the same injected state gives the same bytes (nothing crafted leaves defined behaviour);
  * the branch populations, read off the reference's output — or, where the output cannot show them (the depth gate, alpha < thresh),
    predicted in numpy from the input, with the prediction of "left alone by the regularizer" checked against the output bit for bit
    and against the reference's own count of regularized KeyLines;
  * the port (oracle/port) follows the reference on every list and stage with the tolerances of tests/test_mapping_crafted_gpu.py,
    and with the branch outcomes as exact sets: two independent implementations read the crafted lists the same way.

The EKF's fourth arm (s_rho < 0, edge_tracker.cpp:1045) cannot be taken: s_rho is a sqrt, so it is >= 0, -0.0 or NaN, and NaN went to
the third arm.  Nothing is excluded from any comparison.
"""
import numpy as np
import pytest

from helpers import (RESCALE_REGIONS, RHO_INIT, RHO_MAX, RHO_MIN, crafted_mapping_lists, cut_list, depth_state_mismatches, indices_inside,
                     mapping_lengths, mapping_stages, require_ref, scalar_close)

CASES = [(376, 240, 16000), (752, 480, 20000)]
VARIANTS = ("ekf", "regularize", "rescale", "rescale_none")
MIN_POP = 50


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def crafted(request):
    oracle = require_ref()
    w, h, cap = request.param
    c = crafted_mapping_lists(w, h, cap)
    c["port"] = oracle.Oracle("port", oracle.euroc_params(w, h, max_points=cap))
    yield c
    c["port"].close()
    c["orc"].close()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same_bits(a, b, fields):
    return all(_bits(a[f]) == _bits(b[f]) for f in fields)


def regularize_prediction(kl):
    """Which KeyLines Regularize_1_iter leaves alone, from its input (edge_tracker.cpp:98-118): float alpha, double gates."""
    n = len(kl)
    valid = (kl["n_id"] >= 0) & (kl["p_id"] >= 0)
    ni, pi = np.where(valid, kl["n_id"], 0), np.where(valid, kl["p_id"], 0)
    with np.errstate(all="ignore"):
        d = kl["rho"][ni] - kl["rho"][pi]
        gate = valid & (d * d > kl["s_rho"][ni] * kl["s_rho"][ni] + kl["s_rho"][pi] * kl["s_rho"][pi])
        mn, mp = kl["m_m"][ni], kl["m_m"][pi]
        alpha = (mn[:, 0] * mp[:, 0] + mn[:, 1] * mp[:, 1]) / (kl["n_m"][ni] * kl["n_m"][pi])
        assert alpha.dtype == np.float32
        below = valid & ~gate & (alpha.astype(np.float64) - 0.5 < 0)
    done = valid & ~gate & ~below
    assert len(done) == n
    return dict(valid=valid, gate=gate, below=below, done=done, alpha=alpha, alpha_nan=done & np.isnan(alpha))


def rescale_replica(kl):
    """EstimateReScalingOpt (edge_tracker.cpp:1113-1130) in numpy: the same expressions, summed in list order (cumsum)."""
    counted = ~((kl["m_num"].astype(np.uint32) < np.uint32(1)) | (kl["s_rho0"] <= 0) | (kl["s_rho"] > RHO_MAX))
    k = kl[counted]
    Kp, RKp = 1.0, 0.0
    with np.errstate(all="ignore"):
        for _ in range(5):
            den = k["s_rho"] * k["s_rho"] + Kp * Kp * k["s_rho0"] * k["s_rho0"]
            a = np.cumsum(k["rho"] * k["rho"] / den)[-1] if len(k) else 0.0
            b = np.cumsum(k["rho0"] * k["rho0"] / den)[-1] if len(k) else 0.0
            Kp = float(np.sqrt(a / b)) if b > 0 else 1.0
            RKp = float(np.float64(1.0) / np.float64(b))
    return counted, Kp, RKp


def _populations(variant, lst, out, edits):
    """(counts to print, assertions that hold at full length) for one list."""
    n = len(lst)
    c, must = {}, []
    # ---- EKF alone on the crafted list ----
    o = out["ekf_raw"]["kl"]
    m = lst["m_id"] >= 0
    c["ekf"] = dict(rho_max=int(((o["rho"] == RHO_MAX) & m).sum()), rho_min=int(((o["rho"] == RHO_MIN) & m).sum()),
                    reset=int(((o["rho"] == RHO_INIT) & (o["s_rho"] == RHO_MAX) & m).sum()),
                    nonfinite_left=int((~np.isfinite(o["rho"]) | ~np.isfinite(o["s_rho"])).sum()))
    # an unmatched KeyLine is not touched by the EKF (edge_tracker.cpp:710): all four fields keep their bits, in every EKF stage
    for st in ("ekf_raw", "ekf", "regularize_ekf"):
        a, b = out[st]["kl"], out[st]["input"] if st != "regularize_ekf" else out["regularize"]["kl"]
        assert _same_bits(a[~m], b[~m], ("rho", "s_rho", "rho0", "s_rho0")), (variant, n, st)
    if variant == "ekf":
        e = {k: v[v < n] for k, v in edits.items()}
        c["ekf"]["unmatched_edited"] = len(e["unmatched"])
        cls = np.where(~m, "unmatched", np.where(o["rho"] == RHO_MAX, "max", np.where(o["rho"] == RHO_MIN, "min", np.where(
            (o["rho"] == RHO_INIT) & (o["s_rho"] == RHO_MAX), "reset", np.where(np.isfinite(o["rho"]) & np.isfinite(o["s_rho"]), "inside", "nonfinite")))))
        c["ekf_by_edit"] = {k: {str(a): int(b) for a, b in zip(*np.unique(cls[v], return_counts=True))} for k, v in e.items()}
        live = {k: v[m[v]] for k, v in e.items() if k != "unmatched"}
        must += [(f"EKF edit {k}: live KeyLines", len(v)) for k, v in live.items()]
        must += [("EKF RHO_MAX clamp", c["ekf"]["rho_max"]), ("EKF RHO_MIN clamp", c["ekf"]["rho_min"]), ("EKF reset", c["ekf"]["reset"]),
                 ("EKF pass-through of edited unmatched KeyLines", len(e["unmatched"])),
                 ("rho_max edit at RHO_MAX", int((cls[live["rho_max"]] == "max").sum())),
                 ("rho_min edit at RHO_MIN, s_rho grown by the overshoot", int(((cls[live["rho_min"]] == "min") & (o["s_rho"][live["rho_min"]] > 1)).sum())),
                 ("n_m0 = 0 reset", int((cls[live["n_m0_zero"]] == "reset").sum())), ("NaN reset", int((cls[live["nan"]] == "reset").sum())),
                 ("s_rho = inf reset", int((cls[live["s_rho_inf"]] == "reset").sum()))]
        huge = np.concatenate([live["huge_s_rho_max"], live["huge_s_rho_min"]])
        c["ekf"]["clamped_with_nan_s_rho"] = int((np.isin(cls[huge], ("max", "min")) & np.isnan(o["s_rho"][huge])).sum())
        must.append(("clamped at a limit with a NaN s_rho (only the arm order keeps them from the reset)", c["ekf"]["clamped_with_nan_s_rho"]))
        pole = cls[live["rho_pole"]]                  # rho_p = inf: +inf is caught by the RHO_MAX arm, -inf by the RHO_MIN arm, NaN by the reset
        must.append(("pole handled by one of the first three arms", int(np.isin(pole, ("max", "min", "reset")).sum())))
    # ---- regularize ----
    p = regularize_prediction(lst)
    o = out["regularize"]["kl"]
    assert out["regularize"]["r_num"] == int(p["done"].sum()), (variant, n, out["regularize"]["r_num"], int(p["done"].sum()))
    assert _same_bits(o[~p["done"]], lst[~p["done"]], ("rho", "s_rho")), (variant, n, "a KeyLine predicted as left alone changed")
    c["reg"] = dict(done=int(p["done"].sum()), no_neighbour=int((~p["valid"]).sum()), gate=int(p["gate"].sum()), below=int(p["below"].sum()),
                    alpha_nan=int(p["alpha_nan"].sum()), nan_out=int((np.isnan(o["rho"]) | np.isnan(o["s_rho"])).sum()))
    if variant == "regularize":
        e = {k: v[v < n] for k, v in edits.items()}
        must += [(f"regularize edit {k}: centres", len(v)) for k, v in e.items()]
        alpha_reached = p["done"] | p["below"]                    # past both the neighbour check and the depth gate: alpha is computed
        must += [("depth gate rejects", c["reg"]["gate"]), ("alpha < thresh", c["reg"]["below"]), ("NaN alpha let through", c["reg"]["alpha_nan"]),
                 ("NaN out of regularize", c["reg"]["nan_out"])]
        exact = dict(gate_on=p["done"], gate_above=p["gate"], gate_below=p["done"], alpha_on=p["done"], alpha_below=p["below"], alpha_above=p["done"],
                     alpha_one=p["valid"] & (p["alpha"] == 1), no_next=~p["valid"], no_prev=~p["valid"], nb_alpha_nan=p["alpha_nan"],
                     next_is_prev=p["done"], own_s_rho_zero=p["valid"], nb_n_m_zero_n=alpha_reached, nb_n_m_zero_p=alpha_reached,
                     next_is_self=alpha_reached, prev_is_self=alpha_reached, nb_s_rho_zero=p["done"])
        c["reg_by_edit"] = {k: f"{int(v[e[k]].sum())}/{len(e[k])}" for k, v in exact.items()}
        must += [(f"regularize edit {k} lands where it is aimed", int(v[e[k]].sum()) if v[e[k]].all() else 0) for k, v in exact.items()]
        own = e["own_s_rho_zero"][p["done"][e["own_s_rho_zero"]]]
        must.append(("own s_rho = 0: the regularized KeyLines are NaN (inf / inf)", len(own) if np.isnan(o["rho"][own]).all() and len(own) else 0))
        nb = e["nb_s_rho_zero"][p["done"][e["nb_s_rho_zero"]]]
        c["reg"]["nb_s_rho_zero_done"] = len(nb)
        must.append(("neighbour s_rho = 0: wrn is infinite and the regularized KeyLines are NaN (inf / inf)",
                     len(nb) if len(nb) and np.isnan(o["rho"][nb]).all() and np.isnan(o["s_rho"][nb]).all() else 0))
        for k in ("nb_n_m_zero_n", "nb_n_m_zero_p"):              # alpha = x / 0: +inf or NaN goes on (not < thresh), -inf is skipped
            a = p["alpha"][e[k]]
            must.append((f"{k}: alpha is not finite", len(a) if not np.isfinite(a).any() else 0))
        on = e["alpha_on"]                                        # (own s_rho = 0: see helpers) regularized at alpha == thresh shows as NaN
        must.append(("alpha == thresh is regularized: NaN (inf / inf) where a skipped KeyLine keeps its bits",
                     len(on) if np.isnan(o["rho"][on]).all() and np.isnan(o["s_rho"][on]).all() else 0))
        bl = e["alpha_below"]
        must.append(("one float below thresh is skipped: the bits stay", len(bl) if _same_bits(o[bl], lst[bl], ("rho", "s_rho")) else 0))
    # ---- rescale ----
    counted, kp, rkp = rescale_replica(lst)
    r = out["rescale"]
    assert scalar_close(kp, r["Kp"], 1e-13) and scalar_close(rkp, r["RKp"], 1e-13), (variant, n, kp, r["Kp"], rkp, r["RKp"])
    c["rescale"] = {f"region{j}": (int(counted[lo:hi].sum()), int((~counted[lo:hi]).sum())) for j, (lo, hi) in enumerate(RESCALE_REGIONS) if lo < n}
    c["rescale"]["Kp"], c["rescale"]["RKp"] = r["Kp"], r["RKp"]
    if variant == "rescale":
        edits = {k: v[v < n] for k, v in edits.items()}
        for k in ("s_rho_at", "s_rho_below", "m_num_neg"):
            must.append((f"rescale edit {k} counts", len(edits[k]) if counted[edits[k]].all() else 0))
        for k in ("s_rho0_zero", "s_rho0_neg", "s_rho0_negzero", "s_rho_above", "m_num_zero"):
            must.append((f"rescale edit {k} is rejected", len(edits[k]) if not counted[edits[k]].any() else 0))
        for j, (lo, hi) in enumerate(RESCALE_REGIONS):
            if lo < n:
                must += [(f"rescale region {j}: counted", int(counted[lo:hi].sum())), (f"rescale region {j}: rejected", int((~counted[lo:hi]).sum()))]
        without = lst.copy()                      # m_num = -1 compares as unsigned in the reference (:1119): those KeyLines count
        without["m_num"][edits["m_num_neg"]] = 0
        assert len(edits["m_num_neg"]) == 0 or not scalar_close(rescale_replica(without)[1], r["Kp"], 1e-10)
    if variant == "rescale_none":
        assert not counted.any() and r["Kp"] == 1 and r["RKp"] == np.inf, (n, r["Kp"], r["RKp"])      # tb = 0
        assert _same_bits(out["rescale_div"]["kl"], lst, ("rho", "s_rho"))
    return c, must


def test_reference_repeats_and_every_branch_is_populated(crafted):
    c = crafted
    pose = (c["V"], c["RVel"], c["RW0"])
    for variant in VARIANTS:
        for n in mapping_lengths(c["kn"]):
            lst, mask = cut_list(c["variants"][variant], c["mask"], n)
            assert indices_inside(lst) and len(lst) == n
            a = mapping_stages(c["orc"], c["slot"], lst, mask, c["retuned"], *pose)
            b = mapping_stages(c["orc"], c["slot"], lst, mask, c["retuned"], *pose)
            for st in a:
                assert _bits(a[st]["kl"]) == _bits(b[st]["kl"]), (variant, n, st)
                for k in ("Kp", "RKp", "r_num"):
                    assert k not in a[st] or _bits(np.float64(a[st][k])) == _bits(np.float64(b[st][k])), (variant, n, st, k)
            counts, must = _populations(variant, lst, a, c["edits"][variant])
            print(f"crafted {c['orc'].w}x{c['orc'].h} {variant} n={n}: {counts}")
            if n == c["kn"]:
                short = [(what, got) for what, got in must if got < MIN_POP]
                assert not short, (variant, short)
                if variant == "rescale" and c["orc"].w >= 752:
                    assert sum(1 for k in counts["rescale"] if k.startswith("region")) == 3
    assert c["kn"] > 16385 or c["orc"].w < 752


def test_port_follows_the_reference(crafted):
    c = crafted
    pose = (c["V"], c["RVel"], c["RW0"])
    bad, checked = [], 0
    for variant in VARIANTS:
        for n in mapping_lengths(c["kn"]):
            lst, mask = cut_list(c["variants"][variant], c["mask"], n)
            ref = mapping_stages(c["orc"], c["slot"], lst, mask, c["retuned"], *pose)
            port = mapping_stages(c["port"], 0, lst, mask, c["retuned"], *pose)
            for st in ref:
                tag = f"{variant} n={n} {st}: "
                bad += [tag + m for m in depth_state_mismatches(port[st]["kl"], ref[st]["kl"])]
                for k in ("Kp", "RKp"):
                    if k in ref[st] and not scalar_close(port[st][k], ref[st][k]):
                        bad.append(tag + f"{k} {port[st][k]} vs {ref[st][k]}")
                if "r_num" in ref[st] and port[st]["r_num"] != ref[st]["r_num"]:
                    bad.append(tag + f"r_num {port[st]['r_num']} vs {ref[st]['r_num']}")
                checked += 1
    print(f"crafted {c['orc'].w}x{c['orc'].h}: port against reference, {checked} stage runs, {len(bad)} mismatches")
    assert not bad, f"{len(bad)} mismatches, first 25:\n" + "\n".join(bad[:25])
