"""CPU: stage A's gates, joins and threshold law on crafted images (tests/stage_a_crafted.py) — what the reference does on them,
that a plain restatement and oracle/port agree with it, that the set holds the populations a kernel can get wrong, and that
every entry of DEFECTS would show.  No kernel runs here; tests/test_stage_a_crafted_gpu.py runs the same set on the device.

Conditions that cannot be met are listed in UNREACHABLE with the search that was made; a population test that finds one of them
after all fails, so the list cannot go stale."""
import collections

import numpy as np
import pytest

import stage_a_crafted as sc

# name -> why, and the search that found nothing.  At most three may stand here.
UNREACHABLE = {
    "infinite_offset": "xs = -t0 t2 / (t0^2 + t1^2): a zero denominator needs t0 = t1 = 0, and then the numerator is 0 too -> NaN, never "
                       "inf; looked for among all pixels that reach the position gate in every case of the set: none",
    "negative_zero_dog": "DoG = img1 - img0 of two finite floats: a - a = +0 in round-to-nearest, and no other difference is zero; "
                         "looked for by sign bit in the DoG plane of every case: none",
}


def _all_cases():
    for g in sc.GROUPS:
        for label, over, names in sc.param_sets(g):
            for n in names:
                yield g, label, over, n


@pytest.fixture(scope="module")
def cases():
    """Every (parameter set, image) once: the reference's result and the restatement's, shared and left unchanged."""
    out = []
    for g, label, over, n in _all_cases():
        out.append(dict(group=g, label=label, over=over, image=n, ref=sc.ref_case(over, n), rs=sc.restated(over, n), p=sc.params_of(over)))
    return out


@pytest.fixture(scope="module")
def seq_runs():
    return {name: (over, frames, sc.run_oracle("ref", over, frames)) for name, (over, frames) in sc.sequences().items()}


def _same_stage_a(a, b, what):
    assert a["kn"] == b["kn"], f"{what}: kn {a['kn']} vs {b['kn']}"
    assert np.array_equal(a["mask"], b["mask"]), f"{what}: mask"
    for f in sc.STAGE_A_FIELDS:
        assert a["kl"][f].tobytes() == b["kl"][f].tobytes(), f"{what}: KeyLine.{f}"
    assert a["tresh"] == b["tresh"] and a["lkl"] == b["lkl"], f"{what}: threshold state"
    if a["kn"] > 0:     # kn == 0: the reference reads kl[0] of an empty list (edge_finder.cpp:376)
        assert np.float32(a["retuned"]).tobytes() == np.float32(b["retuned"]).tobytes(), f"{what}: reTunedThresh"


def test_image_set_and_parameter_sets_are_what_the_module_says():
    ims = sc.images()
    assert list(ims) == list(sc.IMAGE_NAMES) and len(ims) == 43
    for a in ims.values():
        assert a.shape == (sc.H, sc.W, 3) and a.dtype == np.uint8 and np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2])
    assert len({a.tobytes() for a in ims.values()}) == len(ims), "two names for one image"
    assert sc.W % 4 == 0 and sc.W % 16 != 0 and sc.H % 4 != 0 and sc.H % 12 != 0 and sc.W > 64


def test_pos_neg_thresholds_that_land_on_an_odd_integer():
    """|pn| is odd (25 signs), so 25 * PosNegThresh in float is reachable only where it is an odd integer: 0.2, 0.28, 0.36 and 1.0
    land on 5, 7, 9 and 25 exactly; the shipped 0.4 gives 10 (even: nothing sits on it) and 0.0 gives 0 (everything is rejected)."""
    got = {v: float(np.float32(25) * np.float32(v)) for v in sc.POS_NEG + (0.4,)}
    assert got == {0.0: 0.0, 0.2: 5.0, 0.28: 7.0, 0.36: 9.0, 1.0: 25.0, 0.4: 10.0}


def test_reference_twice_identical():
    for g in ("base", "euroc", "pos_neg_1.0", "cut:checker4"):
        for label, over, names in sc.param_sets(g):
            again = sc.run_oracle("ref", over, [sc.images()[n] for n in names])
            for n, b in zip(names, again):
                a = sc.ref_case(over, n)
                # every frame of `again` ran after another frame in the same context; with auto_gain = 0 nothing carries over
                assert a["kn"] == b["kn"] and np.array_equal(a["mask"], b["mask"]), (label, n)
                for f in sc.STAGE_A_FIELDS:
                    assert a["kl"][f].tobytes() == b["kl"][f].tobytes(), (label, n, f)
                for pl in a["planes"]:
                    assert a["planes"][pl].tobytes() == b["planes"][pl].tobytes(), (label, n, pl)
                assert a["tresh"] == b["tresh"] and a["lkl"] == b["lkl"], (label, n)
                assert a["kn"] == 0 or a["retuned"].tobytes() == b["retuned"].tobytes(), (label, n)


@pytest.mark.parametrize("kind", ["thr_g", "thr_d"])
def test_threshold_searches_find_a_value_on_most_images(kind):
    """Per image, a detector_thresh with thr_g exactly on a KeyLine pixel's dx^2 + dy^2, and a dog_thresh with thr_d exactly on a
    KeyLine's n2_m.  The two horizontal / vertical ramps have no KeyLine at the base threshold, so nothing to aim at there."""
    found = [n for n in sc.IMAGE_NAMES if sc.param_sets(f"{kind}:{n}")]
    missing = sorted(set(sc.IMAGE_NAMES) - set(found))
    assert missing == ["ramp_h", "ramp_v"], missing
    for n in found:
        (_, lo, _), (_, on, _), (_, hi, _) = sc.param_sets(f"{kind}:{n}")
        key = "detector_thresh" if kind == "thr_g" else "dog_thresh"
        assert np.float32(lo[key]) < np.float32(on[key]) < np.float32(hi[key]) and np.nextafter(np.float32(lo[key]), np.float32(np.inf)) == np.float32(on[key])


@pytest.mark.parametrize("group", sc.GROUPS)
def test_restatement_and_port_equal_the_reference(group):
    for label, over, names in sc.param_sets(group):
        port = sc.run_oracle("port", over, [sc.images()[n] for n in names])
        for n, pr in zip(names, port):
            ref = sc.ref_case(over, n)
            _same_stage_a(sc.restated(over, n), ref, f"restatement {label} {n}")
            _same_stage_a(pr, ref, f"port {label} {n}")
            for pl in ("img0", "img1", "dog"):
                assert pr["planes"][pl].tobytes() == ref["planes"][pl].tobytes(), f"port {label} {n}: plane {pl}"
            for pl in ("dx", "dy"):
                assert pr["planes"][pl][2:-2, 2:-2].tobytes() == ref["planes"][pl][2:-2, 2:-2].tobytes(), f"port {label} {n}: plane {pl}"


def test_threshold_law_sequences(seq_runs):
    """auto_gain > 0, frame after frame: the restatement's UpdateThresh and the port follow the reference, and the sequences hold the
    three clamp states, a clamp held for two frames running, and l_kl_num going through 0."""
    states, held, through_zero = set(), False, False
    for name, (over, frames, ref) in seq_runs.items():
        p = sc.params_of(over)
        port = sc.run_oracle("port", over, frames)
        prev = None
        for k, r in enumerate(ref):
            rs = sc.restate_stage_a(r["planes"], p, r["tresh_in"], r["lkl_in"])
            _same_stage_a(rs, r, f"restatement {name} frame {k}")
            _same_stage_a(port[k], r, f"port {name} frame {k}")
            st = sc.clamp_state(p, r["tresh"])
            states.add(st)
            held |= st != "inside" and st == prev
            prev = st
        lk = [r["lkl"] for r in ref]
        through_zero |= any(lk[i] > 0 and lk[j] == 0 and lk[k] > 0 for i in range(len(lk)) for j in range(i, len(lk)) for k in range(j, len(lk)))
    assert states == {"max", "min", "inside"} and held and through_zero
    inside = seq_runs["inside"][2]
    assert all(sc.clamp_state(sc.params_of(seq_runs["inside"][0]), r["tresh"]) == "inside" for r in inside)
    assert len({r["tresh"] for r in inside}) == len(inside)


def _populations(cases):
    c = collections.Counter()
    quad_probe = collections.Counter()
    for cs in cases:
        rs, ref, p = cs["rs"], cs["ref"], cs["p"]
        g = rs["gate"]
        for code in sc.GATE_NAMES:
            c[f"rejected by gate {code}"] += int((g == code).sum())
            c[f"passed on by gate {code}"] += int((g > code).sum())
        scanned = g != sc.UNSCANNED
        c["n2g == thr_g"] += int((scanned & (rs["n2g"] == rs["thr_g"])).sum())
        at_sign, at_pos, at_dog = g >= sc.G_SIGN, g >= sc.G_POS, g >= sc.G_DOGGRAD
        c["|pn| == pn_thr"] += int((at_sign & (np.abs(rs["pn"]) == rs["pn_thr"])).sum())
        half = (np.abs(rs["xs"]) == np.float32(0.5)) | (np.abs(rs["ys"]) == np.float32(0.5))
        c["|xs| or |ys| == 0.5f"] += int((at_pos & half).sum())
        c["|xs| or |ys| == 0.5f and a KeyLine"] += int(((g == sc.KEYLINE) & half).sum())
        c["n2_m == thr_d"] += int((at_dog & (rs["n2m"] == rs["thr_d"])).sum())
        nan = np.isnan(rs["xs"]) | np.isnan(rs["ys"])
        c[f"NaN offset at pos_neg {p.pos_neg_thresh}"] += int((at_pos & nan).sum())
        c["infinite offset"] += int((at_pos & (np.isinf(rs["xs"]) | np.isinf(rs["ys"]))).sum())
        c["zero DoG inside a fitted window"] += int((at_pos & rs["win_has_zero"]).sum())
        c["-0 in the DoG plane"] += int((np.signbit(ref["planes"]["dog"]) & (ref["planes"]["dog"] == 0)).sum())
        kl = ref["kl"]
        nid = kl["n_id"][kl["n_id"] >= 0]
        c["KeyLines named as n_id by several"] += int((np.bincount(nid, minlength=1) > 1).sum())
        c["m_m.x == 0 or m_m.y == 0"] += int(((kl["m_m"][:, 0] == 0) | (kl["m_m"][:, 1] == 0)).sum())
        c["max_dog == min_dog with kn > 0"] += int(len(kl) > 0 and kl["n_m"].max() == kl["n_m"].min())
        c["kn == 0"] += int(len(kl) == 0)
        for q, pr in zip(rs["quad"], rs["probe"]):
            quad_probe[(int(q), int(pr))] += 1
        if rs["uncut"] >= p.max_points:
            where = "first" if p.max_points == 1 else "last" if p.max_points == rs["uncut"] else "middle"
            c[f"cut on the {where} KeyLine"] += 1
    return c, quad_probe


def test_population_conditions(cases, seq_runs):
    """Asserted on the reference (the restatement only says which gate decided, after the test above held it to the reference)."""
    c, quad_probe = _populations(cases)
    for k in sorted(c):
        print(f"{k}: {c[k]}")
    print("NextPoint (quadrant, probe):", sorted(quad_probe.items()))
    print("cases:", len(cases))
    for code in sc.GATE_NAMES:
        assert c[f"rejected by gate {code}"] > 0 and c[f"passed on by gate {code}"] > 0, sc.GATE_NAMES[code]
    for k in ("n2g == thr_g", "|pn| == pn_thr", "|xs| or |ys| == 0.5f", "n2_m == thr_d", "NaN offset at pos_neg 0.4", "NaN offset at pos_neg 1.0",
              "|xs| or |ys| == 0.5f and a KeyLine", "max_dog == min_dog with kn > 0", "zero DoG inside a fitted window", "KeyLines named as n_id by several", "m_m.x == 0 or m_m.y == 0",
              "cut on the first KeyLine", "cut on the middle KeyLine", "cut on the last KeyLine"):
        assert c[k] > 0, k
    for q in range(4):
        for pr in range(3):
            assert quad_probe[(q, pr)] > 0, f"NextPoint quadrant {q} never answers with probe {pr}"
    assert c["infinite offset"] == 0 and c["-0 in the DoG plane"] == 0, "listed in UNREACHABLE, but found: take it off the list and test it"
    assert len(UNREACHABLE) <= 3


@pytest.mark.parametrize("defect", sorted(sc.DEFECTS))
def test_every_defect_shows_on_some_case(defect, cases, seq_runs):
    """A defect counts as seen when the mutated restatement's mask, a stage-A KeyLine field or the threshold state differs from the
    reference's on at least one case — the very quantities the GPU test compares."""
    def differs(rs, ref):
        if rs["kn"] != ref["kn"] or not np.array_equal(rs["mask"], ref["mask"]) or rs["tresh"] != ref["tresh"] or rs["lkl"] != ref["lkl"]:
            return True
        return any(rs["kl"][f].tobytes() != ref["kl"][f].tobytes() for f in sc.STAGE_A_FIELDS)

    if defect == "clamp_before_gain":
        for name, (over, frames, ref) in seq_runs.items():
            p = sc.params_of(over)
            if any(differs(sc.restate_stage_a(r["planes"], p, r["tresh_in"], r["lkl_in"], defect), r) for r in ref):
                return
        pytest.fail(defect)
    n = 0
    for cs in cases:
        ref = cs["ref"]
        if differs(sc.restate_stage_a(ref["planes"], cs["p"], ref["tresh_in"], ref["lkl_in"], defect), ref):
            n += 1
            if n >= 2:
                break
    assert n >= 1, f"{defect} ({sc.DEFECTS[defect]}) changes nothing on any case"
