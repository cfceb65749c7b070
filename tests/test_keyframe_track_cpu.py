"""Key-frame match repair (TrackKeyFrames), CPU: the plain-Python port against the fixtures the reference's own kfvo.cpp produced
(tests/golden/keyframe_track, tools/make_keyframe_track_golden.py), and the component-ordered form of phase 2 — what the device runs —
against the serial form."""
import os
import random

import numpy as np
import pytest

import keyframe_track_port as port

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_track")


def crafted_cases():
    z = np.load(os.path.join(GOLD, "crafted.npz"))
    out = {}
    for name in z["names"]:
        pre = f"{name}_"
        out[str(name)] = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    return out


def chained_cases():
    z = np.load(os.path.join(GOLD, "chained.npz"))
    out = {}
    for k in range(1, int(z["n_frames"])):
        c = {key[len(f"f{k}_"):]: z[key] for key in z.files if key.startswith(f"f{k}_")}
        kf = int(c["kf"])
        for key in ("p_m", "p_id", "n_id", "Pose", "Pos"):
            c[f"kf_{key}"] = z[f"kf{kf}_{key}"]
        c.update(zf=z["zf"], dist_thresh=z["dist_thresh"], dist_tolerance=z["dist_tolerance"], augmentate=np.int32(1))
        out[f"f{k}"] = c
    return out, z


def run_port(case, order="serial", rng=None):
    kf = {k: case[f"kf_{k}"] for k in ("p_m", "p_id", "n_id", "m_id_f", "Pose", "Pos")}
    new = {k: case[f"new_{k}"] for k in ("p_m", "p_id", "n_id", "m_id", "m_id_kf")}
    st = port.Stats()
    out = {}
    out["m_id_f_0"], out["fow_m0"] = port.build_forward_match(kf["m_id_f"], new["m_id"], int(case["old_kn"]))
    kf1 = dict(kf, m_id_f=out["m_id_f_0"])
    args = (case["Pose"], case["Pos"], float(case["zf"]), float(case["dist_thresh"]), float(case["dist_tolerance"]), bool(case["augmentate"]))
    out["m_id_f_1"], out["fow_m"], g1 = port.forward_correct_augmentate(kf1, new, *args, order=order, rng=rng, stats=st)
    out["m_id_kf_1"], out["back_m"], g2 = port.back_correct_augmentate(kf, new, *args, order=order, rng=rng, stats=st)
    out["guard"] = g1 | g2
    return out, st


ALL = dict(crafted_cases())
ALL.update(chained_cases()[0])
SMALL = [n for n in sorted(ALL) if n != "BIG"]   # (20000 KeyLines in pure Python: checked once, in the serial form, below)


def equals_reference(out, case):
    assert out["guard"] == 0
    assert np.array_equal(out["m_id_f_0"], case["ref_m_id_f_0"])
    assert np.array_equal(out["m_id_f_1"], case["ref_m_id_f_1"])
    assert np.array_equal(out["m_id_kf_1"], case["ref_m_id_kf_1"])
    assert [out["fow_m0"], out["fow_m"], out["back_m"]] == [int(v) for v in case["ref_counts"]]


@pytest.mark.parametrize("name", sorted(ALL))
def test_port_equals_the_reference(name):
    out, st = run_port(ALL[name])
    equals_reference(out, ALL[name])
    # the branch populations stored with the fixture are the ones this run sees
    for k, v in zip(ALL[name]["stat_names"], ALL[name]["stat_values"]):
        if k not in ("fan_in", "cycle", "self_link", "duplicate_m_id"):
            assert st.get(str(k), 0) == int(v), k


@pytest.mark.parametrize("name", SMALL)
def test_component_order_equals_the_reference(name):
    for seed in range(3):   # components in three different orders
        out, _ = run_port(ALL[name], order="components", rng=random.Random(seed))
        equals_reference(out, ALL[name])


def test_crafted_fixtures_populate_every_branch():
    c = crafted_cases()
    need = ("slide_along_n", "slide_along_p", "slide_stop_chain_end", "slide_stop_non_decrease", "walk_stop_missing_link",
            "walk_stop_matched", "walk_stop_failed_correction", "filled_after_failure_from_other_side", "walk_met_other_seed_fill",
            "far_seed_propagated", "fan_in", "cycle", "self_link", "duplicate_m_id")
    for name, extra in (("A", ()), ("B", ("slide_tolerance_at_once", "slide_stop_tolerance"))):
        st = dict(zip((str(k) for k in c[name]["stat_names"]), c[name]["stat_values"]))
        assert all(st.get(k, 0) > 0 for k in need + extra), (name, st)
    assert float(c["B"]["dist_tolerance"]) > 0
    assert not np.any(np.asarray(c["E0"]["Pos"])) and [len(c[n]["kf_p_id"]) for n in ("K00", "K01", "K10", "K11")] == [0, 0, 1, 1]
    assert all(np.isfinite(v["kf_p_m"]).all() and np.isfinite(v["new_p_m"]).all() for v in c.values())


def test_chained_fixture_inserts_by_the_criterion():
    cases, z = chained_cases()
    ins = list(z["inserts"])
    assert ins[0] == 0 and len(ins) >= 2
    for k in range(1, int(z["n_frames"])):
        c = cases[f"f{k}"]
        crit = int(c["ref_counts"][2]) < min(int(z["track_points"]), len(c["new_p_id"])) * float(z["kf_save_percent"])
        assert crit == bool(c["inserted"]) == (k in ins)
        if k > 1 and (k - 1) not in ins:   # the key-frame state of one frame is the next frame's input
            assert np.array_equal(c["kf_m_id_f"], cases[f"f{k - 1}"]["ref_m_id_f_1"])
    assert any(not bool(cases[f"f{k}"]["inserted"]) for k in range(1, int(z["n_frames"])))


def random_graph_case(seed):
    """Random functional p_id / n_id (any link graph: fan-in, cycles, self-links, links that are not mutual), random p_m, random seeds."""
    rs = np.random.RandomState(seed)
    kn_own, kn_oth = rs.randint(1, 60), rs.randint(1, 60)

    def lst(kn):
        link = lambda: np.where(rs.rand(kn) < 0.75, rs.randint(0, kn, kn), -1).astype(np.int32)
        return rs.uniform(-40, 40, (kn, 2)).astype(np.float32), link(), link()
    own, oth = lst(kn_own), lst(kn_oth)
    m = np.where(rs.rand(kn_own) < 0.25, rs.randint(0, kn_oth, kn_own), -1).astype(np.int32)
    E = rs.normal(size=9) * (rs.rand() > 0.05)
    return own, oth, m, E, float(rs.choice([3.0, 10.0, 40.0])), float(rs.choice([0.0, 0.0, 2.0]))


def test_component_order_equals_serial_order_on_random_link_graphs():
    differ = 0
    for seed in range(400):
        own, oth, m, E, thresh, tol = random_graph_case(seed)
        a = port.correct_augment(*own, m, *oth, E, 420.0, thresh, tol, True, order="serial")
        b = port.correct_augment(*own, m, *oth, E, 420.0, thresh, tol, True, order="components", rng=random.Random(seed))
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], seed
        # (the order matters on these graphs: a reversed serial loop gives other matches on many of them)
        n = len(m)
        rev = port.correct_augment(own[0][::-1], np.where(own[1] >= 0, n - 1 - own[1], -1)[::-1], np.where(own[2] >= 0, n - 1 - own[2], -1)[::-1],
                                   m[::-1], *oth, E, 420.0, thresh, tol, True, order="serial")
        differ += not np.array_equal(rev[0][::-1], a[0])
    assert differ > 20, differ


def test_components_are_labelled_by_their_minimum_index():
    p = np.array([-1, 0, 1, -1, 5, 4, 6, -1], np.int32)    # 0-1-2 | 3 | 4<->5 cycle | 6 self | 7 -> 3 by n
    n = np.array([1, 2, -1, -1, 5, 4, 6, 3], np.int32)
    assert port.components(list(p), list(n), 8) == [0, 0, 0, 3, 4, 4, 6, 3]


def test_walk_cap_sets_guard_on_a_nan_cycle_and_returns():
    # a two-KeyLine n_id cycle in the other list with NaN p_m: `d >= d0` is never true, the reference would slide for ever
    oth = (np.array([[np.nan, 0.0], [np.nan, 1.0], [5.0, 5.0]], np.float32), np.array([-1, -1, -1], np.int32), np.array([1, 0, -1], np.int32))
    own = (np.array([[1.0, 2.0]], np.float32), np.array([-1], np.int32), np.array([-1], np.int32))
    E = [0.0, -0.02, 0.1, 0.02, 0.0, -0.3, -0.1, 0.3, 0.0]
    m, count, guard = port.correct_augment(*own, np.array([2], np.int32), *oth, E, 420.0, 10.0, 0.0, True)
    assert guard == 0 and m[0] == 2   # finite walk: no guard
    oth_nan = (oth[0], oth[1], np.array([1, 0, 0], np.int32))   # KeyLine 2 now leads into the cycle
    big = np.array([[np.nan, 0.0], [np.nan, 1.0], [500.0, 500.0]], np.float32)
    m, count, guard = port.correct_augment(*own, np.array([0], np.int32), big, oth_nan[1], oth_nan[2], E, 420.0, 10.0, 0.0, True)
    assert guard == 0   # a NaN first distance never starts a slide (`d < d0` is false)
    # start on the finite KeyLine: its n neighbour's distance is NaN, `d < d0` false -> no slide either; the cycle is entered only through
    # a finite, strictly smaller distance followed by NaNs: KeyLine 0 finite and close, KeyLines 1 <-> 2 NaN behind it
    pm = np.array([[1.0, 2.0], [np.nan, 0.0], [np.nan, 1.0], [300.0, 300.0]], np.float32)
    nid = np.array([1, 2, 1, 0], np.int32)
    m, count, guard = port.correct_augment(*own, np.array([3], np.int32), pm, np.full(4, -1, np.int32), nid, E, 420.0, 10.0, 0.0, True)
    assert guard == 1 and count in (0, 1)
