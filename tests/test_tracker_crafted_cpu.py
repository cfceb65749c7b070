"""The crafted tracker lists reach what they claim — the reference alone (no GPU).

tests/tracker_crafted.py edits a donor pair (family A) and builds an exact grid (family B) so that TryVelRot's "last valid fi" carry runs
over whole waves, whole 256-KeyLine blocks and two blocks, starts at KeyLine 0, and so that every gate is met on its threshold.  Here every
variant, cut and class goes through the two-pass protocol of tests/test_tracker_crafted_gpu.py on the reference, every old KeyLine is
classified from the reference's own outputs (skipped: the gate on the inputs; out of image: r == max_r and m_id_f == -1; matched:
m_id_f >= 0; otherwise unmatched in the image), and the claims are asserted:

  * every run of `runs`, `head`, `tail`, `hole` has its stated length and position under every pose and cut, is bounded by matched
    KeyLines, and the reference's residual inside it IS the bounding KeyLine's (0 for the run that starts at KeyLine 0); the interleaved
    run alternates unmatched, skipped and out-of-image KeyLines and inherits across them;
  * `hole` leaves blocks 2 and 3 without a match, `none` matches nothing;
  * `gates`: the KeyLines on the s_rho gate and one double below are evaluated, one double above is skipped; m_num = -1 is never skipped
    (it compares as 4294967295), m_num 0 / 1 follow min(MatchNumThresh, FrameCount);
  * `record`: the detector's list passes the host's consistency expression (numpy float32), the edited one fails it in one KeyLine, and
    the reference's residuals differ between the two lists;
  * family B: every old KeyLine matches the new KeyLine it is aimed at (the reference's field() holds that index at that pixel) with the
    residual predicted from p_m + pp exactly — the projection is exact —, every class has 8 members or more, and the Huber requests sit
    on a positive, a negative and an inherited first-pass residual;
  * the reference's minimisers are stable on every list the GPU test runs them on: two runs from starts 1e-12 apart (Minimizer_RV)
    agree within a tenth of the GPU test's tolerance.  Minimizer_V returns its start when iter_max = 0 and its absolute tolerance on V is
    1e-12, so a start moved by 1e-12 cannot agree within a tenth of that; its screen moves the start by 1e-16 instead.

The whole file runs in a few seconds; it prints its populations and its time.
"""
import time

import numpy as np
import pytest

import tracker_crafted as tc
from helpers import require_ref

SPENT = [0.0]                     # seconds inside this file's tests and fixtures (not since import: the suite collects every file first)


@pytest.fixture(autouse=True)
def _clock():
    t = time.perf_counter()
    yield
    SPENT[0] += time.perf_counter() - t


@pytest.fixture(scope="module")
def fam_a():
    require_ref()
    t = time.perf_counter()
    fam = tc.family_a()
    SPENT[0] += time.perf_counter() - t
    return fam


@pytest.fixture(scope="module")
def ref_b():
    orc = tc.make_reference_b(require_ref())
    yield orc
    orc.close()


def _load_a(fam, name, n, new=None):
    kl, m = tc.cut(fam["variants"][name], fam["old_mask"], n)
    fam["orc"].set_keylines(fam["so"], kl, m, fam["old_retuned"])
    return kl


def _statuses(fam, kl, X, mnt=0, fc=0):
    """Both passes in all four modes -> (status of pass 1, status of pass 2, pass 1, pass 2 of the first mode); the classification and
    the residual memory do not depend on the mode."""
    orc, so, sn, gate = fam["orc"], fam["so"], fam["sn"], fam["gate"]
    orc.set_framecount(sn, fc)
    first = None
    for rw, jf in tc.MODES:
        p1, p2 = tc.two_pass(orc, sn, so, X, gate, mnt, rw, jf)
        s1, s2 = tc.classify(kl, p1, gate, mnt, fc), tc.classify(kl, p2, gate, mnt, fc)
        if first is None:
            first = (s1, s2, p1, p2)
        else:
            assert np.array_equal(s2, first[1]) and np.array_equal(p2["r"], first[3]["r"]) and np.array_equal(p2["mid"], first[3]["mid"])
    orc.set_framecount(sn, 0)
    return first


def _check_run(st, r, start, L, kind, n, tag):
    """One run of the layout in a list of n KeyLines, on the statuses and the reference's residuals of one evaluation."""
    if start >= n:
        return 0
    end = min(start + L, n)
    want = r[start - 1] if start > 0 else 0.0
    if start > 0:
        assert st[start - 1] == tc.MATCHED, (tag, "the KeyLine before the run is not matched")
    if end < n and end == start + L:
        assert st[end] == tc.MATCHED, (tag, "the KeyLine behind the run is not matched")
    seg = st[start:end]
    if kind == "mixed":
        j = np.arange(end - start)
        assert np.array_equal(seg, np.where(j % 4 < 2, tc.UNMATCHED, np.where(j % 4 == 2, tc.SKIPPED, tc.OUT))), tag
        assert np.all(r[start:end][seg == tc.UNMATCHED] == want), (tag, "the carry does not pass skipped / out-of-image KeyLines")
        assert np.all(r[start:end][seg == tc.OUT] == tc.MAX_R)
    else:
        assert np.all(seg == tc.UNMATCHED), (tag, np.nonzero(seg != tc.UNMATCHED)[0][:5] + start)
        assert np.all(r[start:end] == want), (tag, "the run does not inherit the residual of the KeyLine before it")
    return int((seg == tc.UNMATCHED).sum())


def test_layout_of_the_runs(fam_a):
    layout = fam_a["runs"]["runs"]
    for kind in ("aligned", "odd"):
        assert sorted(L for _, L, k in layout if k == kind) == sorted(tc.RUN_LENGTHS)
    assert all(s % tc.BLOCK == 0 for s, _, k in layout if k == "aligned")
    assert all(s % 2 == 1 and s % tc.BLOCK != 0 for s, _, k in layout if k != "aligned")
    assert sum(k == "mixed" for _, _, k in layout) == 1
    ends = [(s, s + L) for s, L, _ in layout]
    assert all(b[0] > a[1] for a, b in zip(ends, ends[1:])), "runs must be separated by a KeyLine"
    assert fam_a["copied"]["none"] < 200 and all(v < 200 for v in fam_a["copied"].values()), fam_a["copied"]
    print("family A: kn", len(fam_a["old"]), "anchors' sources", len(fam_a["robust"]), "copies in place of turns", fam_a["copied"])


@pytest.mark.parametrize("name", ["runs", "head", "tail", "hole"])
def test_runs_have_their_length_and_position(fam_a, name):
    seen = 0
    for n in tc.CUTS:
        kl = _load_a(fam_a, name, n)
        for pi, X in enumerate(fam_a["poses"]):
            s1, s2, p1, p2 = _statuses(fam_a, kl, X)
            for st, ev in ((s1, p1), (s2, p2)):
                got = set(tc.carry_runs(st))
                for start, L, kind in fam_a["runs"][name]:
                    cnt = _check_run(st, ev["r"], start, L, kind, len(kl), (name, n, pi, start, L))
                    if cnt and kind != "mixed":
                        end = min(start + L, len(kl))
                        assert (start, end - 1, end - start) in got, (name, n, pi, start, L)
                    seen += cnt
                if name == "hole" and len(kl) >= 1024:
                    assert not np.any(st[2 * tc.BLOCK:4 * tc.BLOCK] == tc.MATCHED), "hole: blocks 2 and 3 must hold no match"
                    assert st[tc.HOLE[0]:tc.HOLE[1] + 1].tolist() == [tc.UNMATCHED] * (tc.HOLE[1] + 1 - tc.HOLE[0])
                if name == "head":
                    assert np.all(ev["r"][:min(tc.HEAD_LEN, len(kl))] == 0.0)            # the initial fi = 0
                if name == "tail" and len(kl) > tc.TAIL_START:
                    assert np.all(st[tc.TAIL_START:] == tc.UNMATCHED)
    print(f"{name}: {seen} unmatched KeyLines in runs over all cuts, poses and passes")
    assert seen > 0


def test_none_matches_nothing_and_plain_is_the_donor(fam_a):
    for n in tc.CUTS:
        kl = _load_a(fam_a, "none", n)
        for X in fam_a["poses"]:
            s1, s2, p1, p2 = _statuses(fam_a, kl, X)
            assert not np.any(s1 == tc.MATCHED) and not np.any(s2 == tc.MATCHED)
            assert np.all(p2["r"][s2 == tc.UNMATCHED] == 0.0)
    kl = _load_a(fam_a, "plain", None)
    s1, s2, _, _ = _statuses(fam_a, kl, fam_a["poses"][1])
    pop = np.bincount(s2, minlength=4)
    print("plain: skipped, out, matched, unmatched =", pop.tolist())
    assert pop[tc.MATCHED] > 0.6 * len(kl) and pop[tc.SKIPPED] > 100 and pop[tc.UNMATCHED] > 100


def test_gates_on_their_thresholds(fam_a):
    sets, gate = fam_a["gate_sets"], fam_a["gate"]
    assert all(len(v) == tc.GATE_POP for v in sets.values()) and len(np.unique(np.concatenate(list(sets.values())))) == tc.GATE_POP * len(sets)
    full = fam_a["variants"]["gates"]
    assert np.all(full["s_rho"][sets["s_rho_at"]] == gate) and np.all(full["s_rho"][sets["s_rho_above"]] > gate)
    assert np.all(full["s_rho"][sets["s_rho_below"]] < gate)
    for n in tc.CUTS:
        kl = _load_a(fam_a, "gates", n)
        for fc in tc.GATES_FC:
            thr = min(tc.GATES_MNT, fc)
            for X in fam_a["poses"]:
                s1, s2, p1, p2 = _statuses(fam_a, kl, X, tc.GATES_MNT, fc)
                for name, idx in sets.items():
                    idx = idx[idx < len(kl)]
                    if name.startswith("m_num"):
                        v = int(name.split("_")[-1])
                        skipped = v >= 0 and v < thr                      # -1 compares as 4294967295: never skipped
                    else:
                        skipped = name == "s_rho_above"
                    for st, ev in ((s1, p1), (s2, p2)):
                        if skipped:                                       # the reference never touches a skipped KeyLine's entry (0 from the harness)
                            assert np.all(st[idx] == tc.SKIPPED) and np.all(ev["mid"][idx] == -1) and np.all(ev["r"][idx] == 0.0), (name, fc, n)
                        else:                                             # the sets are KeyLines that match under every pose
                            assert np.all(st[idx] == tc.MATCHED), (name, fc, n)
    pops = {name: int((idx < 255).sum()) for name, idx in sets.items()}
    print("gates: members of each set inside the first 255 KeyLines", pops)
    assert all(v >= 1 for v in pops.values())


def test_record_fails_the_hosts_consistency_expression_in_one_keyline(fam_a):
    orc, so, sn, gate = fam_a["orc"], fam_a["so"], fam_a["sn"], fam_a["gate"]
    rec = fam_a["record"]
    assert tc.consistent_u_m(fam_a["new"]).all()
    bad = np.nonzero(~tc.consistent_u_m(rec["new"]))[0]
    assert bad.tolist() == [rec["index"]]
    diff = fam_a["new"]["u_m"].view(np.int32) - rec["new"]["u_m"].view(np.int32)
    assert np.abs(diff).sum() == 1                                                      # one float, one ulp
    try:
        for n in tc.CUTS:
            kl = _load_a(fam_a, "plain", n)
            out = []
            for new in (fam_a["new"], rec["new"]):
                orc.set_keylines(sn, new, fam_a["new_mask"], fam_a["new_retuned"])
                orc.build_field(sn, tc.MAX_R, fam_a["new_retuned"])
                out.append(tc.two_pass(orc, sn, so, np.zeros(6), gate, 0, True, True)[1])
            seen = np.nonzero(out[0]["mid"] == rec["index"])[0]
            assert np.array_equal(out[0]["mid"], out[1]["mid"])
            if n is None or n >= 255:
                assert len(seen) >= 1, n
                assert np.all(out[0]["r"][seen] != out[1]["r"][seen]), "the reference must read the stored u_m"
        print("record: new KeyLine", rec["index"], "matched by old KeyLines", seen.tolist(), "of the full list")
    finally:
        orc.set_keylines(sn, fam_a["new"], fam_a["new_mask"], fam_a["new_retuned"])
        orc.build_field(sn, tc.MAX_R, fam_a["new_retuned"])


@pytest.mark.parametrize("salt", [0, 1, 2])
def test_family_b_is_exact(ref_b, salt):
    fam = tc.family_b(salt)
    cls, exp = fam["cls"], fam["expect"]
    pop = {c: int((cls == c).sum()) for c in tc.CLASSES_B}
    assert all(v >= tc.MIN_POP for v in pop.values()), pop
    b = cls == "border"
    assert (exp[b] >= 0).sum() >= tc.MIN_POP and (exp[b] == -2).sum() >= tc.MIN_POP
    t = cls == "test_f_k"
    assert (exp[t] >= 0).sum() == (exp[t] == -1).sum() == 8
    assert np.all(np.abs(fam["old"]["rho"]) == 2.0 ** np.round(np.log2(np.abs(fam["old"]["rho"])))) and (fam["old"]["rho"] < 0).sum() >= tc.MIN_POP
    c0, c1 = fam["carry"]
    assert c0 // tc.BLOCK + 2 == c1 // tc.BLOCK and fam["fi"][c0 - 1] != 0           # the run crosses two block boundaries
    for n in tc.CUTS:
        kl = tc.load_b(ref_b, fam, n)
        k = len(kl)
        field = ref_b.field(1)[..., 1]
        new = fam["new"]
        assert np.array_equal(field[new["c_p"][:, 1].astype(int), new["c_p"][:, 0].astype(int)], np.arange(len(new)))
        for rw, jf in tc.MODES:
            p1, p2 = tc.two_pass(ref_b, 1, 0, np.zeros(6), tc.GATE_B, 0, rw, jf)
            for ev in (p1, p2):
                st = tc.classify(kl, ev, tc.GATE_B, max_r=tc.MAX_R_B)
                assert np.array_equal(ev["mid"], np.where(exp[:k] >= 0, exp[:k], -1))
                assert np.array_equal(st, np.where(exp[:k] >= 0, tc.MATCHED, np.where(exp[:k] == -1, tc.UNMATCHED, tc.OUT)))
                m = exp[:k] >= 0
                assert np.array_equal(ev["r"][:k][m], fam["fi"][:k][m]), "the projection is not exact"
                if k > c0:
                    assert np.all(ev["r"][c0:min(c1 + 1, k)] == fam["fi"][c0 - 1])
    reqs = tc.huber_requests(ref_b, fam)
    assert [kind for _, _, kind in reqs[::3]] == ["positive", "negative", "inherited"]
    assert all(reqs[j][0] > reqs[j + 1][0] and reqs[j][0] < reqs[j + 2][0] for j in (0, 3, 6))
    print(f"family B, salt {salt}: {len(fam['old'])} old, {len(fam['new'])} new KeyLines, classes {pop}, Huber on KeyLines {[i for _, i, _ in reqs[::3]]}")


def test_the_references_minimisers_are_stable_on_the_chosen_lists(fam_a):
    n_rv = n_v = 0
    for k, job in enumerate(tc.rv_jobs()):
        start = tc.rv_start(fam_a, job, k)
        for init_type in (0, 1, 2):
            a = tc.ref_minimizer_rv(fam_a, job, start, init_type)
            b = tc.ref_minimizer_rv(fam_a, job, start + 1e-12, init_type)
            assert tc.rv_agree(b, a, 0.1) == [], (job, init_type)
            assert np.array_equal(a["mid"], b["mid"]), (job, init_type)
            n_rv += 1
    for iter_max, min_mod in tc.V_REQUESTS:
        for V0 in tc.V_STARTS:
            for job in tc.v_jobs():
                a = tc.ref_minimizer_v(fam_a, job, np.array(V0), iter_max, min_mod)
                b = tc.ref_minimizer_v(fam_a, job, np.array(V0) + 1e-16, iter_max, min_mod)
                assert tc.v_agree(b, a, 0.1) == [], (job, V0, iter_max, min_mod)
                assert np.array_equal(a["mid"], b["mid"])
                n_v += 1
    old = fam_a["variants"]["behind"]
    assert sum(hi - lo for lo, hi in tc.BEHIND) >= tc.BLOCK and all(np.all(1.0 / old["rho"][lo:hi] + 2e-3 <= 0) for lo, hi in tc.BEHIND)
    dropped = int((fam_a["old"]["n_m"] < 1.5).sum())
    assert 100 < dropped < len(old) // 2
    print(f"minimisers: {n_rv} Minimizer_RV and {n_v} Minimizer_V requests stable; min_mod = 1.5 drops {dropped} KeyLines; seeds replaced: {tc.RV_SEED}")


def test_zz_time():
    dt = SPENT[0]
    print(f"tests/test_tracker_crafted_cpu.py: {dt:.1f} s")
    assert dt < 60
