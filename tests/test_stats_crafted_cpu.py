"""The crafted lists of tests/stats_crafted.py reach what they claim — the reference alone (no GPU).

EstimateQuantile
  * which bin every special value lands in, from the reference's own answer for a list that holds that value alone (pct = 0: the answer is
    the edge of the bin after it): NaN, +-inf, 1e300 and 4.3e8 land in bin 0 (the x86-64 conversion gives INT_MIN), everything at or above
    smax in the last bin, everything below smin in bin 0; a value on a bin edge lands wherever the reference's expression puts it, which
    the restatement reproduces — no bin is assumed;
  * the quantile moves when enough of such values are added to a list that is short of its threshold by one;
  * `threshold`: the balanced and the tipped list of every length differ, the balanced one answers beyond the gap; pct * L is an integer in
    double where the case says it is; losing the KeyLine at any stride boundary moves the tipped list's answer, reading one more moves the
    balanced one's;
  * all_last -> 1e3, all_first -> the edge of bin 1, empty -> 1e3;
  * the restatement without a defect and the port equal the reference bit for bit on every list and every (nbins, pct);
  * every named defect changes the answer of at least one list.  One exception is proved instead: `clamp_order`, the two integer clamps
    swapped, is the same function for every nbins >= 1 (0 <= nbins - 1, so the two clamps commute) and nbins < 1 is refused by the entry
    point; what a reordering can break is the clamp moved in front of the conversion (`clamp_before_convert`), which the cases catch.
reEstimateThresh
  * the float32 histogram of the reference's own KeyLines reproduces reTunedThresh at the default TrackPoints and at every crafted one, through
    stage_a and through process_frame on the reference, through stage_a on the port, at 100 and 256 bins; the walk ends on the bin each value is meant to reach; both defects are caught.
ExtRotVel
  * every claim of erv_list(): rows, rank, eigenvalue gaps (no eigenvalue of the reference's Wx between s_max / 1e10 and s_max / 1e8), cond <= 1e6
    for the full-rank lists, ok and the non-finite pattern of the pole lists; the restatement and the port pass the GPU test's own comparison;
    every named defect fails it on at least one list; no bound exceeds 1e-4 of its solution's size; every loner moves X by 100 bounds or more (the last two
    on the reference and on the port); every variant meets all three velocities, `pole` with a finite rho at a non-zero vel[2], `s_rho` = inf at the zero velocity.

The whole file runs in a few seconds; it prints its populations and its time.
"""
import time

import numpy as np
import pytest

import stats_crafted as sc
from helpers import require_ref

SPENT = [0.0]


@pytest.fixture(autouse=True)
def _clock():
    t = time.perf_counter()
    yield
    SPENT[0] += time.perf_counter() - t


@pytest.fixture(scope="module")
def orcs():
    oracle = require_ref()
    o = {k: oracle.Oracle(k, sc.params(oracle), nslots=2) for k in ("ref", "port")}
    yield o
    for v in o.values():
        v.close()


def _q(orc, s_rho, pct, n):
    orc.set_keylines(0, sc.quantile_keylines(np.asarray(s_rho, np.float64)))
    return orc.quantile(0, sc.SMIN, sc.SMAX, pct, n)


def _bin_of(orc, v, n=100):
    """The bin the reference puts v in, from its answer for the list [v] at pct = 0 (None: the last bin, whose answer is 1e3)."""
    a = _q(orc, [v], 0.0, n)
    if a == 1e3:
        return n - 1
    i = [k for k in range(1, n) if sc.bin_edge(k, n) == a]
    assert len(i) == 1, (v, a)
    return i[0] - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# EstimateQuantile
# ---------------------------------------------------------------------------------------------------------------------------------
def test_special_values_land_where_the_reference_puts_them(orcs):
    ref = orcs["ref"]
    where = {}
    for name, v in sc.CLAMP_VALUES:
        where[name] = _bin_of(ref, v)
        assert where[name] == int(sc.quantile_bins(np.array([v]), sc.SMIN, sc.SMAX, 100)[0]), name
    for name in ("-0.0", "0.0", "just below smin", "truncates to 0", "bin -1", "large negative", "-inf"):
        assert where[name] == 0, (name, where[name])
    for name in ("smax", "above smax", "2 smax"):
        assert where[name] == 99, (name, where[name])
    for name in ("4.3e8", "1e300", "+inf", "NaN"):                       # INT_MIN, clamped to bin 0: NOT the last bin
        assert where[name] == 0, (name, where[name])
        assert int(sc.quantile_bins(np.array([dict(sc.CLAMP_VALUES)[name]]), sc.SMIN, sc.SMAX, 100, "saturating")[0]) != 0 or name == "NaN"
    print("bins of the clamp values:", where)
    # a list one KeyLine short of its threshold: ten KeyLines in the last bin, pct = 0.5; ten more of v leave a = 10 > 10 false, eleven tip it
    for name in ("4.3e8", "1e300", "+inf", "-inf", "NaN", "large negative"):
        v = dict(sc.CLAMP_VALUES)[name]
        last = [sc.filler(100)] * 10
        assert _q(ref, last + [v] * 10, 0.5, 100) == 1e3, name
        assert _q(ref, last + [v] * 11, 0.5, 100) == sc.bin_edge(1, 100), name
    # edges: whatever bin the reference chooses, the restatement chooses it too; and some edge value does not fall in "its" bin i
    off, n_edges = [], 0
    for n in sc.Q_NBINS:
        for name, v in sc.edge_values(n):
            if n == 1:
                continue                                               # one bin: every answer is 1e3
            b = _bin_of(ref, v, n)
            assert b == int(sc.quantile_bins(np.array([v]), sc.SMIN, sc.SMAX, n)[0]), (name, n)
            n_edges += 1
            if not name.endswith(("+", "-")):
                i = int(name.split()[1].split("/")[0])
                if b != min(i, n - 1):
                    off.append((name, b))
    print(f"{n_edges} edge values; on-edge doubles that the reference puts below their own bin: {off}")


def test_threshold_lists_sit_on_their_threshold(orcs):
    ref = orcs["ref"]
    exact = {0.5: 0, 0.9: 0}
    for L in sorted(set(sc.Q_CUTS) | set(sc.Q_TENS)):
        for pct in (0.5, 0.9):
            bal, low = sc.threshold_list(L, pct, False)
            tip, low_t = sc.threshold_list(L, pct, True)
            assert low_t == min(low + 1, L)
            if sc.pct_is_exact(pct, L):
                exact[pct] += 1
                assert low == pct * L                                   # a == pct * kn exactly: only the strict > keeps the walk going
            a, b = _q(ref, bal, pct, 100), _q(ref, tip, pct, 100)
            if L > 1:
                assert a != b, (L, pct, a, b)
                assert a > sc.bin_edge(60, 100) and b <= sc.bin_edge(11, 100), (L, pct, a, b)
            # a wrong loop bound: a low KeyLine at a stride boundary that is not counted below the gap leaves floor(pct L) there, which is
            # the balanced list's count (shown by moving it into the high group: kn stays L); one stale low KeyLine counted in addition
            # gives the balanced list the tipped list's count
            assert low <= pct * L < low + 1
            for i in sc.decisive_indices(L)[:low_t]:
                assert tip[i] < sc.bin_edge(11, 100)
                moved = tip.copy()
                moved[i] = sc.filler(100)
                assert L == 1 or _q(ref, moved, pct, 100) != b, (L, pct, i)
    for L in sc.Q_TENS:
        assert sc.pct_is_exact(0.9, L), L
    for L in sc.Q_CUTS:
        assert sc.pct_is_exact(0.5, L) == (L % 2 == 0)
    assert exact[0.5] >= 5 and exact[0.9] >= len(sc.Q_TENS)
    print("lengths with pct * L exact:", exact)
    assert _q(ref, np.full(300, sc.filler(100)), 0.9, 100) == 1e3
    assert _q(ref, np.full(300, sc.SMIN + 1e-3), 0.9, 100) == sc.bin_edge(1, 100)
    assert _q(ref, np.zeros(0), 0.9, 100) == 1e3


def test_quantile_restatement_port_and_defects(orcs):
    ref, port = orcs["ref"], orcs["port"]
    cases = sc.quantile_cases()
    caught = {d: [] for d in sc.QUANTILE_DEFECTS}
    n_eval = 0
    for name, s in cases:
        kl = sc.quantile_keylines(s)
        ref.set_keylines(0, kl)
        port.set_keylines(0, kl)
        for n in sc.Q_NBINS:
            bins = {d: sc.quantile_bins(s, sc.SMIN, sc.SMAX, n, d) for d in (None, "saturating", "clamp_before_convert", "clamp_order")}
            for pct in sc.Q_PCTS:
                want = ref.quantile(0, sc.SMIN, sc.SMAX, pct, n)
                assert sc.quantile_np(s, sc.SMIN, sc.SMAX, pct, n) == want, (name, n, pct)
                assert port.quantile(0, sc.SMIN, sc.SMAX, pct, n) == want, (name, n, pct)
                n_eval += 1
                for d in sc.QUANTILE_DEFECTS:
                    if d in bins and np.array_equal(bins[d], bins[None]):
                        continue                                       # the same histogram: the same answer
                    if sc.quantile_np(s, sc.SMIN, sc.SMAX, pct, n, d) != want:
                        caught[d].append((name, n, pct))
    print(f"{len(cases)} lists x {len(sc.Q_NBINS) * len(sc.Q_PCTS)} (nbins, pct) = {n_eval} evaluations; lists that catch each defect: "
          f"{ {d: len(set(c[0] for c in v)) for d, v in caught.items()} }")
    for d in sc.QUANTILE_DEFECTS:
        if d != "clamp_order":
            assert caught[d], f"no list catches the defect {d}"
    # clamp_order is no defect: for n >= 1 both orders give min(max(i, 0), n - 1) for every int, INT_MIN and INT_MAX included
    assert not caught["clamp_order"]
    i = np.array([sc.INT_MIN, -1, 0, 1, 254, 255, 256, 2 ** 31 - 1], np.int64)
    for n in range(1, 257):
        a = np.where(np.where(i > n - 1, n - 1, i) < 0, 0, np.where(i > n - 1, n - 1, i))
        b = np.where(np.where(i < 0, 0, i) > n - 1, n - 1, np.where(i < 0, 0, i))
        assert np.array_equal(a, b)
    lens = sorted({len(s) for _, s in cases})
    assert set(sc.Q_CUTS) <= set(lens) and 0 in lens
    order = [len(s) for _, s in cases]
    assert any(a > 4 * b for a, b in zip(order, order[1:]))             # a short list follows a long one


# ---------------------------------------------------------------------------------------------------------------------------------
# reEstimateThresh
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", sc.RT_NBINS)
def test_retune_walk(nbins):
    oracle = require_ref()
    frames = sc.retune_frames()
    histos, n_ms = [], []
    for s, pair in enumerate(frames):
        o = oracle.Oracle("ref", sc.retune_params(oracle, 12000, nbins), nslots=2)
        for k, f in enumerate(pair):
            o.stage_a(k, f, o.p.detector_thresh, 0)
            n_m = o.keylines(k)["n_m"]
            assert len(n_m) > 1000
            h, mx, mn = sc.modulus_histogram(n_m, nbins)
            assert sc.retune_np(n_m, 12000, nbins) == np.float32(o.retuned(k))        # the default TrackPoints: the walk runs out, i = n
            assert sc.retune_bins(h, 12000) == nbins
            if k == 1:
                histos.append(h)
                n_ms.append(n_m)
        o.close()
    values = sorted({v for h in histos for v in sc.retune_track_points(h)})
    print(f"nbins {nbins}: TrackPoints values", values, "bin 0 holds", [int(h[0]) for h in histos], "of", [int(h.sum()) for h in histos])
    assert all(h[0] > 0 for h in histos)                                 # so counting bin 0 changes every cumulative count
    # the walk ends where each value is meant to end, on the sequence it was derived from
    for h in histos:
        v0, v1, ci, ci1, tot, tot1 = sc.retune_track_points(h)
        c = np.cumsum(h[1:])
        i = sc.retune_bins(h, ci)
        assert c[i - 1] == ci and h[i] > 0                               # lands exactly on knum, on a bin that counts
        assert sc.retune_bins(h, ci1) > i                                # one more: a later bin
        assert sc.retune_bins(h, tot) == np.nonzero(h)[0].max() and h[nbins - 1] > 0   # the total without bin 0: reached on the last bin
        assert sc.retune_bins(h, tot1) == nbins                          # never reached -> nbins
        assert sc.retune_bins(h, 0) == 0 and sc.retune_bins(h, -5) == 0
        assert sc.retune_bins(h, 1) == np.nonzero(h[1:])[0].min() + 1
    caught = {d: 0 for d in sc.RETUNE_DEFECTS}
    for v in values:
        for kind in ("ref", "port"):
            for s, pair in enumerate(frames):
                a = oracle.Oracle(kind, sc.retune_params(oracle, v, nbins), nslots=2)
                b = oracle.Oracle(kind, sc.retune_params(oracle, v, nbins), nslots=8) if kind == "ref" else None      # (the port: stage_a alone)
                for k, f in enumerate(pair):
                    a.stage_a(k, f, a.p.detector_thresh, 0)
                    want = sc.retune_np(a.keylines(k)["n_m"], v, nbins)
                    assert np.float32(a.retuned(k)) == want, (kind, v, s, k)
                    if b is not None:
                        _, nav = b.process_frame(f, 0.05 * k)
                        assert np.float32(nav.retuned_thresh) == want, (kind, v, s, k)
                    if kind == "ref" and k == 1:
                        for d in sc.RETUNE_DEFECTS:
                            caught[d] += int(sc.retune_np(n_ms[s], v, nbins, defect=d) != want)
                a.close()
                if b is not None:
                    b.close()
    print("(value, sequence) pairs that catch each retune defect:", caught)
    assert all(caught.values())


# ---------------------------------------------------------------------------------------------------------------------------------
# ExtRotVel
# ---------------------------------------------------------------------------------------------------------------------------------
def _erv(orc, kl, vel):
    orc.set_keylines(0, kl)
    return orc.ext_rot_vel(0, vel, sc.LOC_UNC, sc.HUB)


def test_ext_rot_vel_lists(orcs):
    ref, port = orcs["ref"], orcs["port"]
    caught = {d: set() for d in sc.ERV_DEFECTS}
    conds, worst_bound, n_lists = {}, 0.0, 0
    met, pole_finite_rho, s_rho_inf_at_zero = {}, [], []
    for cut, names, vels in sc.erv_jobs():
        for name, vel in zip(names, vels):
            kl = sc.erv_list(name, cut, vel)
            L, n_rows = len(kl), int((kl["m_id"] >= 0).sum())
            r = _erv(ref, kl, vel)
            rp = _erv(port, kl, vel)
            n_lists += 1
            met.setdefault(name, set()).add(vel)
            assert sc.erv_agree(sc.ext_rot_vel_np(kl, vel), r, n_rows) == [], (name, cut, vel)
            assert sc.erv_agree(rp, r, n_rows) == [], (name, cut, vel)
            for d in sc.ERV_DEFECTS:
                if sc.erv_agree(sc.ext_rot_vel_np(kl, vel, defect=d), r, n_rows):
                    caught[d].add((name, cut))
            finite = np.isfinite(r["Wx"]).all()
            if name == "none":
                assert n_rows == 0 and r["ok"] and not r["Wx"].any() and not r["X"].any() and not r["Rx"].any()
            if name.startswith("few"):
                assert n_rows == min(int(name[3:]), L)
            if name == "pole":
                assert not r["ok"] and not finite and not np.isfinite(r["X"]).any() and not np.isfinite(r["Rx"]).any()
                with np.errstate(divide="ignore"):
                    assert 1 / kl["rho"][L // 2] + vel[2] == 0
                if vel[2] != 0:
                    assert np.isfinite(kl["rho"][L // 2]) and kl["rho"][L // 2] != 0
                    pole_finite_rho.append((cut, vel))
            if name == "s_rho_nan":
                assert not r["ok"] and not np.isfinite(r["Wx"]).any()
            if name == "rho_zero":
                assert r["ok"] and finite
            if name == "s_rho_inf":
                assert r["ok"] == finite == any(vel)                     # a zero velocity makes s_y = sqrt(inf * 0): NaN
                if not any(vel):
                    s_rho_inf_at_zero.append(cut)
            if not finite:
                continue
            cond, s = sc.kept_condition(r["Wx"])
            e = np.abs(np.linalg.eigvalsh(r["Wx"]))
            assert not np.any((e > e.max() / 1e10) & (e < e.max() / 1e8)), (name, cut, e)      # both sides keep / drop the same ones
            rank = int((s * 1e9 > s.max()).sum()) if s.max() > 0 else 0
            conds.setdefault(name, []).append(cond)
            if name in sc.ERV_FULL_RANK and L >= 255:
                assert rank == 6 and cond <= 1e6, (name, cut, rank, cond)
            if name == "parallel" and L >= 255:
                assert rank == 5
            if name.startswith("few"):
                assert rank == n_rows
            _, tol_x, tol_r, _ = sc.erv_bounds(r, n_rows)
            for q in (r, rp):                                            # the bound against the solution's size, on the reference and on the port
                if np.abs(q["X"]).max() > 0:
                    _, tx, tr, _ = sc.erv_bounds(q, n_rows)
                    worst_bound = max(worst_bound, tx / np.abs(q["X"]).max(), tr / np.abs(q["Rx"]).max())
            if name in sc.ERV_LONERS and L >= 255:
                # without the loner's row the rank drops and X moves by far more than the bound — on the reference and on the port
                i = sc.loner_index(name, L)
                assert np.count_nonzero(sc.erv_rows(kl, vel, sc.zfm())[0][:, 5]) == 1
                lost = kl.copy()
                lost["m_id"][i] = -1
                for orc in (ref, port):
                    q = _erv(orc, lost, vel)
                    assert q["Wx"][5, 5] == 0 and not q["Wx"][5].any()
                    assert np.abs(q["X"] - r["X"]).max() >= 100 * tol_x, (name, cut, np.abs(q["X"] - r["X"]).max(), tol_x)
    print(f"{n_lists} lists; cond of the kept singular values, (min, max) per variant:",
          {k: (f"{min(v):.1e}", f"{max(v):.1e}") for k, v in conds.items()})
    print(f"largest bound relative to its solution: {worst_bound:.1e}; lists that catch each defect:", {d: len(v) for d, v in caught.items()})
    assert worst_bound <= 1e-4
    assert all(met[n] == set(sc.E_VELS) for n in sc.ERV_VARIANTS), met      # every variant meets every velocity
    assert len(pole_finite_rho) >= 2 and s_rho_inf_at_zero, (pole_finite_rho, s_rho_inf_at_zero)
    print("pole with a finite rho at (cut, velocity):", pole_finite_rho, "; s_rho = inf at zero velocity at cuts", s_rho_inf_at_zero)
    for d in sc.ERV_DEFECTS:
        assert caught[d], f"no list catches the defect {d}"
    assert any(n == "loner_first" for n, _ in caught["m_id_gt0"]) and any(n == "loner_last" for n, _ in caught["skip_last"])
    assert any(n == "signs" for n, _ in caught["no_fabs"]) and any(n == "promote" for n, _ in caught["early_promote"])


def test_zz_time():
    print(f"tests/test_stats_crafted_cpu.py: {SPENT[0]:.1f} s")
