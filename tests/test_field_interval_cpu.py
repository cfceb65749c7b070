"""build_field's rasteriser tests a KeyLine's samples against its tile only at the two ends of the t-range (k_field_raster,
rebvo_amd/csrc/stage_b.hip).  That rests on two facts, checked here in numpy float32 on the restated arithmetic, no GPU:

  (1) for one KeyLine and one tile, the t in [-r, r - 1] whose sample rounds into the tile (clipped to the image) form ONE contiguous
      run — fl(u t), fl(. + c) and the rounding to a pixel are each monotone in t;
  (2) tile_trange's conservative range never drops such a t, so walking inwards from its two ends to the first sample that passes
      the exact test yields exactly that run.

The sample expression (global_tracker.cpp:78: float u * (float)t + c, no contraction), both roundings (round() as Image::GetIndexRC
uses it, and the hardware's ties-towards-plus-infinity conversion that the tiles away from column / row 0 use) and tile_trange are
restated below; the reciprocal is the correctly rounded one (the device's v_rcp_f32 is within 1 ulp of it, which the range's own
slack of 1e-4 |1/u| samples covers many times over)."""
import numpy as np
import pytest

FT = 64
W, H = 96, 80                       # 2 x 2 tiles, the right and the bottom ones clipped by the image
TILES = [(0, 0), (64, 0), (0, 64), (64, 64)]
RADII = (4, 40, 127, 128)
F = np.float32


def sample_pos(u, c, t):
    """fl(fl(u * t) + c) for u, c [N] and t [T] -> [N, T]; numpy rounds every float32 operation once and never fuses."""
    return (u[:, None] * t[None, :].astype(F)).astype(F) + c[:, None]


def round_half_away(v):
    """round(): halves away from zero (exact: |v| < 2^23 in float64)."""
    v = v.astype(np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def round_ties_up(v):
    """v_cvt_rpi_i32_f32: to nearest, ties towards +infinity, evaluated exactly."""
    return np.floor(v.astype(np.float64) + 0.5).astype(np.int64)


def in_tile(ux, uy, cx, cy, t, tx0, ty0, rnd_x, rnd_y):
    ex, ey = min(FT, W - tx0), min(FT, H - ty0)
    lx = rnd_x(sample_pos(ux, cx, t)) - tx0
    ly = rnd_y(sample_pos(uy, cy, t)) - ty0
    return (lx >= 0) & (lx < ex) & (ly >= 0) & (ly < ey)


def tile_trange(ux, uy, cx, cy, tx0, ty0, r):
    """tile_trange of stage_b.hip, operation by operation in float32.  Returns (ok, t0, t1)."""
    n = len(ux)
    tlo, thi = np.full(n, -r, F), np.full(n, r - 1, F)
    ok = np.ones(n, bool)
    for u, c, o in ((ux, cx, tx0), (uy, cy, ty0)):
        b0 = (F(o) - F(0.51)) - c
        b1 = (F(o + FT) - F(0.49)) - c
        moving = np.abs(u) > F(1e-6)
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            iu = F(1) / u
            a, b = b0 * iu, b1 * iu
            sl = F(0.25) + F(1e-4) * np.abs(iu)
            lo, hi = np.minimum(a, b) - sl, np.maximum(a, b) + sl
        tlo = np.where(moving, np.maximum(tlo, lo), tlo).astype(F)
        thi = np.where(moving, np.minimum(thi, hi), thi).astype(F)
        ok &= moving | ~((b0 > 0) | (b1 < 0))
    t0 = np.maximum(np.ceil(tlo.astype(np.float64)), -r).astype(np.int64)
    t1 = np.minimum(np.floor(thi.astype(np.float64)), r - 1).astype(np.int64)
    return ok & (t0 <= t1), t0, t1


def crafted_records(r, seed):
    """(ux, uy, cx, cy) float32: unit directions, short ones, components near 1e-6 and 1e-3 and exactly 0; centres spread over the
    image and beyond its border, and centres that put a sample exactly on k + 0.5 (a tie of the rounding) or on -0.5."""
    rs = np.random.RandomState(seed)
    n = 600
    ang = rs.uniform(0, 2 * np.pi, n)
    sets = [np.stack([np.cos(ang), np.sin(ang)], 1),                                   # unit length
            rs.uniform(-1, 1, (n, 2)),                                                 # |u| <= 1, any length
            np.stack([rs.uniform(0.5e-6, 2e-6, n) * rs.choice([-1, 1], n), rs.choice([-1.0, 1.0], n)], 1),   # across the 1e-6 gate
            np.stack([rs.choice([-1.0, 1.0], n), rs.uniform(0.5e-6, 2e-6, n) * rs.choice([-1, 1], n)], 1),
            np.stack([rs.uniform(0.5e-3, 2e-3, n) * rs.choice([-1, 1], n), rs.choice([-1.0, 1.0], n)], 1),   # near 1e-3
            np.stack([rs.choice([-1.0, 1.0], n), rs.uniform(0.5e-3, 2e-3, n) * rs.choice([-1, 1], n)], 1),
            np.stack([np.zeros(n), rs.choice([-1.0, 1.0], n)], 1),                     # exactly axis-parallel
            np.stack([rs.choice([-1.0, 1.0], n), np.zeros(n)], 1),
            np.zeros((n // 4, 2))]                                                     # a point
    gate = F(1e-6)
    edge = np.array([[gate, 1], [np.nextafter(gate, F(1)), 1], [np.nextafter(gate, F(0)), 1], [-gate, -1],
                     [1, gate], [1, np.nextafter(gate, F(1))], [1, np.nextafter(gate, F(0))], [-1, -gate]], np.float64)
    sets.append(np.repeat(edge, n // 8, 0))
    u = np.concatenate(sets).astype(F)
    m = len(u)
    c = np.stack([rs.uniform(-3, W + 3, m), rs.uniform(-3, H + 3, m)], 1).astype(F)
    # a third: the sample at a random t* lands on a tie k + 0.5 — k around the tile and image borders, and k = -1 (-0.5)
    ks_x = np.array([-1, 0, 62, 63, 64, 94, 95, 96])
    ks_y = np.array([-1, 0, 62, 63, 64, 78, 79, 80])
    tie = rs.rand(m) < 1 / 3
    tstar = rs.randint(-r, r, m).astype(F)
    for j, ks in ((0, ks_x), (1, ks_y)):
        k = ks[rs.randint(0, len(ks), m)].astype(F) + F(0.5)
        cj = k - (u[:, j] * tstar).astype(F)                       # fl(u t*) + c is then k + 0.5 exactly, or one rounding off it
        sel = tie & (rs.rand(m) < 0.7)
        c[sel, j] = cj[sel]
    # another sixth: the centre itself on a tie (t = 0), -0.5 included
    own = ~tie & (rs.rand(m) < 0.25)
    c[own, 0] = ks_x[rs.randint(0, len(ks_x), own.sum())] + 0.5
    own2 = ~tie & (rs.rand(m) < 0.25)
    c[own2, 1] = ks_y[rs.randint(0, len(ks_y), own2.sum())] + 0.5
    return u[:, 0].copy(), u[:, 1].copy(), c[:, 0].copy(), c[:, 1].copy()


@pytest.fixture(scope="module", params=RADII)
def case(request):
    r = request.param
    return (r,) + crafted_records(r, 100 + r)


def _runs(inside):
    """first, last index of True per row and the count; (-1, -1, 0) for an empty row."""
    cnt = inside.sum(1)
    first = np.where(cnt > 0, inside.argmax(1), -1)
    last = np.where(cnt > 0, inside.shape[1] - 1 - inside[:, ::-1].argmax(1), -1)
    return first, last, cnt


def test_the_crafted_records_hold_the_cases(case):
    r, ux, uy, cx, cy = case
    t = np.arange(-r, r)
    fx, fy = sample_pos(ux, cx, t), sample_pos(uy, cy, t)
    assert (fx == F(-0.5)).any() and (fy == F(-0.5)).any()
    for k in (63.5, 95.5):
        assert (fx == F(k)).any()
    for k in (63.5, 79.5):
        assert (fy == F(k)).any()
    assert (ux == 0).any() and (np.abs(ux) == F(1e-6)).any() and ((np.abs(ux) > F(1e-6)) & (np.abs(ux) < F(2e-6))).any()
    assert (np.abs(np.hypot(ux.astype(np.float64), uy.astype(np.float64)) - 1) < 1e-6).sum() >= 600


@pytest.mark.parametrize("tile", TILES)
def test_in_tile_samples_form_one_run(case, tile):
    r, ux, uy, cx, cy = case
    tx0, ty0 = tile
    t = np.arange(-r, r)
    exact = in_tile(ux, uy, cx, cy, t, tx0, ty0, round_half_away, round_half_away)
    first, last, cnt = _runs(exact)
    assert cnt.max() > 0 and (cnt == 0).any()
    assert np.array_equal(last - first + 1, np.where(cnt > 0, cnt, 1)), "the in-tile t are not one contiguous run"
    # the rounding each tile's loop uses: the bare conversion away from column / row 0 selects the same samples
    used = in_tile(ux, uy, cx, cy, t, tx0, ty0, round_half_away if tx0 == 0 else round_ties_up,
                   round_half_away if ty0 == 0 else round_ties_up)
    assert np.array_equal(used, exact)
    # and inside the run the bare conversion names the same pixel in EVERY tile (the test-free loop uses nothing else)
    px_a, px_b = round_half_away(sample_pos(ux, cx, t)), round_ties_up(sample_pos(ux, cx, t))
    py_a, py_b = round_half_away(sample_pos(uy, cy, t)), round_ties_up(sample_pos(uy, cy, t))
    assert np.array_equal(px_a[exact], px_b[exact]) and np.array_equal(py_a[exact], py_b[exact])


@pytest.mark.parametrize("tile", TILES)
def test_trimming_the_conservative_range_yields_exactly_the_run(case, tile):
    r, ux, uy, cx, cy = case
    tx0, ty0 = tile
    t = np.arange(-r, r)
    exact = in_tile(ux, uy, cx, cy, t, tx0, ty0, round_half_away, round_half_away)
    first, last, cnt = _runs(exact)
    ok, t0, t1 = tile_trange(ux, uy, cx, cy, tx0, ty0, r)
    assert not (cnt[~ok] > 0).any(), "tile_trange refused a KeyLine that has a sample in the tile"
    assert ok.any() and (t0[ok] >= -r).all() and (t1[ok] <= r - 1).all()
    # the walk from both ends, as the kernel does it: up from t0 to the first inside sample, down from t1 to the last
    window = (t[None, :] >= t0[:, None]) & (t[None, :] <= t1[:, None]) & ok[:, None]
    wfirst, wlast, wcnt = _runs(exact & window)
    assert np.array_equal(wcnt, cnt), "the conservative range dropped an inside sample"
    assert np.array_equal(wfirst, first) and np.array_equal(wlast, last)
    # nothing left <=> nothing inside: such an item is skipped
    assert np.array_equal(wcnt == 0, cnt == 0)
    # the bin entry's bytes: both ends biased by the radius fit a byte up to r = 127 (2 r - 1 <= 253 < the 0xFFFF "no hit" mark's 255)
    if r <= 127:
        assert (t0[ok] + r).min() >= 0 and (t1[ok] + r).max() <= 253
