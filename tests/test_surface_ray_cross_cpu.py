"""CPU: the exhaustive cross-view ray check (SurfaceInt::checkDFRayCrossExaustive).  The numpy restatement
(tests/surface_ray_cross_port.py) against the reference's own flags (tests/golden/surface_ray_cross/*.npz,
tools/make_surface_ray_cross_golden.py), flag for flag; the branch populations of the fixtures; the IEEE branches on the crafted views;
and the new C ABI entry point in the built library."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import surface_ray_cross_port as port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "surface_ray_cross")
SRC = os.path.join(ROOT, "tests", "golden", "surface_integrate")
SCENES = {"376x240_b10": (0, 3), "376x240_b7": (0, 1), "752x480_b10": (0, 7)}   # the pair the issue's estimate put at 0.126, 0.644, 0.889
NAMES = list(SCENES) + ["crafted"]


def load(name):
    """-> dict(w, h, bw, bh, cam, views, steps [(start, absent, pairs or None)], ref [nsteps][nviews](gh, gw) bool, ocgrid, src).
    ocgrid: the flags of the OcGrid cut (cut 0 of the surface_integrate fixture) that a step with start == 2 falls from; src: that
    fixture (None for `crafted`, which holds its own views)."""
    f = np.load(os.path.join(GOLD, name + ".npz"))
    src = np.load(os.path.join(SRC, name + ".npz")) if name in SCENES else None
    g = f if src is None else src
    nv = len(g["K"])
    gh, gw = g["rho"].shape[1:]
    views = [port.view(g["rho"][k], g["s_rho"][k], g["Pose"][k], g["Pos"][k], g["K"][k]) for k in range(nv)]
    steps = [(int(s[0]), int(s[1]), None if s[2] < 0 else [(int(s[3 + 2 * j]), int(s[4 + 2 * j])) for j in range(s[2])]) for s in f["steps"]]
    ref = np.unpackbits(f["vis"])[:len(steps) * nv * gh * gw].reshape(len(steps), nv, gh, gw).astype(bool)
    oc = None if src is None else list(np.unpackbits(src["vis"])[:nv * gh * gw].reshape(nv, gh, gw).astype(bool))
    return dict(w=int(g["w"]), h=int(g["h"]), bw=int(g["bw"]), bh=int(g["bh"]), cam=port.camera(*g["cam"]), views=views, steps=steps,
                ref=ref, ocgrid=oc, src=src)


def step_views(fx, absent):
    return [None if k == absent else v for k, v in enumerate(fx["views"])]


_PORT = {}


def port_flags(name):
    """The port's flags after every step of a fixture, computed once -> ([nsteps][nviews], branch populations)."""
    if name not in _PORT:
        fx = load(name)
        out, prev, stats = [], None, {}
        for start, absent, pairs in fx["steps"]:
            base = {0: prev, 1: None, 2: fx["ocgrid"]}[start]
            prev = port.ray_cross(step_views(fx, absent), pairs, fx["bw"], fx["bh"], fx["cam"], base, stats)
            out.append(prev)
        _PORT[name] = (out, stats)
    return _PORT[name]


def test_fixtures_present():
    paths = sorted(glob.glob(os.path.join(GOLD, "*.npz")))
    assert sorted(os.path.basename(p)[:-4] for p in paths) == sorted(NAMES)
    limit = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "depth_surface", "*.npz")))
    assert all(os.path.getsize(p) <= limit for p in paths)
    for name, grid, nv in (("376x240_b10", (24, 37), 4), ("376x240_b7", (34, 53), 5), ("752x480_b10", (48, 75), 8), ("crafted", (24, 37), 3)):
        fx = load(name)
        assert fx["ref"].shape[1:] == (nv,) + grid
        assert set(np.load(os.path.join(GOLD, name + ".npz")).files) >= {"steps", "vis"}
    for name in SCENES:   # the scenes store no views of their own; their K shows the unscaled dist
        assert set(np.load(os.path.join(GOLD, name + ".npz")).files) == {"steps", "vis"}
        K = np.array([v["K"] for v in load(name)["views"]])
        assert np.abs(K - 1).max() > 0.1


def test_steps_cover_the_issue():
    """Every scene: all ordered pairs after a reset; one pair in each direction; an accumulating step on top of the first; a step on
    top of the OcGrid cut's flags; a list that names an empty slot."""
    for name, (a, b) in SCENES.items():
        steps, ref = load(name)["steps"], load(name)["ref"]
        assert steps[0] == (1, -1, None)
        assert steps[1] == (1, -1, [(a, b)]) and steps[3] == (1, -1, [(b, a)])
        assert steps[2][0] == 0 and (ref[2] <= ref[1]).all() and ref[2].sum() < ref[1].sum()
        assert steps[4][0] == 2 and steps[5][1] >= 0 and any(steps[5][1] in p for p in steps[5][2])
        oc = np.stack(load(name)["ocgrid"])
        assert (ref[4] <= oc).all() and ref[4].sum() < oc.sum() and not oc.all()
        assert ref[1, a].sum() < ref[1, a].size and ref[1, [k for k in range(ref.shape[1]) if k != a]].all()   # only the target changes


@pytest.mark.parametrize("name", NAMES)
def test_port_equals_reference(name):
    fx = load(name)
    got, stats = port_flags(name)
    print(name, "branch populations:", stats)
    for i, (_, absent, _) in enumerate(fx["steps"]):
        for k in range(len(fx["views"])):
            if k == absent:
                assert got[i][k] is None
            else:
                assert np.array_equal(got[i][k], fx["ref"][i, k]), (i, k, int((got[i][k] != fx["ref"][i, k]).sum()))
    # the branches of :100-104: outside and inside the bubble, past the hidder's surface, crossed
    assert stats["tests"] > stats["near"] > stats["hits"] > 0 and stats["past_surface"] > 0


def test_behind_the_centre_is_populated():
    """The `0 <` gate decides cells in the fixtures: cells inside a ray's bubble but behind the hidder's centre."""
    behind = {name: port_flags(name)[1]["behind_origin"] for name in NAMES}
    print("inside the bubble and behind the hidder's centre:", behind)
    assert sum(v > 0 for v in behind.values()) >= 2


@pytest.mark.parametrize("name", list(SCENES))
def test_branch_populations(name):
    """The reference's flags: the pair (a, b) hides a share of a's cells inside [0.05, 0.95]; the reverse direction is printed beside
    it; both outcomes are populated in both."""
    fx = load(name)
    a, b = SCENES[name]
    fwd, rev = 1 - fx["ref"][1, a].mean(), 1 - fx["ref"][3, b].mean()
    every = 1 - fx["ref"][0].mean()
    print(f"{name}: hidden share of ({a}, {b}) {fwd:.3f}, of ({b}, {a}) {rev:.3f}, after every ordered pair {every:.3f}")
    assert 0.05 <= fwd <= 0.95
    assert 0 < rev < 1 and 0.05 <= every <= 0.95


def test_unscaled_dist_quirk_shows():
    """`dist` multiplied by the hidder's K, or the `0 <` gate dropped, would change flags of every scene: the fixtures can tell."""
    for name, (a, b) in SCENES.items():
        fx = load(name)
        t, h = fx["views"][a], fx["views"][b]
        scaled = dict(h, rho=h["rho"] / h["K"], K=port.F64(1.0))   # the same surface with K folded into the grid: dist comes out scaled
        assert abs(h["K"] - 1) > 0.05
        plain = port.crossed(t, h, fx["bw"], fx["bh"], fx["cam"])
        assert np.array_equal(~plain.reshape(fx["ref"].shape[2:]), fx["ref"][1, a])
        assert (plain != port.crossed(t, scaled, fx["bw"], fx["bh"], fx["cam"])).sum() > 0, name


def test_crafted_ieee_branches():
    """The crafted views: rho zero, negative, NaN and infinite in a target and in a hidder; a hidder in the target's centre (ray_orig is
    exactly zero, the ray vectors are not); a view with K = 1.  The expected flags are the reference's."""
    fx = load("crafted")
    v0, v1, v2 = fx["views"]
    r = v0["rho"]
    assert r[5, 7] == 0 and r[5, 8] < 0 and np.isnan(r[6, 7]) and np.isposinf(r[6, 8]) and np.isneginf(r[15, 20])
    assert r[16, 30] == 0 and np.signbit(r[16, 30])
    assert np.isnan(v1["rho"][10, 12]) and v1["rho"][11, 12] == 0
    assert v0["K"] == 1.0 and v1["K"] != 1.0 and v2["K"] != 1.0
    assert np.array_equal(v0["Pos"], v1["Pos"]) and not np.array_equal(v0["Pose"], v1["Pose"])
    ro, v, dist = port.rays(v0, v1, fx["bw"], fx["bh"], fx["cam"])
    assert (ro == 0).all()
    ok = np.isfinite(v1["rho"].reshape(-1)) & (v1["rho"].reshape(-1) != 0)
    assert np.isfinite(v[ok]).all() and (np.abs(v[ok]).max(-1) > 0.5).all()
    assert np.isnan(v[~ok]).all()                     # a ray through a point at infinity, or at no number, has no direction
    ref = fx["ref"]
    # a NaN bubble or a NaN point compares false everywhere: never hidden; a negative bubble is below every distance: never hidden
    for y, x in ((6, 7), (5, 8), (15, 20)):
        assert ref[:, 0, y, x].all(), (y, x)
    # rho = +inf: the point is the centre itself and the bubble is zero: never inside
    assert ref[:, 0, 6, 8].all()
    # both outcomes among the ordinary cells of every pair of the list
    assert 0.05 < 1 - ref[1, 0].mean() < 0.95           # (0, 1): the hidder stands in the target's centre
    assert ref[2, 1].sum() < ref[1, 1].sum() and 0.05 < 1 - ref[2, 1].mean() < 0.95   # (1, 0) on top
    assert 0.05 < 1 - ref[3, 0].mean() < 0.95 and 0.05 < 1 - ref[3, 2].mean() < 0.95
    got, _ = port_flags("crafted")
    print("crafted: hidden per step", [round(1 - float(ref[i].mean()), 3) for i in range(len(ref))],
          "flags of rho = 0 cells", ref[:, 0, 5, 7].astype(int), ref[:, 0, 16, 30].astype(int))
    for i in range(len(ref)):
        for k in range(3):
            if got[i][k] is not None:
                assert np.array_equal(got[i][k], ref[i, k]), (i, k)


def test_order_free_and_skips():
    """Visibility only falls: the pairs of a step in any order, or one at a time accumulating, give the same flags; a pair that names
    an empty slot changes nothing."""
    fx = load("376x240_b10")
    args = (fx["bw"], fx["bh"], fx["cam"])
    pairs = port.all_pairs(fx["views"])
    a = port.ray_cross(fx["views"], pairs[::-1], *args)
    b = None
    for p in pairs:
        b = port.ray_cross(fx["views"], [p], *args, b)
    for k in range(len(fx["views"])):
        assert np.array_equal(a[k], fx["ref"][0, k]) and np.array_equal(b[k], fx["ref"][0, k])
    vv = step_views(fx, 1)
    c = port.ray_cross(vv, [(0, 1), (1, 0), (2, 1)], *args)
    assert c[1] is None and all(c[k].all() for k in (0, 2, 3))


@pytest.mark.parametrize("name", NAMES)
def test_culled_port_decides_the_same(name):
    """crossed_culled, which the GPU test of 64 views uses on its 504 pairs, gives the reference's flags too, on every step."""
    fx = load(name)
    prev = None
    for i, (start, absent, pairs) in enumerate(fx["steps"]):
        base = {0: prev, 1: None, 2: fx["ocgrid"]}[start]
        prev = port.ray_cross(step_views(fx, absent), pairs, fx["bw"], fx["bh"], fx["cam"], base, cull=True)
        for k in range(len(fx["views"])):
            if k != absent:
                assert np.array_equal(prev[k], fx["ref"][i, k]), (i, k)


def test_abi_symbol_and_null_context():
    """The entry point exists; a NULL context is EDGEHIP_ERR_ARG before anything touches a device."""
    lib = edgehip.load_library()
    assert hasattr(lib, "edgehip_surface_ray_cross")
    assert "edgehip_surface_ray_cross" in edgehip.EXPORTS
    assert lib.edgehip_surface_ray_cross(None, -1, None, None, 0) == -1
    one = (C.c_int32 * 1)(0)
    assert lib.edgehip_surface_ray_cross(None, 1, one, one, 1) == -1
    assert hasattr(edgehip.EdgeHip, "surface_ray_cross")
