"""CPU: the cross-view surface integration (analizeSpaceSize, OcGrid::fillKFList / rayCutSurface).  The numpy restatement
(tests/surface_integrate_port.py) against the reference's own results (tests/golden/surface_integrate/*.npz,
tools/make_surface_integrate_golden.py), flag for flag; the fixture conditions re-asserted from the stored data; the documented
departures on hand-made cases; and the new C ABI entry points in the built library."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import surface_integrate_port as port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "surface_integrate")
NAMES = ["376x240_b10", "376x240_b7", "752x480_b10"]


def load(name):
    """-> (fixture, views, cuts [(reset, cast or None)], reference visibility [ncuts][nviews](gh, gw) bool, camera)."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    nv = len(g["K"])
    views = [port.view(g["rho"][k], g["s_rho"][k], g["Pose"][k], g["Pos"][k], g["K"][k]) for k in range(nv)]
    cuts = [(int(c[0]), None if c[1] < 0 else [int(v) for v in c[2:2 + c[1]]]) for c in g["cuts"]]
    gh, gw = g["rho"].shape[1:]
    vis = np.unpackbits(g["vis"])[:len(cuts) * nv * gh * gw].reshape(len(cuts), nv, gh, gw).astype(bool)
    return g, views, cuts, vis, port.camera(*g["cam"])


def test_fixtures_present():
    paths = sorted(glob.glob(os.path.join(GOLD, "*.npz")))
    assert [os.path.basename(p)[:-4] for p in paths] == NAMES
    limit = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "depth_surface", "*.npz")))
    assert all(os.path.getsize(p) <= limit for p in paths)
    for name, res, blk, nv, nvox in (("376x240_b10", (376, 240), 10, 3, 0), ("376x240_b7", (376, 240), 7, 3, 0),
                                     ("752x480_b10", (752, 480), 10, 8, 128 ** 3)):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        assert (int(g["w"]), int(g["h"])) == res and int(g["bw"]) == int(g["bh"]) == blk
        assert len(g["K"]) >= nv and int(np.prod(g["n"].astype(np.int64))) >= nvox
        p = edgehip.euroc_params(*res)
        assert np.array_equal(g["cam"], np.array([p.ppx, p.ppy, p.zfx, p.zfy], np.float32))
    g = np.load(os.path.join(GOLD, "376x240_b7.npz"))
    assert 376 % 7 and 240 % 7 and g["rho"].shape[1:] == (34, 53)   # the partial row and column


@pytest.mark.parametrize("name", NAMES)
def test_port_equals_reference(name):
    g, views, cuts, ref, cam = load(name)
    bw, bh = int(g["bw"]), int(g["bh"])
    o, s = port.space(views, bw, bh, cam)
    assert o.tobytes() == g["space_origin"].tobytes() and s.tobytes() == g["space_size"].tobytes()
    # the fixture's conditions, from the stored data
    for v in views:
        q = v["rho"] / v["K"]
        assert np.isfinite(q).all() and (q > 0).all()
        assert ((v["Pos"] > g["origin"]) & (v["Pos"] < g["origin"] + g["size"])).all()   # the camera centre lies inside the box
    hid = 1.0 - ref[0].mean()
    assert 0.05 <= hid <= 0.95, hid
    assert any(0 < ref[0, k].sum() < ref[0, k].size for k in range(len(views)))
    vis = None
    for c, (reset, cast) in enumerate(cuts):
        vis, stats = port.integrate(views, g["origin"], g["size"], g["n"], bw, bh, cam, cast, None if reset else vis)
        assert stats["ray_steps_outside"] == 0 and stats["samples_outside"] == 0, (c, stats)
        for k in range(len(views)):
            assert np.array_equal(vis[k], ref[c, k]), (c, k, int((vis[k] != ref[c, k]).sum()))


def test_cuts_cover_the_viewer_sequence():
    """Every fixture holds main.cpp's sequence (all key frames, then one on top: nothing new), an accumulation that adds hides, and
    a subset."""
    for name in NAMES:
        _, views, cuts, ref, _ = load(name)
        assert cuts[0] == (1, None) and cuts[1][0] == 0 and len(cuts[1][1]) == 1
        assert np.array_equal(ref[0], ref[1])
        assert cuts[2][0] == 1 and cuts[3][0] == 0 and (ref[3] <= ref[2]).all() and ref[3].sum() < ref[2].sum()
        assert any(r and cast is not None and len(cast) > 1 for r, cast in cuts)
        for c, (_, cast) in enumerate(cuts):   # a view's own rays never hide it
            if cast is not None and len(cast) == 1 and cuts[c][0]:
                assert ref[c, cast[0]].all()


def small_scene():
    cam = port.camera(40.0, 30.0, 100.0, 100.0)
    w, h, b = 80, 60, 10
    rho = np.full((6, 8), 0.5)
    s = np.full((6, 8), 0.02)
    # two cameras 2 units in front of the origin on either side, facing each other: each one's rays pass through the other's wall
    turn = np.diag([-1.0, 1.0, -1.0])
    views = [port.view(rho, s, np.eye(3), (0, 0, -1.5), 1.0), port.view(rho, s, turn, (0, 0, 1.5), 1.0)]
    return views, w, h, b, cam


def test_small_scene_hides_and_own_rays_do_not():
    views, w, h, b, cam = small_scene()
    o, s = np.array([-4.0, -4.0, -4.0]), np.array([8.0, 8.0, 8.0])
    vis, st = port.integrate(views, o, s, (40, 40, 40), b, b, cam)
    assert st["ray_steps_outside"] == 0 and st["samples_outside"] == 0
    assert not vis[0].all() and not vis[1].all()
    vis0, _ = port.integrate(views, o, s, (40, 40, 40), b, b, cam, cast=[0])
    assert vis0[0].all() and not vis0[1].all()
    # accumulate: falling from an earlier result only removes flags
    acc, _ = port.integrate(views, o, s, (40, 40, 40), b, b, cam, cast=[1], vis=vis0)
    assert np.array_equal(acc[0], vis[0]) and np.array_equal(acc[1], vis[1])
    # an empty slot neither casts nor is tested
    e, _ = port.integrate([views[0], None, views[1]], o, s, (40, 40, 40), b, b, cam)
    assert e[1] is None and np.array_equal(e[0], vis[0]) and np.array_equal(e[2], vis[1])


def test_departure_view_outside_the_box():
    """A box that holds neither camera nor surface: every sample and step is dropped, nothing hides; a box that holds half the scene
    drops the rest and keeps its flags."""
    views, w, h, b, cam = small_scene()
    vis, st = port.integrate(views, (10.0, 10.0, 10.0), (2.0, 2.0, 2.0), (16, 16, 16), b, b, cam)
    assert vis[0].all() and vis[1].all()
    assert st["samples_outside"] == st["samples"] > 0 and st["ray_steps_outside"] > 0 and st["voxels_marked"] == 0
    # camera 1 (z = +1.5) and its wall's far side are outside: z in [-4, 1)
    vis, st = port.integrate(views, (-4.0, -4.0, -4.0), (8.0, 8.0, 5.0), (40, 40, 25), b, b, cam)
    assert st["ray_steps_outside"] > 0 and st["voxels_marked"] > 0
    # negative quotients are outside too, also those in (-1, 0) that a truncating conversion would put in voxel 0
    inside, _, q = port.voxel(np.array([[-0.05, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 1.0, 0.5], [np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5]]),
                              port.box((0, 0, 0), (1, 1, 1), (10, 10, 10)))
    assert list(inside) == [False, True, False, False, False]   # p - origin == size is outside


@pytest.mark.parametrize("bad", [0.0, np.nan, -0.5, np.inf])
def test_departure_cell_without_samples(bad):
    """rho = 0, NaN, negative (or infinite): the cell contributes no samples and stays visible; the others are as before."""
    views, w, h, b, cam = small_scene()
    o, s, n = np.array([-4.0, -4.0, -4.0]), np.array([8.0, 8.0, 8.0]), (40, 40, 40)
    base, st0 = port.integrate(views, o, s, n, b, b, cam, cast=[0])
    assert not base[1][2, 3]
    rho = views[1]["rho"].copy()
    rho[2, 3] = bad
    views[1] = port.view(rho, views[1]["s_rho"], views[1]["Pose"], views[1]["Pos"], 1.0)
    vis, st = port.integrate(views, o, s, n, b, b, cam, cast=[0])
    assert vis[1][2, 3]
    assert st["samples"] < st0["samples"]
    far = np.ones((6, 8), bool)
    far[1:5, 2:6] = False          # the neighbours interpolate with the bad cell: compare away from it
    assert np.array_equal(vis[1][far], base[1][far])


def test_departure_ray_without_length():
    """rho + s_rho = 0: the ray's end is at infinity, its step count is no int: no steps.  With every ray of the only casting view so,
    nothing is marked."""
    views, w, h, b, cam = small_scene()
    o, s, n = np.array([-4.0, -4.0, -4.0]), np.array([8.0, 8.0, 8.0]), (40, 40, 40)
    views[0] = port.view(views[0]["rho"], -views[0]["rho"], views[0]["Pose"], views[0]["Pos"], 1.0)
    vis, st = port.integrate(views, o, s, n, b, b, cam, cast=[0])
    assert st["voxels_marked"] == 0 and st["ray_steps_outside"] == 0 and vis[1].all()
    one = views[0]["s_rho"].copy()
    one[:] = 0.02
    one[3, 4] = -views[0]["rho"][3, 4]
    views[0] = port.view(views[0]["rho"], one, views[0]["Pose"], views[0]["Pos"], 1.0)
    vis, st = port.integrate(views, o, s, n, b, b, cam, cast=[0])
    assert st["voxels_marked"] > 0 and not vis[1].all()


def test_space_starts_its_maxima_at_1e_minus_20():
    """A scene entirely at negative world coordinates keeps max = 1e-20 (surface_integrator.cpp:36-38)."""
    cam = port.camera(40.0, 30.0, 100.0, 100.0)
    v = port.view(np.full((6, 8), 0.5), np.full((6, 8), 0.1), np.eye(3), (-10.0, -10.0, -10.0), 1.0)
    o, s = port.space([v], 10, 10, cam)
    assert (o < -7).all()
    assert np.array_equal(s, np.full(3, 1e-20) - o)


def test_abi_symbols_and_errors_without_gpu_state():
    """The entry points exist; a NULL context is EDGEHIP_ERR_ARG before anything touches a device."""
    lib = edgehip.load_library()
    for s in ("edgehip_surface_views_enable", "edgehip_surface_view_capture", "edgehip_surface_view_upload", "edgehip_surface_view_clear",
              "edgehip_surface_space", "edgehip_surface_integrate", "edgehip_download_surface_visibility",
              "edgehip_download_surface_visibilities_batch"):
        assert hasattr(lib, s), s
    p = edgehip.SurfaceViewsParams(64, 500, 500, 500)
    assert C.sizeof(p) == 16
    assert lib.edgehip_surface_views_enable(None, C.byref(p)) == -1
    assert lib.edgehip_surface_integrate(None, None, None, 0, None, 0) == -1
    assert lib.edgehip_surface_space(None, None, None) == -1
