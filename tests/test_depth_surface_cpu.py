"""CPU: the depth surface (computeDistance / get3DPos / calcSurfNormals / calcSurfArea / getImgRho / getImgRhoTriInterp).  The numpy
restatement (tests/depth_surface_port.py) on the grids of tests/depth_fill_port.py against the reference's own results
(tests/golden/depth_surface/*.npz, tools/make_depth_surface_golden.py), bit for bit; the vectorised normal owner rule against the
raster loop; the border terms of the interpolation; and the new C ABI entry points in the built library."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import depth_fill_port as fport
from tests import depth_surface_port as port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "depth_surface")
CASES = sorted(p for p in glob.glob(os.path.join(GOLD, "*_case*.npz")) if "_image" not in p)
SENTINEL64 = 0x7FF4DEADBEEF0001   # tools/depth_surface_ref_driver.cpp
SENTINEL32 = 0x7FA0DEAD


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    """Bit for bit, except that a NaN the arithmetic creates equals any NaN."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def fill_case(path):
    """-> (fixture, fill grids (rho, s_rho), bw, bh, camera) of a depth_surface fixture, the grids from the depth_fill port."""
    g = np.load(path)
    w, h, i = int(g["w"]), int(g["h"]), int(g["case"])
    z = np.load(os.path.join(ROOT, "tests", "golden", "depth_fill", f"{w}x{h}.npz"))
    lst, bw, bh, it, mode, disc, m = (int(v) for v in z["cases"][i])
    kl = {f: z[f"kl{chr(lst)}_{f}"] for f in fport.FIELDS}
    rho, s_rho, _ = fport.depth_fill(kl, w, h, bw, bh, it, float(z[f"case{i}_thresh_rel_rho"]), m, mode, disc)
    cam = port.camera(*g["cam"])
    return g, (rho, s_rho), bw, bh, cam


def test_fixtures_present():
    assert len(CASES) == 16
    images = glob.glob(os.path.join(GOLD, "*_image*.npz"))
    assert len(images) == 4
    assert all(os.path.getsize(p) < 1 << 20 for p in CASES + images)


def test_camera_matches_context():
    """The fixtures' camera is edgehip.euroc_params', as the library keeps it (float pp and focal lengths)."""
    for w, h in ((376, 240), (752, 480)):
        p = edgehip.euroc_params(w, h)
        g = np.load(os.path.join(GOLD, f"{w}x{h}_case0.npz"))
        assert np.array_equal(g["cam"], np.array([p.ppx, p.ppy, p.zfx, p.zfy], np.float32))


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-4] for p in CASES])
def test_port_equals_reference(path):
    g, (rho, s_rho), bw, bh, cam = fill_case(path)
    s = port.surface(rho, bw, bh, cam)
    assert same_bits(s["point"], g["point"]).all()
    assert same_bits(s["dist"], g["dist"]).all()
    assert bits(np.float64(s["min_dist"])) == bits(np.float64(g["min_dist"]))
    # the cells the reference never writes hold its sentinel; the port writes NaN there
    ns = bits(g["normal"]) == SENTINEL64
    asn = bits(g["area"]) == SENTINEL32
    assert (ns.all(-1) == ns.any(-1)).all()
    assert np.array_equal(ns.any(-1), np.isnan(s["normal"]).all(-1) & ~np.isnan(g["normal"]).all(-1) | ns.any(-1))
    assert np.isnan(s["normal"][ns]).all() and np.isnan(s["area"][asn]).all()
    assert same_bits(s["normal"][~ns], g["normal"][~ns]).all()
    assert same_bits(s["area"][~asn], g["area"][~asn]).all()
    if "image" in g.files:   # 752x480: a seeded pixel sample plus the four border rows and columns
        px, py = g["sample"][:, 0], g["sample"][:, 1]
        for mode in (1, 2):
            r, sr = port.image_at(rho, s_rho, bw, bh, px, py, mode)
            assert same_bits(r, g["image"][2 * mode - 2]).all(), mode
            assert same_bits(sr, g["image"][2 * mode - 1]).all(), mode


def test_unwritten_cells_are_the_sentinel_cells():
    """Exactly (gw-1, 0) and (0, gh-1) lack a normal and exactly the last row and column lack an area: in every fixture."""
    for path in CASES:
        g = np.load(path)
        gh, gw = g["area"].shape
        want_n = np.zeros((gh, gw), bool)
        want_n[0, gw - 1] = want_n[gh - 1, 0] = True
        want_a = np.zeros((gh, gw), bool)
        want_a[gh - 1, :] = want_a[:, gw - 1] = True
        assert np.array_equal((bits(g["normal"]) == SENTINEL64).all(-1), want_n), path
        assert np.array_equal(bits(g["area"]) == SENTINEL32, want_a), path
        assert np.array_equal(np.isnan(port.normals(g["point"])).all(-1), want_n | np.isnan(g["normal"]).all(-1) & ~want_n)


@pytest.mark.parametrize("name", sorted({os.path.basename(p).rsplit("_image", 1)[0] for p in glob.glob(os.path.join(GOLD, "*_image*.npz"))}))
def test_whole_image_equals_reference(name):
    g, (rho, s_rho), bw, bh, cam = fill_case(os.path.join(GOLD, name + ".npz"))
    w, h = int(g["w"]), int(g["h"])
    for mode in (1, 2):
        ref = np.load(os.path.join(GOLD, f"{name}_image{mode}.npz"))
        r, sr = port.image(rho, s_rho, w, h, bw, bh, mode)
        assert same_bits(r, ref["rho"]).all(), (name, mode, int((~same_bits(r, ref["rho"])).sum()))
        assert same_bits(sr, ref["s_rho"]).all(), (name, mode)


@pytest.mark.parametrize("gw,gh", [(1, 1), (1, 5), (5, 1), (2, 2), (7, 4), (37, 24)])
def test_normal_owner_rule_equals_raster_loop(gw, gh):
    rng = np.random.default_rng(gw * 100 + gh)
    rho = rng.uniform(0.05, 3.0, (gh, gw))
    rho[rng.random((gh, gw)) < 0.05] = -rng.uniform(0.1, 1.0)
    P = port.points(rho, 10, 10, port.camera(367.215, 248.375, 458.654, 457.296))
    a, b = port.normals(P), port.raster_normals(P)
    assert same_bits(a, b).all()
    if gw == 1 or gh == 1:
        assert np.isnan(a).all() and np.isnan(port.areas(P)).all()


def test_border_extrapolation_at_zero():
    """x = 0: ceil(-0.5) = -0 clamps to 0 with floor(-0.5) = -1, so xf = xc = 0 and dx = -0.5; the formula extrapolates there."""
    f, c, d = port.terms(np.array([0, 4, 5, 375]), 10, 37)
    assert list(f) == [0, 0, 0, 36] and list(c) == [0, 0, 0, 36]
    assert d[0] == np.float32(-0.5) and d[1] == np.float32(np.float64(np.float32(0.4)) - 0.5) and d[2] == np.float32(0)
    assert d[3] == np.float32(1.0)   # the partial column clamps to the last cell and extrapolates past it
    # at px = 0 both columns are cell 0 with weights 1.5 and -0.5: the value is the formula's, rounding included
    rho = np.array([[0.3, 2.0], [1.7, 5.0]])
    f32 = np.float32
    for py, (yf, yc) in ((0, (0, 0)), (12, (0, 1)), (19, (1, 1))):
        dy = f32(f32(py) / f32(10)) - f32(0.5) - f32(yf)
        dx = f32(-0.5)
        a, b = f32(rho[yf, 0]), f32(rho[yc, 0])
        want = a * (f32(1) - dx) * (f32(1) - dy) + a * dx * (f32(1) - dy) + b * (f32(1) - dx) * dy + b * dx * dy
        r, _ = port.image_at(rho, rho, 10, 10, np.array([0]), np.array([py]), 1)
        assert bits(r)[0] == bits(np.array([want], np.float32))[0], py


def test_abi_symbols_and_errors_without_gpu_state():
    """The entry points exist; a NULL context is EDGEHIP_ERR_ARG before anything touches a device."""
    lib = edgehip.load_library()
    for s in ("edgehip_depth_surface_enable", "edgehip_depth_surface", "edgehip_download_depth_surface",
              "edgehip_download_depth_surfaces_batch", "edgehip_download_depth_image", "edgehip_download_depth_images_batch",
              "edgehip_depth_image_device"):
        assert hasattr(lib, s), s
    p = edgehip.DepthSurfaceParams(1, 1)
    assert C.sizeof(p) == 8
    assert lib.edgehip_depth_surface_enable(None, C.byref(p)) == -1
    assert lib.edgehip_depth_surface(None) == -1
