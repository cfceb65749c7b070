"""CPU: the dense depth fill (depth_filler).  The numpy restatement (tests/depth_fill_port.py) against the reference's own grids
(tests/golden/depth_fill/*.npz, tools/make_depth_fill_golden.py), hand cases for the corners of FillEdgeData, the skewed wavefront
against the raster Gauss-Seidel loop, and the new C ABI entry points in the built library."""
import ctypes as C
import glob
import math
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import depth_fill_port as port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "depth_fill", "*.npz")))


def golden_cases():
    for path in GOLDEN:
        z = np.load(path)
        for i in range(len(z["cases"])):
            yield pytest.param(path, i, id=f"{os.path.basename(path)[:-4]}-{i}")


def case(z, i):
    lst, bw, bh, it, mode, disc, m = (int(v) for v in z["cases"][i])
    kl = {f: z[f"kl{chr(lst)}_{f}"] for f in port.FIELDS}
    kw = dict(iter_num=it, thresh_rel_rho=float(z[f"case{i}_thresh_rel_rho"]), thresh_match_num=m, bound_mode=mode, discard=disc)
    return kl, bw, bh, kw


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_fixtures_present():
    assert len(GOLDEN) == 2
    assert sum(os.path.getsize(p) for p in GOLDEN) < 3_000_000


@pytest.mark.parametrize("path,i", list(golden_cases()))
def test_port_equals_reference_grids(path, i):
    z = np.load(path)
    kl, bw, bh, kw = case(z, i)
    rho, s_rho, fixed = port.depth_fill(kl, int(z["w"]), int(z["h"]), bw, bh, **kw)
    assert np.array_equal(bits(rho), bits(z[f"case{i}_rho"]))
    assert np.array_equal(bits(s_rho), bits(z[f"case{i}_s_rho"]))
    assert np.array_equal(fixed, z[f"case{i}_fixed"].astype(bool))


def test_fixtures_cover_the_issue_matrix():
    seen = set()
    for path in GOLDEN:
        z = np.load(path)
        w = int(z["w"])
        for lst, bw, bh, it, mode, disc, m in z["cases"]:
            seen |= {("w", w), ("block", int(bw)), ("iter", int(it)), ("mode", int(mode)), ("discard", int(disc))}
            seen.add(("partial", w % int(bw) != 0))
            seen.add(("list", chr(lst), len(z[f"kl{chr(lst)}_rho"]) == 0))
        for k in z.files:
            if k.endswith("_m_num"):
                assert len(z[k]) == 0 or (z[k] >= 5).mean() > 0.05   # a real share of matched KeyLines
    need = {("w", 376), ("w", 752), ("block", 10), ("block", 5), ("iter", 0), ("iter", 1), ("iter", 10), ("mode", 0), ("mode", 1),
            ("mode", 2), ("discard", 0), ("discard", 1), ("partial", True), ("list", "E", True)}
    assert need <= seen, need - seen


def _kl(rows):
    """KeyLine fields from (cx, cy, rho, s_rho, rho0, m_num, p_id, n_id) rows."""
    a = np.array(rows, np.float64).reshape(-1, 8)
    return {"c_p": a[:, :2].astype(np.float32), "rho": a[:, 2], "s_rho": a[:, 3], "rho0": a[:, 4],
            "m_num": a[:, 5].astype(np.int32), "p_id": a[:, 6].astype(np.int32), "n_id": a[:, 7].astype(np.int32)}


def test_nan_keyline_is_folded():
    """s_rho / NaN is NaN, and NaN > thresh is false: the reference does not skip it; NaN <= 0 is false too, so it is not weak."""
    kl = _kl([(3, 3, math.nan, 1.0, 1.0, 9, 0, 0)])
    rho, s_rho, fixed = port.depth_fill(kl, 20, 20, 10, 10, iter_num=0)
    assert fixed[0, 0] and fixed.sum() == 1
    assert math.isnan(rho[0, 0])
    I = 1.0 / 1600.0 + 1.0
    assert s_rho[0, 0] == math.sqrt(1.0 / I)


def test_negative_rho_without_discard_takes_rho0():
    kl = _kl([(3, 3, -2.0, 0.5, 3.0, 9, 0, 0)])
    rho, s_rho, fixed = port.depth_fill(kl, 20, 20, 10, 10, iter_num=0, discard=0)
    I0, kI = 1.0 / 1600.0, 1.0 / 400.0
    i_rho = I0 * 1.0
    i_rho += 3.0 * kI
    I = I0 + kI
    assert fixed[0, 0] and rho[0, 0] == i_rho * (1.0 / I) and s_rho[0, 0] == math.sqrt(1.0 / I)
    _, _, fixed = port.depth_fill(kl, 20, 20, 10, 10, iter_num=0, discard=1)
    assert not fixed.any()


def test_partial_column_wraps_and_last_row_overflow_is_dropped():
    """w = 25, block 10: gw = 2; c_p.x = 21 gives x == gw = 2.  On row 0 that is cell (0, 1); on the last row it is past the grid."""
    good = (9, 0, 0)
    kl = _kl([(21.0, 3.0, 1.0, 0.1, 1.0) + good])
    _, _, fixed = port.depth_fill(kl, 25, 20, 10, 10, iter_num=0)
    assert fixed.tolist() == [[False, False], [True, False]]
    kl = _kl([(21.0, 13.0, 1.0, 0.1, 1.0) + good])
    rho, s_rho, fixed = port.depth_fill(kl, 25, 20, 10, 10, iter_num=0)
    assert not fixed.any() and (rho == 1).all() and (s_rho == 40).all()
    assert port.cell_index(np.array([[21.0, 13.0]], np.float32), 2, 2, 10, 10)[0] == -1


def test_one_wide_grid():
    """gw = 1: no coarse-fine level (sizes must both be > 1); the sweeps average the one or two vertical neighbours."""
    kl = _kl([(5.0, 25.0, 2.0, 0.1, 1.0, 9, 0, 0)])
    rho, s_rho, fixed = port.depth_fill(kl, 10, 50, 10, 10, iter_num=3)
    assert rho.shape == (5, 1) and fixed[:, 0].tolist() == [False, False, True, False, False]
    r2, s2, f2 = port.fill_edge_data(kl, 1, 5, 10, 10, 1.0, 5, 1)
    r2, s2, f2 = r2.reshape(5, 1), s2.reshape(5, 1), f2.reshape(5, 1)
    port.raster_sweeps(r2, s2, f2, 1, 5, 0, 3)
    assert np.array_equal(bits(rho), bits(r2)) and np.array_equal(bits(s_rho), bits(s2))
    assert rho[1, 0] != 1.0


def test_empty_list():
    rho, s_rho, fixed = port.depth_fill(_kl([]), 752, 480, 10, 10, iter_num=10)
    assert rho.shape == (48, 75) and (rho == 1).all() and (s_rho == 40).all() and not fixed.any()


@pytest.mark.parametrize("gw,gh,mode,iters", [(7, 5, 0, 3), (9, 4, 2, 4), (5, 8, 1, 2), (1, 6, 0, 2), (6, 1, 2, 3), (12, 9, 0, 10)])
def test_wavefront_equals_raster_loop(gw, gh, mode, iters):
    """The skewed wavefront t = x + 2y + 4k (what the kernel runs) against Integrate1Step's raster loop, with negative, zero and
    non-finite values in the grid."""
    rng = np.random.default_rng(gw * 100 + gh)
    rho = rng.normal(size=(gh, gw))
    rho[rng.random((gh, gw)) < 0.1] = -0.0
    s_rho = rng.random((gh, gw)) * 3
    fixed = rng.random((gh, gw)) < 0.3
    if gw * gh > 20:
        rho[1, 1] = np.inf
        fixed[1, 1] = True
    a = (rho.copy(), s_rho.copy())
    b = (rho.copy(), s_rho.copy())
    with np.errstate(all="ignore"):
        port.sweeps(a[0], a[1], fixed, gw, gh, mode, iters)
    port.raster_sweeps(b[0], b[1], fixed, gw, gh, mode, iters)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def test_a_skew_of_three_would_not_do():
    """The argument for the skew: with t = x + 2y + 3k, sweep k-1 updates (x+1, y+1) at the step at which sweep k updates (x, y),
    which must read it after that update.  A step computes all its cells from the values before it, so skew 3 departs from the
    raster loop."""
    gw, gh, iters = 6, 5, 3
    rng = np.random.default_rng(3)
    rho, s_rho = rng.normal(size=(gh, gw)), rng.random((gh, gw))
    fixed = np.zeros((gh, gw), bool)
    ref = rho.copy(), s_rho.copy()
    port.raster_sweeps(ref[0], ref[1], fixed, gw, gh, 0, iters)
    r3 = rho.copy()
    for t in range((gw - 1) + 2 * (gh - 1) + 3 * (iters - 1) + 1):
        cells = [(t - 3 * k - 2 * y, y) for k in range(iters) for y in range(gh) if 0 <= t - 3 * k - 2 * y < gw]
        new = {}
        for x, y in cells:
            nb = [r3[y + dy, x + dx] for dy, dx in port._NB if 0 <= x + dx < gw and 0 <= y + dy < gh]
            s = 0.0
            for v in nb:
                s += v
            new[(x, y)] = s / len(nb)
        for (x, y), v in new.items():
            r3[y, x] = v
    assert not np.array_equal(r3, ref[0])


def test_library_exports_depth_fill():
    lib = edgehip.load_library()
    for s in ("edgehip_depth_fill_enable", "edgehip_depth_fill_size", "edgehip_depth_fill", "edgehip_download_depth_grid",
              "edgehip_download_depth_grids_batch"):
        assert hasattr(lib, s), s
        assert s in edgehip.EXPORTS


def test_params_struct_matches_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "edgehip.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   'sizeof(edgehip_depth_fill_params),offsetof(edgehip_depth_fill_params,thresh_rel_rho),'
                   'offsetof(edgehip_depth_fill_params,discard));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    P = edgehip.DepthFillParams
    assert got == [C.sizeof(P), P.thresh_rel_rho.offset, P.discard.offset]
