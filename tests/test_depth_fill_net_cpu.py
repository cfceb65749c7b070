"""CPU: the numpy restatement of the visualizer's depth fill from wire records (tests/depth_fill_net_port.py) against the reference's
own grids (tests/golden/depth_fill_net/*.npz, written by tools/make_depth_fill_net_golden.py): rho, s_rho and fixed equal as bit
patterns, for every fixture."""
import glob
import os

import numpy as np
import pytest

from tests import depth_fill_net_port as port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "depth_fill_net", "*.npz")))
NAMES = ["1_376x240_lds", "2_752x480_hbm", "3_376x240_offset_keep", "4_376x240_all_unmatched", "5_376x240_empty"]


def load(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "depth_fill_net", name + ".npz"))
    bw, bh, it, mode, disc, m = (int(v) for v in z["params"])
    return dict(w=int(z["w"]), h=int(z["h"]), records=z["records"], bw=bw, bh=bh, iter_num=it, bound_mode=mode, discard=disc,
                thresh_match_num=m, thresh_rel_rho=float(z["thresh_rel_rho"]), p_off=tuple(float(v) for v in z["p_off"]),
                want=(z["rho"], z["s_rho"], z["fixed"].astype(bool)))


def run_port(f):
    return port.depth_fill_net(f["records"], f["w"], f["h"], f["bw"], f["bh"], f["iter_num"], f["thresh_rel_rho"], f["thresh_match_num"],
                               f["bound_mode"], f["discard"], f["p_off"])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_the_fixtures_are_the_issue_s():
    assert [os.path.basename(p)[:-4] for p in FIXTURES] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_port_equals_the_reference(name):
    f = load(name)
    rho, s_rho, fixed = run_port(f)
    assert np.array_equal(bits(rho), bits(f["want"][0]))
    assert np.array_equal(bits(s_rho), bits(f["want"][1]))
    assert np.array_equal(fixed, f["want"][2])


def test_the_fixtures_exercise_what_they_are_for():
    f1, f2, f3, f4, f5 = (load(n) for n in NAMES)
    assert f1["want"][0].size * 17 <= 65536 - 2048 < f2["want"][0].size * 17          # grid in LDS / in HBM on the device
    assert f1["want"][2].sum() > 100 and f2["want"][2].sum() > 100
    rec = port.as_records(f3["records"])
    gw, gh = f3["w"] // f3["bw"], f3["h"] // f3["bh"]
    cell = port.cell_index(rec["qx"], rec["qy"], f3["p_off"], gw, gh, f3["bw"], f3["bh"])
    assert f3["discard"] == 0 and (cell < 0).sum() > 50 and (cell >= 0).sum() > 1000   # some records past the grid, most inside
    assert (rec["m_num"] < f3["thresh_match_num"]).sum() > 100                        # ... and weak ones that discard = 0 folds
    assert f4["thresh_match_num"] == 256 and len(f4["records"]) > 1000 and not f4["want"][2].any()
    assert len(f5["records"]) == 0 and (f5["want"][0] == 1.0).all() and (f5["want"][1] == 40.0).all()


def test_the_match_gate_is_the_only_weak_test():
    """Against the edge_tracker overload: no p_id / n_id / rho <= 0 gate.  A record with n_kl = -1 and full match count folds with its own s_rho."""
    rec = np.zeros(2, port.NET_DTYPE)
    rec["qx"], rec["qy"], rec["rho"], rec["s_rho"], rec["n_kl"], rec["m_num"] = (3, 13), (3, 3), (10000, 20000), (1000, 1000), -1, (9, 1)
    rho, s_rho, fixed = port.depth_fill_net(rec, 20, 20, 10, 10, 0, 1.0, 5, 0, 0)
    assert fixed.tolist() == [[True, True], [False, False]]
    I0 = 1.0 / 1600.0
    v = 1.0 / (I0 + 1.0 / (0.1 * 0.1))
    assert rho[0, 0] == (I0 * 1.0 + 1.0 * (1.0 / (0.1 * 0.1))) * v and s_rho[0, 0] == np.sqrt(v)
    v = 1.0 / (I0 + 1.0 / 400.0)                                            # m_num 1 < 5, discard 0: s_rho = RHO_MAX
    assert rho[0, 1] == (I0 * 1.0 + 2.0 * (1.0 / 400.0)) * v and s_rho[0, 1] == np.sqrt(v)
    rho, s_rho, fixed = port.depth_fill_net(rec, 20, 20, 10, 10, 0, 1.0, 5, 0, 1)
    assert fixed.tolist() == [[True, False], [False, False]]
