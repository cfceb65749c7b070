"""Crafted compressed_kl record lists for the receiving side of the compressed edge map (edgemap_com_decoder: Decode, HideVisible,
fillDepthMap), shared by tools/make_edgemap_decode_golden.py (which writes tests/golden/edgemap_decode/ from the compiled reference),
tests/test_edgemap_decode_cpu.py and tests/test_edgemap_decode_gpu.py.

The image is 64x48 with 8-px blocks: a 8x6 grid.  A record's x byte is half its pixel column (COMPRESSED_X_SCALING 0.5), its y byte the
pixel row; rho is in units of 20 / 32767 (times rho_scale), s_rho in units of 20 / 255.  Every list is there for one branch; case(name)
-> dict(records, rho_scale, v_thresh, a_thresh).  Out of domain and not built: a rho_scale that is not finite or <= 0 (refused)."""
import os
import subprocess

import numpy as np

from rebvo_amd import edgehip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, BW, BH = 64, 48, 8, 8
ITER_NUM, BOUND_MODE = 4, 0
CAM = (32.0, 24.0, 60.0, 60.0, 60.0)        # ppx, ppy, zfx, zfy, zfm
V_THRESH, A_THRESH = 2.0, 45.0
CAP_RECORDS, CAP_SEGMENTS, CAP_ITEMS = 64, 32, 512
ONE = 1638                                   # rho 1.0 at rho_scale 1


def nav(p=(0, 0, 0), w=(0, 0, 0), K=1.0):
    """em_compressed_nav_pkg as 17 floats."""
    n = np.zeros(17, np.float32)
    n[0:3], n[3:6], n[12] = p, w, K
    return n


EM_NAV = nav(p=(0.05, -0.02, 0.1), w=(0.01, -0.02, 0.015), K=1.25)
# the views of HideVisible, in the order they are applied: a turn to either side, a view from beyond the points, a view with another K
VIEWS = (nav(p=(0.1, 0.0, 0.2), w=(0.0, 0.6, 0.0), K=1.0), nav(p=(-0.1, 0.05, 0.0), w=(0.05, -0.6, 0.02), K=0.8),
         nav(p=(0.0, 0.0, 9.0), K=1.0), nav(p=(0.3, 0.1, -0.5), w=(0.3, 0.1, -0.2), K=2.0))


def R(x, y, rho, s=3):
    return (x, y, rho, s)


def _ratio(rho, s):
    """kl.rho / kl.s_rho of a record at rho_scale 1, in getPair's float operations."""
    f = np.float32
    return float(f(f(rho) / f(f(32767.0 / 20) / f(1.0))) / f(f(s) / f(255.0 / 20)))


def _rec(rows):
    a = np.zeros(len(rows), edgehip.COMPRESSED_KL_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a


def _cases():
    c = {}

    def add(name, rows, **kw):
        c[name] = dict(dict(records=_rec(rows), rho_scale=1.0, v_thresh=V_THRESH, a_thresh=A_THRESH), **kw)

    add("empty", [])
    add("one_record", [R(4, 10, ONE)])
    add("horizontal_nt_integer", [R(4, 10, ONE), R(20, 10, -ONE - 300)])            # 8 .. 40 px: nt = 32
    add("diagonal", [R(3, 5, ONE), R(17, 33, -2 * ONE)])                            # nt not an integer
    add("shared_vertex", [R(2, 4, ONE), R(12, 9, ONE + 200), R(25, 30, -ONE - 500)])
    add("open_polyline", [R(2, 40, ONE), R(14, 36, ONE + 100)])                     # the last record is a partner only
    add("negative_k0", [R(2, 4, ONE), R(10, 4, -ONE), R(20, 20, -ONE), R(5, 30, ONE), R(9, 44, -ONE)])
    add("zeros_between", [R(2, 4, ONE), R(10, 8, -ONE), R(0, 0, 0), R(0, 0, 0), R(20, 30, ONE), R(28, 40, -ONE)])
    add("degenerate_before_zero", [R(6, 6, ONE), R(0, 0, 0), R(8, 20, ONE), R(16, 20, -ONE)])
    add("leading_negative", [R(6, 6, -ONE), R(8, 20, ONE), R(16, 22, -ONE)])
    add("s_rho_byte_0", [R(4, 12, ONE, 0), R(18, 14, -ONE, 0)])
    add("s_rho_byte_0_one_end", [R(4, 30, ONE, 0), R(18, 34, -ONE, 20)])
    add("gate_sigma_k0", [R(4, 10, 32767, 255), R(20, 12, -32767, 5)])
    add("gate_sigma_k1", [R(4, 10, 32767, 5), R(20, 12, -32767, 255)])
    add("gate_sum", [R(4, 10, ONE, 200), R(20, 12, -ONE, 200)])
    add("gate_rel_k0", [R(4, 10, ONE, 10), R(20, 12, -4 * ONE, 5)])                 # 1.0 / 0.78 < 2
    add("gate_rel_k1", [R(4, 10, 4 * ONE, 5), R(20, 12, -ONE, 10)])
    add("gate_rel_on_threshold", [R(4, 10, ONE, 5), R(20, 12, -ONE, 5)], v_thresh=_ratio(ONE, 5))   # rho / s_rho == v_thresh: folded
    add("gate_angle", [R(22, 24, ONE), R(31, 24, -ONE), R(14, 20, ONE), R(16, 28, -ONE)], a_thresh=80.0)   # radial far out; tangential near the centre
    add("clamp_right_bottom", [R(29, 44, ONE), R(40, 60, -ONE)])                    # past 64 x 48: getImgPoint clamps
    add("clamp_right_edge", [R(36, 2, ONE), R(36, 46, -ONE)])
    add("cross_ab", [R(4, 10, ONE), R(12, 18, -ONE), R(4, 18, 3 * ONE, 6), R(12, 10, -3 * ONE, 6)])   # both pass through cells (1, 1) and (2, 1)
    add("cross_ba", [R(4, 18, 3 * ONE, 6), R(12, 10, -3 * ONE, 6), R(4, 10, ONE), R(12, 18, -ONE)])
    add("on_cell_boundary", [R(8, 16, ONE), R(20, 16, -ONE), R(12, 8, ONE), R(12, 32, -ONE)])   # starts at x = 16, y = 16 and runs along y = 16 / x = 24
    add("backwards", [R(28, 40, ONE), R(3, 2, -2 * ONE)])                           # negative direction
    add("rho_scale", [R(4, 10, ONE), R(20, 30, -ONE - 300), R(6, 40, 2 * ONE), R(26, 44, -ONE)], rho_scale=2.5)
    add("mixed", [R(2, 4, ONE), R(12, 9, ONE + 200), R(25, 30, -ONE - 500), R(0, 0, 0), R(30, 2, ONE, 0), R(20, 2, 2 * ONE, 3), R(6, 6, -ONE, 255),
                  R(9, 9, -ONE), R(0, 0, 0), R(1, 45, ONE, 7), R(31, 47, -ONE, 9), R(16, 24, ONE), R(16, 24, -ONE)])
    return c


_CASES = None


def names():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return list(_CASES)


def case(name):
    names()
    d = dict(_CASES[name])
    d["records"] = d["records"].copy()
    return d


# ---- the host restatement (rebvo/edgemap_com.h) through a small program built on first use --------------------------------------------
HOST_TOOL_SRC = os.path.join(ROOT, "tools", "edgemap_decode_host_check.cpp")


def build_host_tool(out_dir):
    exe = os.path.join(str(out_dir), "edgemap_decode_host_check")
    inc = [os.path.join(ROOT, *q) for q in (("rebvo_amd", "host", "include"), ("include",), ("rebvo_amd", "csrc"))]
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + ["-I" + i for i in inc] + [HOST_TOOL_SRC, "-o", exe], check=True)
    return exe


def payload(records, rho_scale, v_thresh, a_thresh, size=(W, H), block=(BW, BH), cam=CAM, em_nav=EM_NAV, views=VIEWS, iter_num=ITER_NUM,
            bound_mode=BOUND_MODE, use_visibility=False, reps=0, x_scaling=0.0, y_scaling=0.0):
    """The input both tools/edgemap_decode_host_check.cpp and tools/edgemap_decode_ref_driver.cpp read."""
    rec = np.ascontiguousarray(records, edgehip.COMPRESSED_KL_DTYPE)
    hdr = np.array([len(rec), size[0], size[1], block[0], block[1], iter_num, bound_mode, len(views), int(use_visibility), reps], np.int32)
    fv = np.array([rho_scale, cam[0], cam[1], cam[2], cam[3]], np.float32)
    dv = np.array([cam[4], v_thresh, a_thresh, x_scaling, y_scaling], np.float64)
    return hdr.tobytes() + fv.tobytes() + dv.tobytes() + np.asarray(em_nav, np.float32).tobytes() + \
        b"".join(np.asarray(v, np.float32).tobytes() for v in views) + rec.tobytes()


def parse(out, nviews, G, host):
    """The output of either tool -> dict(segments, dpose, dpos, flags (per view), s_num, fill = (rho, s_rho, fixed),
    and gates + steps (host) or chain = (rho, s_rho, fixed) (reference))."""
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(out, dtype, n, at).copy()
        at += a.nbytes
        return a

    nseg = int(take(np.int32, 1)[0])
    r = {"segments": take(np.float32, 8 * nseg).reshape(nseg, 8), "dpose": [], "dpos": [], "flags": [], "s_num": []}
    for _ in range(nviews):
        r["dpose"].append(take(np.float64, 9).reshape(3, 3))
        r["dpos"].append(take(np.float64, 3))
        r["flags"].append(take(np.uint8, nseg))
        r["s_num"].append(int(take(np.int32, 1)[0]))
    r["fill"] = (take(np.float64, G), take(np.float64, G), take(np.uint8, G))
    if host:
        r["gates"] = take(np.int32, nseg)
        r["steps"] = int(take(np.int64, 1)[0])
    else:
        r["chain"] = (take(np.float64, G), take(np.float64, G), take(np.uint8, G))
    assert at == len(out), (at, len(out))
    return r


def host_run(exe, records, rho_scale, v_thresh, a_thresh, **kw):
    size, block, views = kw.get("size", (W, H)), kw.get("block", (BW, BH)), kw.get("views", VIEWS)
    out = subprocess.run([exe], input=payload(records, rho_scale, v_thresh, a_thresh, **kw), check=True, capture_output=True).stdout
    return parse(out, len(views), (size[0] // block[0]) * (size[1] // block[1]), True)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
GOLD = os.path.join(ROOT, "tests", "golden", "edgemap_decode")
SETS = ("crafted", "billboard")


def load(which):
    """tests/golden/edgemap_decode/<which>.npz -> (meta dict, {case name: dict of arrays})."""
    g = np.load(os.path.join(GOLD, which + ".npz"))
    cases = {}
    for k in g.files:
        if "__" in k:
            tag, f = k.split("__", 1)
            cases.setdefault(tag, {})[f] = g[k]
    meta = {k: g[k] for k in g.files if "__" not in k}
    return meta, cases


def bits(a):
    return np.ascontiguousarray(a).view(np.int64 if np.asarray(a).dtype == np.float64 else np.int32)
