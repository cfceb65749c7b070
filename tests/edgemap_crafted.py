"""Crafted KeyLine lists for the compressed edge map (edgemap_com_sender::compress_edgemap, src/CommLib/edgemap_com.cpp:162-326), shared
by tools/make_edgemap_golden.py (which writes tests/golden/edgemap/ from the compiled reference), tests/test_edgemap_cpu.py (the host
restatement rebvo_compress_edgemap and the packet codec against that fixture) and tests/test_edgemap_gpu.py (the device against it).

Every list is a few chains laid out by hand; p_id is written from n_id last-writer, as edge_finder::join_edges leaves it, so a head is a
KeyLine nobody names.  case(name) -> (KeyLine list, parameter overrides).  Out of domain and not built: NaN or infinite rho / s_rho and
s_rho <= 0 (the reference's integer conversions are undefined there)."""
import os
import subprocess

import numpy as np

from rebvo_amd import edgehip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 752, 480
MAX_POINTS = 320                 # capacity of the test contexts: the longest crafted list fits
MIN_LEN, MAX_LEN = 3, 20
DEFAULTS = dict(min_line_len=MIN_LEN, max_line_len=MAX_LEN, max_angle=0.3, match_n_t=2, rho_rel_max=1.5, scale=1.0)
NAV = np.arange(1, 18, dtype=np.float32) * np.float32(0.25)   # em_compressed_nav_pkg of the prepared packets: 17 floats
MAX_KL_NUM = 6                   # PreparePkg's max_kl_num: shorter than the longer record lists, so kl_num < kl_total occurs


def camera():
    """(ppx, ppy, zfx, zfy) as cam_model keeps them (float), and zfm = (zfx + zfy) / 2 formed in float."""
    p = edgehip.euroc_params(W, H)
    ppx, ppy, zfx, zfy = (np.float32(v) for v in (p.ppx, p.ppy, p.zfx, p.zfy))
    return float(ppx), float(ppy), float(zfx), float(zfy), float((zfx + zfy) / np.float32(2))


def _blank(n):
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    kl["p_id"], kl["n_id"] = -1, -1
    kl["m_id"], kl["m_id_f"], kl["m_id_kf"], kl["net_id"], kl["stereo_m_id"] = -1, -1, -1, -1, -1
    kl["stereo_rho"], kl["stereo_s_rho"] = 1.0, 20.0
    kl["n_m"] = 1.0
    return kl


def _run(n, x0, y0, dx, dy, rho=1.0, drho=0.002, s_rho=0.05, m_num=5, turn_at=(), turn=0.7):
    """n KeyLines on a polyline from (x0, y0) with step (dx, dy); at every index in turn_at the direction turns by `turn` radians.  u_m is
    the unit normal of the running direction (float), rho a gentle ramp.  Linked i -> i + 1."""
    kl = _blank(n)
    x, y, a = float(x0), float(y0), float(np.arctan2(dy, dx))
    step = float(np.hypot(dx, dy))
    for i in range(n):
        if i in turn_at:
            a += turn
        kl["c_p"][i] = (x, y)
        kl["u_m"][i] = (-np.sin(a), np.cos(a))
        kl["m_m"][i] = kl["u_m"][i]
        kl["rho"][i] = rho + drho * i
        kl["s_rho"][i] = s_rho
        kl["m_num"][i] = m_num
        kl["n_id"][i] = i + 1 if i + 1 < n else -1
        if not turn_at:
            x, y = x0 + dx * (i + 1), y0 + dy * (i + 1)      # exact grid positions on a straight run
        else:
            x, y = x + step * np.cos(a), y + step * np.sin(a)
    return kl


def _cat(*parts):
    """Concatenate chains, shifting their links."""
    out, off = [], 0
    for p in parts:
        p = p.copy()
        p["n_id"] = np.where(p["n_id"] >= 0, p["n_id"] + off, p["n_id"])
        out.append(p)
        off += len(p)
    return np.concatenate(out) if out else _blank(0)


def _finish(kl):
    """p_id from n_id, the last writer in ascending index winning (edge_finder::join_edges); links out of range are left alone."""
    kl["p_id"] = -1
    for k in range(len(kl)):
        n = int(kl["n_id"][k])
        if 0 <= n < len(kl):
            kl["p_id"][n] = k
    return kl


def _cases():
    c = {}
    straight = lambda n, **kw: _run(n, 100, 100, 2, 1, **kw)   # noqa: E731
    # chain lengths around min_line_len (steps = points - 1) and max_line_len (points)
    for steps in (MIN_LEN, MIN_LEN + 1, MIN_LEN + 2):
        c[f"steps_{steps}"] = (_finish(straight(steps + 1)), {})
    for pts in (MAX_LEN - 1, MAX_LEN, MAX_LEN + 7):
        c[f"points_{pts}"] = (_finish(straight(pts)), {})
    # angle cuts
    c["cut_first"] = (_finish(straight(12, turn_at=(1,))), {})                 # turned from step 1: cut at the first step past min_line_len
    c["cut_middle"] = (_finish(straight(16, turn_at=(8,))), {})                # then a long tail: final fit, shared vertex
    c["cut_last"] = (_finish(straight(10, turn_at=(9,))), {})                  # cut at the last step: the pending vertex is negated
    c["cut_twice"] = (_finish(straight(19, turn_at=(6, 12))), {})              # two cuts in a row
    c["cut_short_tail"] = (_finish(straight(11, turn_at=(8,))), {})            # cut, then a tail of <= min_line_len steps
    # depth ratio on and just past rho_rel_max, both directions
    for name, a, b in (("ratio_on_up", 1.0, 1.5), ("ratio_past_up", 1.0, float(np.nextafter(1.5, 2.0))),
                       ("ratio_on_down", 1.5, 1.0), ("ratio_past_down", float(np.nextafter(1.5, 2.0)), 1.0)):
        kl = straight(12, drho=0.0)
        kl["rho"][:6], kl["rho"][6:] = a, b
        c[name] = (_finish(kl), {})
    kl = straight(2, drho=0.0)
    kl["rho"][1] = 2.0                                 # line_len counts the step whose KeyLine never entered the fit list: with
    c["single_point"] = (_finish(kl), dict(min_line_len=0))   # min_line_len 0 the final fit is of the head alone
    # two heads that merge
    a = straight(16)                                   # A: 0..15, fitted to its end: the shared tail stays masked
    b = _run(6, 60, 300, 2, 0)
    kl = _cat(a, b)
    kl["n_id"][len(kl) - 1] = 8                        # B runs into A's KeyLine 8
    c["merge_masked"] = (_finish(kl), {})
    a = straight(13, turn_at=(10,))                    # A: cut at 10, tail 11, 12 unfitted: 10..12 unmasked again
    kl = _cat(a, b)
    kl["n_id"][len(kl) - 1] = 11                       # B runs into the unmasked tail and walks it again
    c["merge_rewalk"] = (_finish(kl), {})
    # graph shapes
    kl = straight(7)
    kl["n_id"][6] = 5                                  # ... -> 5 -> 6 -> 5
    c["cycle_2"] = (_finish(kl), {})
    kl = straight(11)
    kl["n_id"][10] = 6                                 # ... -> 6 -> 7 -> 8 -> 9 -> 10 -> 6
    c["cycle_5"] = (_finish(kl), {})
    kl = straight(6)
    kl["n_id"][5] = 5
    c["self_link"] = (_finish(kl), {})
    c["isolated"] = (_finish(_cat(straight(1), straight(8))), {})
    kl = straight(9)
    kl["n_id"][8] = 0                                  # one ring: nobody is a head
    c["no_head"] = (_finish(kl), {})
    c["kn_0"] = (_blank(0), {})
    c["kn_1"] = (_finish(straight(1)), {})
    # fit edge cases
    c["vertical"] = (_finish(_run(9, 200, 50, 0, 3)), {})
    c["horizontal"] = (_finish(_run(9, 50, 200, 3, 0)), {})
    c["diagonal"] = (_finish(_run(9, 50, 60, 2, 2)), {})
    c["antidiagonal"] = (_finish(_run(9, 50, 260, 2, -2)), {})
    c["identical"] = (_finish(_run(8, 120, 90, 0, 0)), {})       # degenerate system: p0 / p1 stay homogeneous, negative, clamp at 0
    c["unmatched"] = (_finish(straight(9, m_num=1)), {})        # every m_num below match_n_t: every s_rho 1e10, degenerate
    kl = straight(10, drho=0.0)                                  # a depth bow: neighbours at most 0.04 apart (s_rho 0.05), but the ends
    kl["rho"] = 1.0 + 0.005 * (np.arange(10) - 4.5) ** 2         # lie 0.06 off the fitted line: the residual rule alone gives sigma 1e10
    c["outlier"] = (_finish(kl), {})
    kl = straight(10, drho=0.0)
    kl["rho"][5:] = 1.2                                          # neighbours 0.2 apart, s_rho 0.05 (ratio 1.2 < rho_rel_max)
    c["neighbour_jump"] = (_finish(kl), {})
    c["rho_ceiling"] = (_finish(straight(9, rho=25.0)), {})      # 25 * 1638.35 > 32767
    c["rho_floor"] = (_finish(straight(9, rho=1e-5, drho=1e-8, s_rho=1e-6)), {})
    c["xy_clamp"] = (_finish(_run(9, 600, 300, 4, 5)), {})       # x > 510, y > 255
    c["scale"] = (_finish(straight(12)), dict(scale=2.5))
    # several chains of different kinds in one list, chains interleaved in index order
    c["mixed"] = (_finish(_cat(straight(16, turn_at=(8,)), _run(9, 200, 50, 0, 3), straight(1), straight(27), _run(6, 60, 300, 2, 0))), {})
    return c


_CASES = None


def names():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return list(_CASES)


def case(name):
    """-> (KeyLine list, parameters): DEFAULTS with the case's overrides."""
    names()
    kl, over = _CASES[name]
    p = dict(DEFAULTS)
    p.update(over)
    return kl.copy(), p


def params_struct(p):
    q = edgehip.EdgemapParams()
    q.min_line_len, q.max_line_len, q.match_n_t = p["min_line_len"], p["max_line_len"], p["match_n_t"]
    q.max_angle, q.rho_rel_max = p["max_angle"], p["rho_rel_max"]
    q.x_scaling, q.y_scaling = p.get("x_scaling", 0.0), p.get("y_scaling", 0.0)
    return q


# ---- the host restatement (rebvo/edgemap_com.h) through a small program built on first use -------------------------------------------
HOST_TOOL_SRC = os.path.join(ROOT, "tools", "edgemap_host_check.cpp")


def build_host_tool(out_dir):
    exe = os.path.join(str(out_dir), "edgemap_host_check")
    inc = [os.path.join(ROOT, *q) for q in (("rebvo_amd", "host", "include"), ("include",), ("rebvo_amd", "csrc"))]
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + ["-I" + i for i in inc] + [HOST_TOOL_SRC, "-o", exe], check=True)
    return exe


def host_run(exe, kl, p, cap, cam=None, nav=NAV, max_kl_num=MAX_KL_NUM):
    """tools/edgemap_host_check.cpp on one list -> dict(records (n, 5) uint8, count, status, sent, packet uint8, segments (m, 8) float32,
    trace (f, 6) int32: start, n, the bit patterns of tx, ty, zfo, flags)."""
    ppx, ppy, _, _, zfm = cam or camera()
    kl = np.ascontiguousarray(kl, dtype=edgehip.KEYLINE_DTYPE)
    hdr = np.array([len(kl), p["min_line_len"], p["max_line_len"], p["match_n_t"], max_kl_num, cap], np.int32).tobytes()
    dv = np.array([p["scale"], p["max_angle"], p["rho_rel_max"], p.get("x_scaling", 0.0), p.get("y_scaling", 0.0), zfm], np.float64).tobytes()
    payload = hdr + dv + np.array([ppx, ppy], np.float32).tobytes() + np.asarray(nav, np.float32).tobytes() + kl.tobytes()
    out = subprocess.run([exe], input=payload, check=True, capture_output=True).stdout
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(out, dtype, n, at).copy()
        at += a.nbytes
        return a

    count, status = (int(v) for v in take(np.int32, 2))
    r = {"count": count, "status": status, "records": take(np.uint8, 5 * count).reshape(count, 5)}
    r["sent"], plen = (int(v) for v in take(np.int32, 2))
    r["packet"] = take(np.uint8, plen)
    nseg = int(take(np.int32, 1)[0])
    r["segments"] = take(np.float32, 8 * nseg).reshape(nseg, 8)
    nfit = int(take(np.int32, 1)[0])
    r["trace"] = take(np.int32, 6 * nfit).reshape(nfit, 6)
    assert at == len(out)
    return r
