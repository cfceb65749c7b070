"""Crafted KeyLine lists for the ROS nodelet's per-KeyLine output (rebvo_nodelet.cpp:176-212: one xyz point, one Keyline.msg record),
shared by tests/test_ros_edgemap_cpu.py (host packer against the reference's own arithmetic, tests/golden/ros_edgemap/crafted.npz),
tests/test_ros_edgemap_gpu.py (device packer against the host packer) and tools/make_ros_edgemap_golden.py (which writes the fixture).

One list per sequence, lengths (0, 1, 37, max_points), a distinct K each.  KeyLine j takes rho kind j % 7 and p_m kind j % 5 — 35
combinations, all inside the 37-KeyLine list — and ids, match counts and the remaining fields from cycles of other lengths."""
import ctypes as C
import os

import numpy as np

from rebvo_amd import edgehip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so")
W, H = 376, 240
MAX_POINTS = (67, 128)          # 67: strides of 804 B and 3484 B, sequences start inside a 16-byte word; 128: word-aligned
K_PROF = (1.0, 2.5, 0.7, 1.3)   # one scale per list
RHO_KINDS = ("plain", "zero", "negative", "tiny", "huge", "overflow", "nan")
PM_KINDS = ("zero", "plus", "minus", "tie_x", "tie_z")
IDS = (-1, 0, 32767, 32768, 40000, 65535, 70000)   # p_id / n_id: the low 16 bits are what the message keeps
INT32 = (-2 ** 31, 2 ** 31 - 1, 0, -1, 7)


def zfm_of(params):
    """cam_model's zfm (include/UtilLib/cam_model.h:51-52): the mean of the two float focal lengths, formed in float."""
    return float((np.float32(params.zfx) + np.float32(params.zfy)) / np.float32(2))


ZFM = zfm_of(edgehip.euroc_params(W, H))


def _tie_rho(px, K, zfm, which, start):
    """A rho for which x = px / (rho / K) / zfm (which = 0) or z = 1 / (rho / K) (which = 1) is, in fp64, exactly half way between two
    neighbouring floats: the narrowing to float is then decided by round-to-nearest-EVEN alone.  Found by trying tie values one after
    the other and checking the forward computation in fp64 (numpy's float64 operations are IEEE)."""
    px, K, zfm = np.float64(px), np.float64(K), np.float64(zfm)
    for m in range(start, start + 4000):
        t = np.float64(1.0) + np.float64(2 * m + 1) * np.float64(2.0) ** -24   # 25 significant bits, the last one set
        q = (px / (t * zfm)) if which == 0 else (np.float64(1.0) / t)
        rho = q * K
        with np.errstate(all="ignore"):
            qq = rho / K
            got = (px / qq / zfm) if which == 0 else (np.float64(1.0) / qq)
        if got == t:
            return float(rho)
    raise AssertionError("no tie found")


def _list(n, which, zfm=ZFM):
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    K = K_PROF[which]
    for j in range(n):
        rk, pk = RHO_KINDS[j % 7], PM_KINDS[j % 5]
        px, py = {"zero": (0.0, 0.0), "plus": (0.05 + j, 17.5), "minus": (-0.03, -101.25 - j), "tie_x": (3.0 + j, -0.04),
                  "tie_z": (-7.25, 0.02 + j)}[pk]
        px, py = np.float32(px), np.float32(py)
        rho = {"plain": 0.8 + 0.01 * j, "zero": 0.0 if j % 2 else -0.0, "negative": -0.3 - 0.01 * j, "tiny": 1e-300, "huge": 1e35,
               "overflow": 1e-40, "nan": float("nan")}[rk]
        if rk == "plain" and pk == "tie_x":
            rho = _tie_rho(px, K, zfm, 0, 100 + j)
        elif rk == "plain" and pk == "tie_z":
            rho = _tie_rho(px, K, zfm, 1, 200 + j)
        kl["p_m"][j] = (px, py)
        kl["rho"][j] = rho
        kl["s_rho"][j] = 0.001 + 0.37 * j          # distinct per record, like m_m and c_p: a swapped field shows
        kl["m_m"][j] = (0.5 + j, -1.25 - 2 * j)
        kl["c_p"][j] = (10.25 + j, 200.5 - j)
        kl["p_id"][j] = IDS[j % 7]
        kl["n_id"][j] = IDS[(j * 3 + 2) % 7]
        kl["m_id"][j] = INT32[j % 5]
        kl["m_num"][j] = INT32[(j * 2 + 1) % 5]
    kl["u_m"] = (1.0, 0.0)
    kl["n_m"] = 1.0
    kl["m_id_f"] = -1
    kl["m_id_kf"] = -1
    kl["net_id"] = -1
    kl["stereo_m_id"] = -1
    kl["stereo_rho"], kl["stereo_s_rho"] = 1.0, 20.0
    return kl


def crafted_lists(max_points):
    """[KeyLine list] per sequence: lengths 0, 1, 37, max_points.  A list is a prefix of the longer ones' pattern, scaled by its own K."""
    return [_list(n, which) for which, n in enumerate((0, 1, 37, max_points))]


def host_pack(kl, K, zfm):
    """rebvo_pack_ros_edgemap of the host library -> (points (n, 12) uint8, records (n, 52) uint8)."""
    host = C.CDLL(HOST)
    host.rebvo_pack_ros_edgemap.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    host.rebvo_pack_ros_edgemap.restype = None
    kl = np.ascontiguousarray(kl)
    pts, recs = np.zeros((len(kl), 12), np.uint8), np.zeros((len(kl), 52), np.uint8)
    host.rebvo_pack_ros_edgemap(kl.ctypes.data, len(kl), float(K), float(zfm), pts.ctypes.data, recs.ctypes.data)
    return pts, recs


def same_points(got, want):
    """Point bytes (n, 12) equal, a NaN counting as equal to any NaN at the same position (the sign and payload of a NaN that a division
    creates are the one thing the reference does not define)."""
    g = np.ascontiguousarray(got).view(np.float32).reshape(-1, 3)
    w = np.ascontiguousarray(want).view(np.float32).reshape(-1, 3)
    if g.shape != w.shape:
        return False
    gn, wn = np.isnan(g), np.isnan(w)
    return bool(np.array_equal(gn, wn) and np.array_equal(g.view(np.uint32)[~gn], w.view(np.uint32)[~wn]))


def same_records(got, want):
    """Record bytes (n, 52) equal; invDepth / invDepthS (bytes 16..32) that are NaN on both sides count as equal."""
    g = np.ascontiguousarray(got).reshape(-1, 52)
    w = np.ascontiguousarray(want).reshape(-1, 52)
    if g.shape != w.shape:
        return False
    gd = np.ascontiguousarray(g[:, 16:32]).view(np.float64)
    wd = np.ascontiguousarray(w[:, 16:32]).view(np.float64)
    gn, wn = np.isnan(gd), np.isnan(wd)
    return bool(np.array_equal(g[:, :16], w[:, :16]) and np.array_equal(g[:, 32:], w[:, 32:]) and np.array_equal(gn, wn) and
                np.array_equal(gd.view(np.uint64)[~gn], wd.view(np.uint64)[~wn]))


def populations(lists, zfm=ZFM):
    """How many crafted KeyLines sit in each corner case, from the inputs and fp64 arithmetic alone."""
    p = dict.fromkeys(["inf", "nan_created", "nan_carried", "negative", "denormal", "overflow", "tie", "id_wraps", "int32_extreme"], 0)
    for which, kl in enumerate(lists):
        K = np.float64(K_PROF[which])
        with np.errstate(all="ignore"):
            q = kl["rho"] / K
            x = kl["p_m"][:, 0].astype(np.float64) / q / zfm
            y = kl["p_m"][:, 1].astype(np.float64) / q / zfm
            z = 1.0 / q
            f = np.stack([x, y, z], 1).astype(np.float32)
        p["inf"] += int(np.isinf(np.stack([x, y, z], 1)).sum())
        p["nan_created"] += int((np.isnan(x) & ~np.isnan(kl["rho"])).sum())
        p["nan_carried"] += int(np.isnan(kl["rho"]).sum())
        p["negative"] += int((kl["rho"] < 0).sum())
        p["denormal"] += int(((f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)).sum())
        p["overflow"] += int((np.isinf(f) & np.isfinite(np.stack([x, y, z], 1))).sum())
        for v in (x, y, z):
            fin = np.isfinite(v) & (v != 0)
            m = np.frexp(v[fin])[0] * 2.0 ** 25          # 25 significant bits in front of the point
            p["tie"] += int(((m == np.floor(m)) & (np.floor(m) % 2 == 1)).sum())
        p["id_wraps"] += int(((kl["p_id"] > 32767) | (kl["n_id"] > 32767)).sum())
        p["int32_extreme"] += int((np.abs(kl["m_id"].astype(np.int64)) >= 2 ** 31 - 1).sum())
    return p
