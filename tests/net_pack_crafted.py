"""Crafted KeyLine lists that drive every branch of the wire-format packer (copy_net_keyline + copy_net_keyline_nextid,
src/CommLib/net_keypoint.cpp:29-108), shared by tests/test_net_pack_crafted_cpu.py (reference packer against the host packer) and
tests/test_net_pack_gpu.py (device packer against the host packer).  Everything lies where the reference is defined: finite values,
positions inside a 376x240 image, stereo ids inside the pair list."""
import ctypes as C
import os

import numpy as np

from rebvo_amd import edgehip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so")
W, H = 376, 240
KL_SIZE = 64                    # records per sequence: 64 * 15 = 960 B, a whole number of 16-byte words: every sequence starts on a word
KL_SIZE_ODD = 67                # 67 * 15 = 1005 B: sequences 1 .. 3 start inside a word, where a vector store would run into the neighbour
LENGTHS = (0, 1, 37, 69)        # empty; one record; a tail that ends inside a 16-byte word (555 B); longer than KL_SIZE
K_PROF = (1.0, 2.5, 0.7, 1.3)   # one scale per list

# c_p: .5 ties on either axis (round half away from zero), plain values, the image's corners
C_P = [(10.5, 20.5), (11.5, 7.0), (12.25, 100.5), (100.0, 33.75), (0.5, 0.5), (374.5, 238.5), (0.0, 239.0), (375.0, 0.0), (200.49, 120.51)]
# rho, s_rho as multiples of k_prof: 0; negative; just below / above the clamp at 6.5535; small enough for the max(., 1) floor; plain
RHO = [0.0, -0.3, np.nextafter(6.5535, 0.0), 6.5536, 7.5, 0.00005, 0.00015, 0.8, 1.7, 3.14159]
M_NUM = [0, 255, 256, 100000, 3, 7, 254, 1]
# matched displacement p_m - p_m_0 (p_m_0 = 0): products * 10 at -127.x, 0, +128.x, beyond either clamp, and .5 ties of the sum
FLOW = [-12.73, 0.0, 12.83, -13.0, 20.0, 0.25, -0.25, 0.05, 1.0, -12.75, 12.75, 3.3]
# stereo disparity per axis: at the 127 gate (126 passes, 127 and 128 do not), negative, ties, none
DISP = [126.0, 127.0, 128.0, -126.0, -127.0, -128.0, 0.0, 3.5, -3.5, 126.4, 126.5, -126.5, 50.0]


def _list(n, which):
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    i = np.arange(n)
    k = K_PROF[which]
    kl["c_p"] = np.array([C_P[j % len(C_P)] for j in i], np.float32).reshape(n, 2)
    kl["rho"] = np.array([RHO[j % len(RHO)] * k for j in i], np.float64)
    kl["s_rho"] = np.array([RHO[(j * 3 + 1) % len(RHO)] * k for j in i], np.float64)
    kl["m_num"] = np.array([M_NUM[j % len(M_NUM)] for j in i], np.int32)
    kl["p_m_0"] = np.array([(1.0, -2.0)] * n, np.float32).reshape(n, 2)
    kl["p_m"][:, 0] = kl["p_m_0"][:, 0] + np.array([FLOW[j % len(FLOW)] for j in i], np.float32)
    kl["p_m"][:, 1] = kl["p_m_0"][:, 1] + np.array([FLOW[(j * 5 + 2) % len(FLOW)] for j in i], np.float32)
    # n_id: none for every third KeyLine, else the next KeyLine but one (wrapping) — on the long list that reaches ids >= KL_SIZE
    nid = np.where(i % 3 == 0, -1, (i + 2) % max(n, 1)).astype(np.int32)
    if n > KL_SIZE:
        nid[5], nid[11] = KL_SIZE, n - 1          # packed KeyLines that name unpacked ones
    kl["n_id"] = nid
    kl["p_id"] = np.where(i % 4 == 0, -1, (i - 1) % max(n, 1)).astype(np.int32)
    kl["m_id"] = -1
    kl["m_id_f"] = -1
    kl["m_id_kf"] = -1
    kl["net_id"] = -1                             # a fresh list: no net_id is stale
    kl["stereo_m_id"] = -1
    kl["stereo_rho"], kl["stereo_s_rho"] = 1.0, 20.0
    kl["m_m"] = (1.0, 0.0)
    kl["u_m"] = (1.0, 0.0)
    kl["n_m"] = 1.0
    return kl


def crafted_lists():
    """[(KeyLine list, pair list)] per sequence.  The pair list holds, for KeyLine i with a stereo match, a KeyLine at c_p + disparity."""
    out = []
    for which, n in enumerate(LENGTHS):
        kl = _list(n, which)
        pair = _list(n, which)
        i = np.arange(n)
        sm = np.where(i % 5 == 4, -1, (i * 7 + 3) % max(n, 1)).astype(np.int32)   # a permutation's worth of ids, some none
        kl["stereo_m_id"] = sm
        for j in range(n):
            if sm[j] >= 0:
                # every second KeyLine gets a tame disparity on one axis, so that the other axis alone decides the gate
                dx, dy = DISP[j % len(DISP)], DISP[(j * 3 + 1) % len(DISP)]
                if j % 4 == 1:
                    dy = 2.0
                elif j % 4 == 3:
                    dx = -7.5
                pair["c_p"][sm[j]] = kl["c_p"][j] + np.array([dx, dy], np.float32)
        out.append((kl, pair))
    return out


def host_pack(kl, pair, kl_size, k_prof, fill=0):
    """rebvo_copy_net_keyline + rebvo_copy_net_keyline_nextid of the host library on a copy of `kl` -> (records (kl_size, 15) uint8 with
    the bytes behind the packed records left at `fill`, count)."""
    host = C.CDLL(HOST)
    host.rebvo_copy_net_keyline.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double]
    host.rebvo_copy_net_keyline_nextid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    kl = np.ascontiguousarray(kl.copy())
    kl["net_id"] = -1
    out = np.full((kl_size, 15), fill, np.uint8)
    pp = np.ascontiguousarray(pair) if pair is not None else None
    n = host.rebvo_copy_net_keyline(kl.ctypes.data, len(kl), pp.ctypes.data if pp is not None and len(pp) else None, out.ctypes.data,
                                    kl_size, float(k_prof))
    if pp is not None and len(pp) == 0:   # an empty pair list still selects the stereo arm; nothing is packed either way
        assert n == 0
    host.rebvo_copy_net_keyline_nextid(kl.ctypes.data, len(kl), out.ctypes.data, kl_size)
    return out, n


def populations(lists, kl_size=KL_SIZE):
    """How many PACKED KeyLines of the crafted lists sit in each branch of the packer, from the inputs alone."""
    p = dict.fromkeys(["cp_tie", "rho_zero", "rho_neg", "rho_below_clamp", "rho_above_clamp", "rho_floor", "m0", "m255", "m256", "m_big",
                       "flow_neg", "flow_zero", "flow_over", "flow_tie", "nid_none", "nid_in", "nid_past", "st_none", "st_126", "st_127",
                       "st_128", "st_pass", "st_gated"], 0)
    for which, (kl, pair) in enumerate(lists):
        n = min(len(kl), kl_size)
        k = K_PROF[which]
        a = kl[:n]
        p["cp_tie"] += int(((a["c_p"] % 1) == 0.5).any(axis=1).sum())
        for f in ("rho", "s_rho"):
            q = np.float32(10000.0 * a[f] / k)
            p["rho_zero"] += int((a[f] == 0).sum())
            p["rho_neg"] += int((a[f] < 0).sum())
            p["rho_below_clamp"] += int(((q > 65534) & (q <= 65535)).sum())
            p["rho_above_clamp"] += int((q > 65535).sum())
            p["rho_floor"] += int(((q > 0) & (q < 1)).sum())
        p["m0"] += int((a["m_num"] == 0).sum())
        p["m255"] += int((a["m_num"] == 255).sum())
        p["m256"] += int((a["m_num"] == 256).sum())
        p["m_big"] += int((a["m_num"] > 256).sum())
        d = ((a["p_m"] - a["p_m_0"]) * np.float32(10)).astype(np.float64) + 127.0
        p["flow_neg"] += int((d < 0).sum())
        p["flow_zero"] += int((d == 127.0).sum())
        p["flow_over"] += int((d > 255).sum())
        p["flow_tie"] += int(((d % 1) == 0.5).sum())
        p["nid_none"] += int((a["n_id"] < 0).sum())
        p["nid_in"] += int(((a["n_id"] >= 0) & (a["n_id"] < n)).sum())
        p["nid_past"] += int((a["n_id"] >= kl_size).sum())
        sm = a["stereo_m_id"]
        p["st_none"] += int((sm < 0).sum())
        has = sm >= 0
        disp = np.abs(np.round((-a["c_p"][has] + pair["c_p"][sm[has]]).astype(np.float64)))
        for v in (126, 127, 128):
            p[f"st_{v}"] += int((disp == v).sum())
        p["st_pass"] += int((disp < 127).all(axis=1).sum())
        p["st_gated"] += int((disp >= 127).any(axis=1).sum())
    return p
