"""CPU: the host packer of the ROS nodelet's per-KeyLine output (rebvo_pack_ros_edgemap, rebvo_amd/host/src/ros_edgemap.cpp) against the
reference's own arithmetic on the crafted lists (tests/golden/ros_edgemap/crafted.npz, written by tools/make_ros_edgemap_golden.py from
the reference's cam_model::unprojectHomCordVec and the message's C++ types), byte for byte; NaNs compare as "is NaN" at the same
positions.  tests/test_ros_edgemap_gpu.py holds the device packer equal to the host packer."""
import ctypes as C
import os

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import ros_edgemap_crafted as crafted

GOLD = os.path.join(crafted.ROOT, "tests", "golden", "ros_edgemap", "crafted.npz")


def test_record_sizes():
    assert edgehip.ROS_POINT_DTYPE.itemsize == 12 and edgehip.ROS_KEYLINE_DTYPE.itemsize == 52
    f = edgehip.ROS_KEYLINE_DTYPE.fields
    assert [f[n][1] for n in edgehip.ROS_KEYLINE_DTYPE.names] == [0, 8, 16, 24, 32, 40, 44, 48, 50]   # Keyline.msg order, no padding


def test_new_entry_points_are_exported():
    lib = edgehip.load_library()
    for name in edgehip.EXPORTS:
        if "_ros_" in name:
            assert hasattr(lib, name), name
    assert sum("_ros_" in n for n in edgehip.EXPORTS) == 9
    assert lib.edgehip_abi_version() == 2


def test_crafted_lists_match_the_fixture():
    """The generator still produces the lists the fixture was computed from, and they hold every corner case."""
    g = np.load(GOLD)
    lists = crafted.crafted_lists(128)
    assert [len(k) for k in lists] == [0, 1, 37, 128]
    assert float(g["zfm"]) == crafted.ZFM and tuple(g["K"]) == crafted.K_PROF
    for s, kl in enumerate(lists):
        assert np.array_equal(np.ascontiguousarray(kl).view(np.uint8).reshape(len(kl), 168), g[f"keylines_{s}"]), s
    short = crafted.crafted_lists(67)
    assert short[3].tobytes() == lists[3][:67].tobytes()
    p = crafted.populations(lists)
    assert all(v > 0 for v in p.values()), p


def test_host_packer_equals_reference_bytes():
    g = np.load(GOLD)
    for s in range(4):
        kl = g[f"keylines_{s}"].view(edgehip.KEYLINE_DTYPE).reshape(-1)
        pts, recs = crafted.host_pack(kl, g["K"][s], float(g["zfm"]))
        assert crafted.same_points(pts, g[f"points_{s}"]), (s, np.argwhere(pts != g[f"points_{s}"])[:5].tolist())
        assert crafted.same_records(recs, g[f"records_{s}"]), (s, np.argwhere(recs != g[f"records_{s}"])[:5].tolist())
    # what the comparison lets through is the NaNs alone: everything else is bit-equal
    pts, _ = crafted.host_pack(g["keylines_3"].view(edgehip.KEYLINE_DTYPE).reshape(-1), g["K"][3], float(g["zfm"]))
    f, w = pts.view(np.float32), g["points_3"].view(np.float32)
    assert np.isnan(f).sum() == np.isnan(w).sum() > 0 and np.isinf(f).sum() > 0
    assert ((f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)).sum() > 0          # float denormals are kept


def test_host_packer_fields_and_null_outputs():
    kl = crafted.crafted_lists(67)[2]
    pts, recs = crafted.host_pack(kl, 0.7, crafted.ZFM)
    r = recs.view(edgehip.ROS_KEYLINE_DTYPE).reshape(-1)
    assert np.array_equal(r["KlGrad"], kl["m_m"]) and np.array_equal(r["KlImgPos"], kl["c_p"]) and np.array_equal(r["KlFocPos"], kl["p_m"])
    assert np.array_equal(r["invDepth"].view(np.uint64), kl["rho"].view(np.uint64))            # rho is NOT divided by K
    assert np.array_equal(r["invDepthS"], kl["s_rho"])
    assert np.array_equal(r["KlMatchID"], kl["m_id"]) and np.array_equal(r["ConsMatch"], kl["m_num"])
    assert np.array_equal(r["KlPrevMatchID"], kl["p_id"].astype(np.uint32).astype(np.uint16).view(np.int16))   # the low 16 bits
    assert np.array_equal(r["KlNextMatchID"], kl["n_id"].astype(np.uint32).astype(np.uint16).view(np.int16))
    assert {-1, 0, 32767, -32768, 4464} <= set(r["KlPrevMatchID"].tolist())                   # 32768 -> -32768, 70000 -> 4464
    # either output may be null
    host = C.CDLL(crafted.HOST)
    host.rebvo_pack_ros_edgemap.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    host.rebvo_pack_ros_edgemap.restype = None
    k = np.ascontiguousarray(kl)
    p2, r2 = np.zeros_like(pts), np.zeros_like(recs)
    host.rebvo_pack_ros_edgemap(k.ctypes.data, len(k), 0.7, crafted.ZFM, p2.ctypes.data, None)
    host.rebvo_pack_ros_edgemap(k.ctypes.data, len(k), 0.7, crafted.ZFM, None, r2.ctypes.data)
    assert crafted.same_points(p2, pts) and np.array_equal(r2, recs)


def _parsed_keys(tmp_path, section):
    from tests.helpers import write_global_config
    cfg = tmp_path / "cfg"
    write_global_config(cfg, edgehip.euroc_params(376, 240))
    if section:
        with open(cfg, "a") as f:
            f.write(section)
    host = C.CDLL(crafted.HOST)
    out = (C.c_int * 3)(-1, -1, -1)
    assert host.rebvo_edgemap_output_config(str(cfg).encode(), out) == 0
    return list(out)


def test_config_parser_reads_the_three_edge_map_output_keys(tmp_path):
    """&EdgeMapOutput PointCloud / KeylineMsg / KeyLineList; an absent section, or absent keys, leave the products off and the list on."""
    assert _parsed_keys(tmp_path, "") == [0, 0, 1]
    assert _parsed_keys(tmp_path, "\n&EdgeMapOutput\nPointCloud=1\n") == [1, 0, 1]
    assert _parsed_keys(tmp_path, "\n&EdgeMapOutput\nKeylineMsg=1\nKeyLineList=0\n") == [0, 1, 0]
    assert _parsed_keys(tmp_path, "\n&EdgeMapOutput\nPointCloud=1\nKeylineMsg=1\nKeyLineList=1\n") == [1, 1, 1]


@pytest.mark.parametrize("rec", [12, 52])
def test_store_bookkeeping_of_the_kernel(rec):
    """k_ros_pack's cut of a store, restated (rebvo_amd/csrc/ros_edgemap.hip: 256 KeyLines per workgroup, LDS laid out from the offset
    b0 & 15, whole 16-byte words stored whole, the first and last word dword by dword): for aligned and misaligned strides, one and
    several workgroups, every byte of a list's kn records is written exactly once, from the right record, and no other byte."""
    lds_bytes = 16 + 256 * rec
    for stride in (1, 67, 128, 255, 257, 601):
        for count in (0, 1, 37, 67, 128, 256, 257, 601):
            if count > stride:
                continue
            for lst in (0, 1, 2, 3):
                lo, written = lst * stride * rec, {}
                for bx in range(max(1, (stride + 255) // 256)):
                    r0 = bx * 256
                    r1 = min(r0 + 256, count)
                    if r0 >= count:
                        continue
                    b0, b1 = lo + r0 * rec, lo + r1 * rec
                    w0 = b0 & ~15
                    assert (b0 & 15) + (r1 - r0) * rec <= lds_bytes
                    for t in range((b1 - w0 + 15) >> 4):
                        g = w0 + 16 * t
                        assert 16 * t + 16 <= lds_bytes
                        whole = g >= b0 and g + 16 <= b1
                        for d in range(0, 16, 4):
                            if whole or b0 <= g + d < b1:
                                for i in range(4):
                                    assert g + d + i not in written
                                    written[g + d + i] = divmod(16 * t + d + i - (b0 & 15), rec)   # LDS offset -> (record of the workgroup, byte)
                                    written[g + d + i] = (r0 + written[g + d + i][0], written[g + d + i][1])
                assert sorted(written) == list(range(lo, lo + count * rec)), (stride, count, lst)
                assert all(a == lo + r * rec + i for a, (r, i) in written.items())
