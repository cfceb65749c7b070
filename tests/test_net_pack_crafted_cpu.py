"""CPU: the crafted KeyLine lists of tests/net_pack_crafted.py through the reference's own packer (src/CommLib/net_keypoint.cpp, compiled
into the reference oracle) and through the host packer rebvo_copy_net_keyline(+_nextid): byte for byte the same records.  That proves
the crafted inputs lie where the reference is defined, and makes the host packer the yardstick tests/test_net_pack_gpu.py holds the
device packer to.  The branch populations are asserted, so that a change of the generator cannot empty a branch unnoticed."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import net_pack_crafted as crafted

# packed KeyLines per branch of the packer (tests/net_pack_crafted.populations), as the generator stands
POPULATIONS = {
    "cp_tie": 58, "rho_zero": 23, "rho_neg": 23, "rho_below_clamp": 20, "rho_above_clamp": 42, "rho_floor": 19,
    "m0": 14, "m255": 13, "m256": 13, "m_big": 13,
    "flow_neg": 53, "flow_zero": 17, "flow_over": 36, "flow_tie": 65,
    "nid_none": 36, "nid_in": 63, "nid_past": 3,
    "st_none": 19, "st_126": 45, "st_127": 18, "st_128": 22, "st_pass": 44, "st_gated": 39,
}


def test_every_branch_is_populated():
    lists = crafted.crafted_lists()
    assert [len(kl) for kl, _ in lists] == list(crafted.LENGTHS)
    assert (37 * 15) % 16 != 0                      # the 37-record tail ends inside a 16-byte word
    assert (crafted.KL_SIZE_ODD * 15) % 16 != 0     # ... and with the odd store size sequences start inside one
    pop = crafted.populations(lists)
    assert pop == POPULATIONS
    assert min(pop.values()) > 0


def test_host_packer_outputs_cover_the_clamps():
    """What the branches produce, on the host packer: both ends of every clamp, the floor, ties rounded away from zero."""
    if not os.path.exists(crafted.HOST):
        pytest.fail("librebvohost.so not built — run __graft_entry__.build()")
    kl, pair = crafted.crafted_lists()[3]
    rec, n = crafted.host_pack(kl, None, crafted.KL_SIZE, crafted.K_PROF[3], 0xA5)
    assert n == crafted.KL_SIZE and (rec[n:] == 0xA5).all()
    r = rec[:n].copy().view(crafted.edgehip.NET_KEYLINE_DTYPE).ravel()
    assert {1, 65535} <= set(r["rho"].tolist()) and {1, 65535} <= set(r["s_rho"].tolist())
    assert {0, 255} <= set(r["m_num"].tolist()) and {0, 127, 255} <= set(r["flow"].ravel().tolist())
    assert (r["qx"][0], r["qy"][0]) == (11, 21)          # (10.5, 20.5): half away from zero
    assert r["n_kl"][5] == -1 and r["n_kl"][11] == -1     # n_id >= kl_size: not packed in this call
    assert (r["n_kl"] >= 0).sum() > 30
    rec_s, _ = crafted.host_pack(kl, pair, crafted.KL_SIZE, crafted.K_PROF[3], 0xA5)
    fl = rec_s[:n, 13:15]
    assert {1, 253, 127} <= set(fl.ravel().tolist())      # -126 and +126 px pass the gate; 127 / 128 px do not
    assert np.array_equal(rec_s[:n, :13], rec[:n, :13])


@pytest.mark.parametrize("stereo", [False, True])
def test_reference_packer_equals_host_packer(stereo):
    from oracle import oracle
    if not oracle.available("ref") or not os.path.exists(crafted.HOST):
        pytest.skip("needs oracle/_ref and librebvohost.so")
    orc = oracle.Oracle("ref", oracle.euroc_params(crafted.W, crafted.H))
    L = orc.lib
    L.ref_copy_net_keyline.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double]
    L.ref_copy_net_keyline_nextid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    mask = np.full((crafted.H, crafted.W), -1, np.int32)
    try:
        for which, (kl, pair) in enumerate(crafted.crafted_lists()):
            if stereo and len(kl) == 0:
                continue   # nothing to pack, and no pair KeyLine to point at
            k = crafted.K_PROF[which]
            want, n_h = crafted.host_pack(kl, pair if stereo else None, crafted.KL_SIZE, k, 0xA5)
            orc.set_keylines(0, kl, mask, 0.01)    # a fresh list: every net_id is -1
            orc.set_keylines(1, pair, mask, 0.01)
            # one guard record in front: copy_net_keyline_nextid writes to[net_id] of a KeyLine it did not pack, net_id = -1
            buf = np.full((crafted.KL_SIZE + 1, 15), 0xA5, np.uint8)
            out = buf[1:]
            n_r = L.ref_copy_net_keyline(orc.ctx, 0, 1 if stereo else -1, out.ctypes.data, crafted.KL_SIZE, k)
            L.ref_copy_net_keyline_nextid(orc.ctx, 0, out.ctypes.data, crafted.KL_SIZE)
            assert n_r == n_h == min(len(kl), crafted.KL_SIZE)
            assert np.array_equal(out, want), (which, np.argwhere(out != want)[:5].tolist())
    finally:
        orc.close()
