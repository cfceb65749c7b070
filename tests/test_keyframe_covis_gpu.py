"""Key-frame pair scoring on the device (edgehip_keyframe_covisibility, edgehip_keyframe_covisibility_slot) against the reference's
recorded counts (tests/golden/keyframe_covis/): every edgehip_kf_pair_count of every pair equals the fixture's, no tolerance and no
excluded pair.  Key frames are seeded with upload_keyframe (each upload retires the one before into the list); the lists are ragged
across the sequences of a batch."""
import ctypes as C
import os

import numpy as np
import pytest

import keyframe_covis_port as port
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_covis")
_FX = {}


def fixture(name):
    if name not in _FX:
        f = port.load_fixture(os.path.join(GOLD, name + ".npz"))
        f["rec"] = [port.records(k, edgehip.KEYLINE_DTYPE) for k in f["kfs"]]
        f["pose"] = [edgehip.EdgeHip.kf_pose(k["Pose"], k["Pos"], t=0.1 * m, K=float(k["K"])) for m, k in enumerate(f["kfs"])]
        _FX[name] = f
    return _FX[name]


def context(f, nseq, capacity, max_points=None, track=True):
    cam = f["cam"]
    mp = max_points or max(len(r) for r in f["rec"]) + 3
    p = edgehip.euroc_params(int(cam["w"]), int(cam["h"]), ppx=float(cam["ppx"]), ppy=float(cam["ppy"]), zfx=float(cam["zfx"]),
                             zfy=float(cam["zfy"]), max_points=mp)
    eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2, device=0)
    if track:
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        if capacity:
            eh.keyframe_list_enable(capacity)
    return eh


def args_of(f, **over):
    a = {k: f["args"][k].item() for k in f["args"]}
    a.update(over)
    return a


def seed(eh, f, orders):
    """orders[seq]: the fixture's key frames in the order the sequence takes them."""
    for s, order in enumerate(orders):
        for m in order:
            eh.upload_keyframe(s, f["rec"][m], f["pose"][m])


def positions(orders, capacity):
    """What each sequence holds afterwards: the last capacity + 1 it took, oldest first."""
    return [list(o[-(capacity + 1):]) for o in orders]


def expected(pos, M, counts4):
    """[nseq][M][M][4] from counts4[to][from] of the fixture's (or the port's) key frames; -1 for positions a sequence lacks."""
    out = np.full((len(pos), M, M, 4), -1, np.int32)
    for s, p in enumerate(pos):
        for i, a in enumerate(p):
            for j, b in enumerate(p):
                out[s, i, j] = counts4[a, b]
    return out


def as4(counts):
    return np.stack([counts[n] for n in ("kl_on_fov", "kl_match", "kls_on_fov", "guard")], -1)


def with_guard(counts3):
    return np.concatenate([counts3, np.zeros(counts3.shape[:-1] + (1,), counts3.dtype)], -1)


def snapshot(eh):
    """Every key frame, list entry and ring slot, as bytes."""
    info = eh.keyframe_list_info()
    out = [info.tobytes()]
    for s in range(eh.nseq):
        kl, pose, count = eh.download_keyframe(s)
        out += [kl.tobytes(), bytes(pose), count]
        for j in range(info["first"][s], info["first"][s] + info["held"][s]):
            e = eh.download_keyframe_list(s, int(j))
            out += [e[0].tobytes(), bytes(e[1])]
        for slot in range(2):
            kl, mask = eh.download_keylines(s, slot)
            out += [kl.tobytes(), mask.tobytes()]
    return out


ORDERS = [[0, 1, 2, 3, 4], [], [4], [1, 2, 3], [4, 3, 2, 1, 0], [3, 3], [2, 4, 0, 1]]


@pytest.mark.parametrize("name,nseq", [("crafted", 7), ("chained", 3)])
def test_every_pair_equals_the_reference(name, nseq):
    """Capacity 4: a full list (5 uploads), no key frame, the current one alone, partial lists, the same key frame twice."""
    f = fixture(name)
    eh = context(f, nseq, 4)
    try:
        orders = ORDERS[:nseq]
        seed(eh, f, orders)
        before = snapshot(eh)
        got, info = eh.keyframe_covisibility(**args_of(f))
        assert got.shape == (nseq, 5, 5)
        pos = positions(orders, 4)
        assert np.array_equal(as4(got), expected(pos, 5, with_guard(f["counts"])))
        assert np.array_equal(info, eh.keyframe_list_info())
        assert [int(x) for x in info["held"]] == [max(len(o) - 1, 0) for o in orders]
        assert snapshot(eh) == before
        # a second call gives the same
        again, _ = eh.keyframe_covisibility(**args_of(f))
        assert np.array_equal(again, got)
    finally:
        eh.close()


def test_wrapped_ring_min_mod_and_slot_form():
    """Capacity 2 with 5 uploads: first > 0, the ring has wrapped.  The min_mod field.  The query form against the all-pairs form."""
    f = fixture("crafted")
    eh = context(f, 3, 2)
    try:
        orders = [[0, 1, 2, 3, 4], [3, 4, 0, 4, 2], [4]]
        seed(eh, f, orders)
        pos = positions(orders, 2)
        got, info = eh.keyframe_covisibility(**args_of(f))
        assert list(info["first"]) == [2, 2, 0] and list(info["held"]) == [2, 2, 0] and list(info["overwritten"]) == [2, 2, 0]
        assert np.array_equal(as4(got), expected(pos, 3, with_guard(f["counts"])))
        z = f["z"]
        got_b, _ = eh.keyframe_covisibility(**args_of(f, field_min_mod=float(z["min_mod_b"])))
        assert np.array_equal(as4(got_b), expected(pos, 3, with_guard(z["counts_b"])))
        assert not np.array_equal(got_b, got)
        # the query form: slot 1 holds key frame 4's KeyLines with its pose in every sequence
        for s in range(3):
            eh.upload_keylines(s, 1, f["rec"][4])
        before = snapshot(eh)
        q, qinfo = eh.keyframe_covisibility_slot(1, poses=[f["pose"][4]] * 3, **args_of(f))
        assert q.shape == (3, 3) and np.array_equal(qinfo, info)
        assert snapshot(eh) == before
        want = np.full((3, 3, 4), -1, np.int32)
        for s, p in enumerate(pos):
            for i, a in enumerate(p):
                want[s, i] = with_guard(f["counts"])[a, 4]
        assert np.array_equal(as4(q), want)
        for s, p in enumerate(pos):                      # sequence s holds key frame 4 at position p.index(4): the same column
            assert np.array_equal(q[s], got[s, :, p.index(4)]), s
    finally:
        eh.close()


def test_chained_slot_form_nseq_7():
    f = fixture("chained")
    eh = context(f, 7, 1)
    try:
        orders = [[0, 1], [1, 2], [2, 3], [3, 4], [4], [], [4, 0]]
        seed(eh, f, orders)
        for s in range(7):
            eh.upload_keylines(s, 0, f["rec"][2])
        q, _ = eh.keyframe_covisibility_slot(0, poses=[f["pose"][2]] * 7, **args_of(f))
        want = np.full((7, 2, 4), -1, np.int32)
        for s, p in enumerate(positions(orders, 1)):
            for i, a in enumerate(p):
                want[s, i] = with_guard(f["counts"])[a, 2]
        assert np.array_equal(as4(q), want)
    finally:
        eh.close()


def test_non_finite_rho_is_counted_and_forms_no_address():
    """The reference cannot run this input (it indexes its field with the result): the port alone is the yardstick."""
    f = fixture("crafted")
    kfs = [dict(k) for k in f["kfs"]]
    kfs[3]["rho"] = kfs[3]["rho"].copy()
    kfs[3]["rho"][[5, 200]] = np.nan
    a = args_of(f)
    want = port.covisibility(kfs, f["cam"], a["field_radius"], a["match_mod"], a["match_ang"], a["rho_tol"], a["max_r"], a["field_min_mod"])
    assert (want[:, 3, 3] == 2).all() and not np.delete(want[..., 3], 3, axis=1).any()
    eh = context(f, 3, 4)
    try:
        orders = [[0, 1, 2, 3, 4], [3], []]
        for s, order in enumerate(orders):
            for m in order:
                eh.upload_keyframe(s, port.records(kfs[m], edgehip.KEYLINE_DTYPE), f["pose"][m])
        got, _ = eh.keyframe_covisibility(**a)
        assert np.array_equal(as4(got), expected(positions(orders, 4), 5, want))
        assert (got["guard"][0, :, 3] == 2).all() and got["guard"][1, 0, 0] == 2
    finally:
        eh.close()


def test_without_a_list_reset_and_resized_list():
    f = fixture("crafted")
    eh = context(f, 3, 0)
    try:
        seed(eh, f, [[3], [], [4]])
        got, info = eh.keyframe_covisibility(**args_of(f))      # M = 1: the current key frames alone
        assert got.shape == (3, 1, 1)
        c = with_guard(f["counts"])
        assert np.array_equal(as4(got)[:, 0, 0], [c[3, 3], [-1] * 4, c[4, 4]])
        assert list(info["kf_count"]) == [1, 0, 1] and list(info["held"]) == [0, 0, 0]
        eh.keyframe_list_enable(3)
        seed(eh, f, [[4], [2, 3], []])
        got, info = eh.keyframe_covisibility(**args_of(f))
        assert np.array_equal(as4(got), expected([[3, 4], [2, 3], [4]], 4, c))
        eh.reset()
        eh.keyframe_list_enable(1)
        got, info = eh.keyframe_covisibility(**args_of(f))
        assert (as4(got) == -1).all() and not info["kf_count"].any()
        seed(eh, f, [[1, 2, 3], [4], [0, 4]])
        got, info = eh.keyframe_covisibility(**args_of(f))
        assert np.array_equal(as4(got), expected([[2, 3], [4], [0, 4]], 2, c))
    finally:
        eh.close()


def test_error_returns():
    f = fixture("crafted")
    eh = context(f, 3, 0, track=False)
    try:
        a = edgehip.KfCovisArgs(5, 0.0, 0.5, 0.9, 1.5, 3.0)
        out = np.zeros((3, 1, 1), edgehip.KF_PAIR_COUNT_DTYPE)
        po = out.ctypes.data_as(C.c_void_p)
        lib = eh.lib
        assert lib.edgehip_keyframe_covisibility(eh.ctx, C.byref(a), po, None) == -4                 # EDGEHIP_ERR_STATE
        assert lib.edgehip_keyframe_covisibility_slot(eh.ctx, 0, None, C.byref(a), po, None) == -4
        eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
        assert lib.edgehip_keyframe_covisibility(eh.ctx, None, po, None) == -1                       # EDGEHIP_ERR_ARG
        assert lib.edgehip_keyframe_covisibility(eh.ctx, C.byref(a), None, None) == -1
        for radius in (0, -3, 4095):
            bad = edgehip.KfCovisArgs(radius, 0.0, 0.5, 0.9, 1.5, 3.0)
            assert lib.edgehip_keyframe_covisibility(eh.ctx, C.byref(bad), po, None) == -1, radius
        for slot in (-1, 2):
            assert lib.edgehip_keyframe_covisibility_slot(eh.ctx, slot, None, C.byref(a), po, None) == -1, slot
        with pytest.raises(edgehip.EdgeHipError):
            eh.keyframe_covisibility(0, 0.5, 0.9, 1.5, 3.0)
        assert lib.edgehip_keyframe_covisibility(eh.ctx, C.byref(a), po, None) == 0                  # the context stays usable
        assert (as4(out) == -1).all()
        big = edgehip.KfCovisArgs(4094, 0.0, 0.5, 0.9, 1.5, 3.0)                                    # the largest radius the key holds
        seed(eh, f, [[2], [], [1]])
        assert lib.edgehip_keyframe_covisibility(eh.ctx, C.byref(big), po, None) == 0
        assert out["kl_on_fov"][0, 0, 0] == f["counts"][2, 2, 0] and out["kls_on_fov"][0, 0, 0] == 65 and out["guard"][0, 0, 0] == 0
    finally:
        eh.close()
