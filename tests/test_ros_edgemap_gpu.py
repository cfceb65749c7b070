"""GPU: the ROS nodelet's per-KeyLine output packed on the device (edgehip_ros_pack / edgehip_ros_export, rebvo_amd/csrc/ros_edgemap.hip)
against the host packer rebvo_pack_ros_edgemap, byte for byte (a NaN equals a NaN at the same position).
tests/test_ros_edgemap_cpu.py holds the host packer equal to the reference's own arithmetic on the same crafted lists.  Fails, not
skips, when the library lacks the entry points."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import ros_edgemap_crafted as crafted

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
SENTINEL = 0xA5
W, H = crafted.W, crafted.H


def whole_stores(eh, what):
    """Every byte of the enabled stores, and the counts, through the device copy."""
    import torch
    pts = torch.empty((eh.nseq, eh.cap, 12), dtype=torch.uint8, device="cuda") if what & 1 else None
    recs = torch.empty((eh.nseq, eh.cap, 52), dtype=torch.uint8, device="cuda") if what & 2 else None
    kn = torch.empty((eh.nseq,), dtype=torch.int32, device="cuda")
    eh.ros_edgemap_into(pts, recs, kn)
    return (None if pts is None else pts.cpu().numpy()), (None if recs is None else recs.cpu().numpy()), kn.cpu().numpy()


def fill_sentinel(eh, what):
    import torch
    pts = torch.full((eh.nseq, eh.cap, 12), SENTINEL, dtype=torch.uint8, device="cuda") if what & 1 else None
    recs = torch.full((eh.nseq, eh.cap, 52), SENTINEL, dtype=torch.uint8, device="cuda") if what & 2 else None
    eh.ros_edgemap_from(pts, recs)


def check_against_host(got_p, got_k, kl, K, zfm, tag):
    want_p, want_k = crafted.host_pack(kl, K, zfm)
    if got_p is not None:
        g = np.ascontiguousarray(got_p).view(np.uint8).reshape(-1, 12)
        assert crafted.same_points(g, want_p), (tag, np.argwhere(g != want_p)[:5].tolist())
    if got_k is not None:
        g = np.ascontiguousarray(got_k).view(np.uint8).reshape(-1, 52)
        assert crafted.same_records(g, want_k), (tag, np.argwhere(g != want_k)[:5].tolist())


@pytest.mark.parametrize("what", [1, 2, 3])
# 601: strides of 7212 B and 31252 B (12 and 4 past a word) and a list of three workgroups, whose neighbours share a 16-byte word
@pytest.mark.parametrize("max_points", list(crafted.MAX_POINTS) + [601])
def test_crafted_lists(max_points, what):
    """kn = 0, 1, 37, max_points in one launch, a K per list.  With 67 records per sequence the strides are 804 B and 3484 B: sequences
    start inside a 16-byte word; with 128 they are word-aligned.  The whole store equals the host packer's bytes, the sentinel behind
    every list intact."""
    lists = crafted.crafted_lists(max_points)
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=max_points), nseq=len(lists), nslots=2)
    try:
        assert eh.cap == max_points
        for s, kl in enumerate(lists):
            eh.upload_keylines(s, 0, kl)
        eh.ros_enable(what)
        zero_p, zero_k, zero_n = whole_stores(eh, what)                        # the stores come zeroed
        assert all(a is None or not a.any() for a in (zero_p, zero_k, zero_n))
        fill_sentinel(eh, what)
        eh.ros_pack(0, crafted.K_PROF)
        pts, recs, kn = whole_stores(eh, what)
        assert kn.tolist() == [len(k) for k in lists]
        both = eh.ros_edgemaps_batch(list(range(eh.nseq)))
        for s, kl in enumerate(lists):
            n = len(kl)
            check_against_host(None if pts is None else pts[s][:n], None if recs is None else recs[s][:n], kl, crafted.K_PROF[s],
                               crafted.ZFM, (s, "store"))
            for a in (pts, recs):
                assert a is None or (a[s][n:] == SENTINEL).all(), (s, "sentinel")
            p1, k1, n1 = eh.ros_edgemap(s)
            assert n1 == n == both[s][2]
            for got, store in ((p1, pts), (k1, recs), (both[s][0], pts), (both[s][1], recs)):
                assert (got is None) == (store is None)
                assert got is None or (len(got) == n and got.tobytes() == store[s][:n].tobytes())
        if what & 1:
            f = pts[3].view(np.float32)
            assert np.isnan(f).any() and np.isinf(f).any() and ((f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)).any()
    finally:
        eh.close()


def _frames(n):
    return [f for f, _, _ in synth.billboard_sequence(W, H, n)]


def _run_frames(eh, frames, first, count):
    for k in range(first, first + count):
        eh.upload_rgb(eh.next_slot(), np.stack([frames[k + s] for s in range(eh.nseq)]))
        eh.process_frame(np.full(eh.nseq, 0.05 * k))


def test_pack_after_real_frames():
    """Three frames, then the current and the OLD slot (whose turned p_m / m_m / rho / s_rho the frame driver keeps beside it), with
    k_prof = None (each sequence's K) and an explicit array: the records equal the host packer's on download_keylines of that slot."""
    nseq = 3
    frames = _frames(3 + nseq)
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=nseq, nslots=3)
    try:
        eh.ros_enable(3)
        _run_frames(eh, frames, 0, 3)
        zfm = crafted.zfm_of(eh.p)
        cur, old = eh.cur_slot(), (eh.cur_slot() - 1) % 3
        for slot, k_prof in ((old, None), (cur, [1.5, 0.25, 3.0]), (old, [2.0, 1.0, 0.5]), (cur, None)):
            eh.ros_pack(slot, k_prof)
            got = eh.ros_edgemaps_batch(list(range(nseq)))
            for s in range(nseq):
                K = eh.get_state(s).K if k_prof is None else k_prof[s]
                kl, _ = eh.download_keylines(s, slot, want_mask=False)
                assert len(kl) > 1000 and got[s][2] == len(kl)
                check_against_host(got[s][0], got[s][1], kl, K, zfm, (slot, s))
        # the two slots differ, so a pack of the wrong one would have shown
        a = eh.download_keylines(0, cur, want_mask=False)[0]
        b = eh.download_keylines(0, old, want_mask=False)[0]
        assert a.tobytes() != b.tobytes()
    finally:
        eh.close()


def test_export_ring_with_four_frames_in_flight():
    """edgehip_ros_export / _fetch / _wait: the old slot's products packed behind frame k without a synchronisation, fetched only after
    frames k+1 .. k+3 have been enqueued (four tickets outstanding; the slot has been detected into again long since).  Equal to the host
    packer on what edgehip_download_keylines returned for that slot right behind frame k (a second context in lock-step provides that),
    with the K handed over at export time."""
    n_obj, n_fr = 4, 8
    frames = _frames(n_fr + n_obj)
    p = edgehip.euroc_params(W, H)
    eh, ref = edgehip.EdgeHip(p, nseq=n_obj, nslots=3), edgehip.EdgeHip(p, nseq=n_obj, nslots=3)
    zfm = crafted.zfm_of(p)
    seqs = [3, 0, 2]
    want, tickets, got, ks = {}, {}, {}, {}
    try:
        t = C.c_int(0)
        arr, kk = np.array(seqs, np.int32), np.ones(3)
        argv = (3, arr.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p))
        assert eh.lib.edgehip_ros_export(eh.ctx, *argv, 3, C.byref(t)) == ERR_STATE      # no frame pair yet

        def collect(k):
            kns = [len(x) for x in want[k]]
            f = eh.ros_export_fetch(tickets.pop(k), kns, registered=(k % 2 == 0))         # page-locked and pageable destinations alike
            got[k] = eh.ros_export_wait(f)
        for k in range(n_fr):
            for e in (eh, ref):
                _run_frames(e, frames, k, 1)
            if k >= 1:
                ks[k] = [1.0 + 0.25 * k + 0.5 * j for j in range(len(seqs))]
                tickets[k] = eh.ros_export(seqs, ks[k], 1 + ((k + 1) % 3))                # both, points, records in turn
                want[k] = [ref.download_keylines(s_, (ref.cur_slot() + 2) % 3, want_mask=False)[0] for s_ in seqs]
            if len(tickets) == 4:
                assert eh.lib.edgehip_ros_export(eh.ctx, *argv, 3, C.byref(t)) == ERR_STATE   # a fifth ticket is refused
                collect(min(tickets))
        for k in sorted(tickets):
            collect(k)
        assert sorted(got) == list(range(1, n_fr))
        for k in got:
            what = 1 + ((k + 1) % 3)
            for j, (pts, recs) in enumerate(got[k]):
                assert (pts is not None) == bool(what & 1) and (recs is not None) == bool(what & 2)
                assert len(want[k][j]) > 1000
                check_against_host(pts, recs, want[k][j], ks[k][j], zfm, (k, j))
        # a ticket released unfetched frees its entry only behind its pack: exports with OTHER sequences into the same entries are right
        held = [eh.ros_export(seqs, [1.0, 1.0, 1.0], 3) for _ in range(4)]
        assert eh.lib.edgehip_ros_export(eh.ctx, *argv, 3, C.byref(t)) == ERR_STATE
        for h in held:
            eh.ros_export_wait(h)
        old = (ref.cur_slot() + 2) % 3
        for other in ([1, 2, 0], [2, 1], [0], [1, 3, 2]):
            tk = eh.ros_export(other, [2.0] * len(other), 3)
            lists = [ref.download_keylines(s_, old, want_mask=False)[0] for s_ in other]
            out = eh.ros_export_wait(eh.ros_export_fetch(tk, [len(x) for x in lists], registered=False))
            for j, (pts, recs) in enumerate(out):
                check_against_host(pts, recs, lists[j], 2.0, zfm, ("other", other, j))
        assert eh.lib.edgehip_ros_export_wait(eh.ctx, 123456) == ERR_ARG
    finally:
        eh.close()
        ref.close()


def test_argument_and_state_errors():
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H), nseq=2, nslots=3)
    lib, ctx = eh.lib, eh.ctx
    try:
        t = C.c_int(0)
        seqs, ks, kn = np.array([0, 1], np.int32), np.ones(2), np.zeros(2, np.int32)
        ps, pk = seqs.ctypes.data_as(C.c_void_p), ks.ctypes.data_as(C.c_void_p)
        assert lib.edgehip_ros_pack(ctx, 0, None) == ERR_STATE
        assert lib.edgehip_download_ros_edgemap(ctx, 0, None, None, None) == ERR_STATE
        assert lib.edgehip_download_ros_edgemaps_batch(ctx, 2, ps, None, None, None) == ERR_STATE
        assert lib.edgehip_ros_edgemap_device(ctx, 0, 1, None, None, None) == ERR_STATE
        assert lib.edgehip_ros_edgemap_from_device(ctx, 0, 1, None, None) == ERR_STATE
        for bad in (4, 7, -1):
            assert lib.edgehip_ros_enable(ctx, bad) == ERR_ARG
        assert lib.edgehip_ros_pack(ctx, 0, None) == ERR_STATE                          # a refused enable leaves the stores off
        assert lib.edgehip_ros_enable(None, 1) == ERR_ARG
        eh.ros_enable(1)
        for slot in (3, -1):
            assert lib.edgehip_ros_pack(ctx, slot, None) == ERR_ARG
        assert lib.edgehip_download_ros_edgemap(ctx, 2, None, None, None) == ERR_ARG
        assert lib.edgehip_download_ros_edgemaps_batch(ctx, 0, ps, None, None, None) == ERR_ARG
        assert lib.edgehip_download_ros_edgemaps_batch(ctx, 2, None, None, None, None) == ERR_ARG
        assert lib.edgehip_ros_edgemap_device(ctx, 1, 2, None, None, None) == ERR_ARG
        assert lib.edgehip_ros_edgemap_device(ctx, 0, 1, None, C.c_void_p(16), None) == ERR_STATE   # the records' store is off
        assert lib.edgehip_ros_edgemap_from_device(ctx, 0, 3, None, None) == ERR_ARG
        # the export: arguments first, then the state
        assert lib.edgehip_ros_export(ctx, 0, ps, pk, 1, C.byref(t)) == ERR_ARG
        assert lib.edgehip_ros_export(ctx, 2, None, pk, 1, C.byref(t)) == ERR_ARG
        assert lib.edgehip_ros_export(ctx, 2, ps, None, 1, C.byref(t)) == ERR_ARG      # k_prof is required
        assert lib.edgehip_ros_export(ctx, 2, ps, pk, 0, C.byref(t)) == ERR_ARG
        assert lib.edgehip_ros_export(ctx, 2, ps, pk, 4, C.byref(t)) == ERR_ARG
        assert lib.edgehip_ros_export(ctx, 2, ps, pk, 1, None) == ERR_ARG
        bad = np.array([0, 2], np.int32)
        assert lib.edgehip_ros_export(ctx, 2, bad.ctypes.data_as(C.c_void_p), pk, 1, C.byref(t)) == ERR_ARG
        assert lib.edgehip_ros_export(ctx, 2, ps, pk, 1, C.byref(t)) == ERR_STATE      # no frame pair yet
        assert lib.edgehip_ros_export_fetch(ctx, 0, kn.ctypes.data_as(C.c_void_p), None, None) == ERR_ARG   # no such ticket
        assert lib.edgehip_ros_export_wait(ctx, 0) == ERR_ARG
        eh.ros_pack(0)                                                                  # still usable: empty slots pack to empty stores
        assert eh.ros_edgemap(1)[2] == 0
        eh.ros_enable(0)
        assert lib.edgehip_ros_pack(ctx, 0, None) == ERR_STATE
        # ... and the context still processes frames
        frames = _frames(3)
        for k in range(3):
            eh.upload_rgb(eh.next_slot(), np.stack([frames[k], frames[k]]))
            eh.process_frame(np.full(2, 0.05 * k))
        assert eh.read_nav()[0].kn > 1000
        tk = eh.ros_export([1, 0], [1.0, 1.0], 2)                                       # the export needs no edgehip_ros_enable
        kns = np.array([99999, 0], np.int32)
        assert lib.edgehip_ros_export_fetch(ctx, tk[0], kns.ctypes.data_as(C.c_void_p), None, None) == ERR_ARG   # beyond the capacity
        f = eh.ros_export_fetch(tk, [0, 0])
        assert lib.edgehip_ros_export_fetch(ctx, tk[0], kn.ctypes.data_as(C.c_void_p), None, None) == ERR_STATE  # fetched already
        eh.ros_export_wait(f)
        assert lib.edgehip_ros_pack(ctx, 0, None) == ERR_STATE
    finally:
        eh.close()


# ---- the mirror library: &EdgeMapOutput through the output callbacks of a batch group (rebvo_amd/host/examples/ros_output_replay.cpp) ----
REPLAY = os.path.join(crafted.ROOT, "rebvo_amd", "lib", "ros_output_replay")


def _replay(tmp_path, frames, n_obj, n_fr, tag, section):
    from tests.helpers import write_global_config
    from tests.test_batch_group_gpu import T0, DT
    if not os.path.exists(REPLAY):
        pytest.fail("ros_output_replay not built — a broken snapshot: run __graft_entry__.build()")
    np.stack(frames).tofile(tmp_path / "frames.rgb24")
    cfg = tmp_path / f"cfg_{tag}"
    write_global_config(cfg, edgehip.euroc_params(W, H))
    with open(cfg, "a") as f:
        f.write(section)
    prefix = tmp_path / tag
    r = subprocess.run([REPLAY, str(cfg), str(tmp_path / "frames.rgb24"), str(len(frames)), str(n_obj), str(n_fr), str(T0), str(DT),
                        "--dump", str(prefix)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    js = json.loads(r.stdout.strip().splitlines()[-1])
    out = []
    for i in range(n_obj):
        raw, at, calls = open(f"{prefix}.{i}.ros", "rb").read(), 0, []
        while at < len(raw):
            p_id, kn, npts, nrec = np.frombuffer(raw, np.int32, 4, at)
            nav = np.frombuffer(raw, np.float64, 10, at + 16)
            at += 96
            pts = recs = None
            if npts >= 0:
                pts = np.frombuffer(raw, np.uint8, 12 * npts, at).reshape(npts, 12)
                at += 12 * npts
            if nrec >= 0:
                recs = np.frombuffer(raw, np.uint8, 52 * nrec, at).reshape(nrec, 52)
                at += 52 * nrec
            calls.append((int(p_id), int(kn), nav.copy(), pts, recs))
        out.append(calls)
    return js, out


SETTINGS = {   # tag: (section, cloud, records, list)
    "cloud_nolist": ("\n&EdgeMapOutput\nPointCloud=1\nKeyLineList=0\n", True, False, False),
    "msg_list": ("\n&EdgeMapOutput\nKeylineMsg=1\nKeyLineList=1\n", False, True, True),
    "both_list": ("\n&EdgeMapOutput\nPointCloud=1\nKeylineMsg=1\n", True, True, True),
}


def test_group_callbacks_get_the_cloud_and_the_records(tmp_path):
    """4 objects in one group, 4 frames, three settings of &EdgeMapOutput: every callback's cloud and records equal the host packer on
    the same object's KeyLines from a ctypes batch run (K = 1, what the group's buffers carry); with KeyLineList = 0 the callback's list is
    empty and the nav records are bit-identical to the runs with it on."""
    from tests.test_batch_group_gpu import _ctypes_batch
    n_obj, n_fr, pool = 4, 4, 6
    frames = [f for f, _, _ in synth.billboard_sequence(W, H, pool)]
    navs, kls = _ctypes_batch(frames, n_obj, n_fr)
    zfm = crafted.zfm_of(edgehip.euroc_params(W, H))
    runs = {}
    for tag, (section, cloud, msg, lst) in SETTINGS.items():
        js, out = _replay(tmp_path, frames, n_obj, n_fr, tag, section)
        assert (js["point_cloud"], js["keyline_msg"], js["keyline_list"]) == (int(cloud), int(msg), int(lst))
        assert js["callbacks"] == n_obj * (n_fr - 1), js
        runs[tag] = out
        for i in range(n_obj):
            assert len(out[i]) == n_fr - 1
            for j, (p_id, kn, nav, pts, recs) in enumerate(out[i]):
                kl = kls[j][i]                       # frame j's slot after frame j + 1 went over it
                assert p_id == j and len(kl) > 1000 and nav[0] == 1.0
                assert kn == (len(kl) if lst else 0)
                assert (pts is not None) == cloud and (recs is not None) == msg
                assert pts is None or len(pts) == len(kl)
                assert recs is None or len(recs) == len(kl)
                check_against_host(pts, recs, kl, 1.0, zfm, (tag, i, j))
                if j > 0:
                    pos, lie, vel = navs[j][i][:3]
                    assert np.array_equal(nav[1:4], pos) and np.array_equal(nav[4:7], lie) and np.array_equal(nav[7:10], vel)
    for i in range(n_obj):
        for a, b in zip(runs["cloud_nolist"][i], runs["both_list"][i]):
            assert a[2].tobytes() == b[2].tobytes()                       # nav records: bit-identical without the list
            assert a[3].tobytes() == b[3].tobytes()


def test_group_refuses_members_with_other_edge_map_output_keys(tmp_path):
    from tests.helpers import write_global_config
    cfg = tmp_path / "cfg"
    write_global_config(cfg, edgehip.euroc_params(W, H))
    host = C.CDLL(crafted.HOST)
    assert host.rebvo_group_edgemap_selftest(str(cfg).encode()) == 0
