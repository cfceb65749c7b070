"""GPU: the wire-format packer on the device (edgehip_net_pack, rebvo_amd/csrc/net_keyline.hip) against the host packer
rebvo_copy_net_keyline(+_nextid), byte for byte, records and headers.  tests/test_net_pack_crafted_cpu.py holds the host packer equal to
the reference's own on the same crafted lists.  Fails, not skips, when the library lacks the entry points."""
import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import net_pack_crafted as crafted

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
SENTINEL = 0xA5


def raw(records):
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1, 15)


def whole_store(eh):
    """Every byte of the record store, and the headers, through the device copy."""
    import torch
    rec = torch.empty((eh.nseq, eh.net_kl_size, 15), dtype=torch.uint8, device="cuda")
    hdr = torch.empty((eh.nseq, 12), dtype=torch.uint8, device="cuda")
    eh.net_keylines_into(rec, hdr)
    return rec.cpu().numpy(), hdr.cpu().numpy().view(edgehip.NET_HEADER_DTYPE).reshape(-1)


def crafted_context(kl_size, stereo):
    lists = crafted.crafted_lists()
    eh = edgehip.EdgeHip(edgehip.euroc_params(crafted.W, crafted.H, max_points=128, stereo_available=1 if stereo else 0),
                         nseq=len(lists), nslots=2)
    for s, (kl, pair) in enumerate(lists):
        eh.upload_keylines(s, 0, kl)
        eh.upload_keylines(s, 1, pair)
    eh.net_enable(kl_size)
    for s in range(eh.nseq):   # the sentinel behind which nothing may be written
        eh.upload_net_keylines(s, np.full((kl_size, 15), SENTINEL, np.uint8))
    return eh, lists


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("kl_size", [crafted.KL_SIZE, crafted.KL_SIZE_ODD])
def test_crafted_lists(kl_size, stereo):
    """kn = 0, 1, 37, 69 in one launch: an empty list, one record, a tail inside a 16-byte word, a truncated list.  With 67 records per
    sequence the sequences start inside a word as well (64 * 15 B is a whole number of words)."""
    eh, lists = crafted_context(kl_size, stereo)
    try:
        eh.net_pack(0, 1 if stereo else -1, crafted.K_PROF)
        store, hdr = whole_store(eh)
        for s, (kl, pair) in enumerate(lists):
            want, n = crafted.host_pack(kl, pair if stereo else None, kl_size, crafted.K_PROF[s], SENTINEL)
            assert n == min(len(kl), kl_size)
            assert np.array_equal(store[s], want), (s, np.argwhere(store[s] != want)[:5].tolist())   # the sentinel behind the records included
            rec, h = eh.net_keylines(s)
            assert h["kline_num"] == n and h["k"] == np.float32(crafted.K_PROF[s]) and h["km_num"] == 0
            assert hdr[s] == h and len(rec) == n and np.array_equal(raw(rec), want[:n])
        if stereo:
            fl = store[3][:, 13:15]
            assert {1, 253, 127} <= set(fl.ravel().tolist())
    finally:
        eh.close()


def _frames(w, h, n):
    return [f for f, _, _ in synth.billboard_sequence(w, h, n)]


def _run_frames(eh, frames, count):
    for k in range(count):
        eh.upload_rgb(eh.next_slot(), np.stack([frames[k + s] for s in range(eh.nseq)]))
        eh.process_frame(np.full(eh.nseq, 0.05 * k))


def _host_records(eh, s, slot, kl_size, k):
    kl, _ = eh.download_keylines(s, slot, want_mask=False)
    want, n = crafted.host_pack(kl, None, kl_size, k, SENTINEL)
    return kl, want, n


def test_pack_after_real_frames():
    """Four frames, then the OLD slot with k_prof = NULL: records equal the host packer's on download_keylines of that slot with the
    sequence's K; 6001 records per sequence truncate the lists, so n_id >= count occurs on real edges."""
    w, h, nseq, kl_size = 376, 240, 3, 6001
    frames = _frames(w, h, 4 + nseq)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
    try:
        eh.net_enable(kl_size)
        for s in range(nseq):
            eh.upload_net_keylines(s, np.full((kl_size, 15), SENTINEL, np.uint8))
        _run_frames(eh, frames, 4)
        old = (eh.cur_slot() - 1) % 3
        eh.net_pack(old)
        store, hdr = whole_store(eh)
        flows, links = 0, 0
        for s in range(nseq):
            st = eh.get_state(s)
            kl, want, n = _host_records(eh, s, old, kl_size, st.K)
            assert len(kl) > kl_size and n == kl_size
            assert np.array_equal(store[s], want), (s, np.argwhere(store[s] != want)[:5].tolist())
            assert (hdr[s]["kline_num"], hdr[s]["km_num"], hdr[s]["k"]) == (n, st.klm_num, np.float32(st.K))
            r = want.view(edgehip.NET_KEYLINE_DTYPE).ravel()
            flows += int((r["flow"] != 127).sum())
            links += int((r["n_kl"] >= 0).sum())
            assert ((kl["n_id"][:n] >= n) & (r["n_kl"] == -1)).sum() > 0
        assert flows > 100 and links > 3000
    finally:
        eh.close()


def test_repeat_and_device_copy():
    """A second pack of another slot into the same store gives that slot's records with no remnants of the first (beyond the bytes the
    shorter list does not cover, which no pack touches); the device copy equals the download."""
    w, h, nseq = 376, 240, 2
    frames = _frames(w, h, 3 + nseq)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
    try:
        kl_size = eh.cap
        eh.net_enable(kl_size)
        _run_frames(eh, frames, 3)
        cur, old = eh.cur_slot(), (eh.cur_slot() - 1) % 3
        eh.net_pack(old, k_prof=2.0)
        first = [eh.net_keylines(s) for s in range(nseq)]
        eh.net_pack(cur, k_prof=[1.0, 0.5])
        store, hdr = whole_store(eh)
        both = eh.net_keylines_batch(list(range(nseq)))
        for s in range(nseq):
            kl, want, n = _host_records(eh, s, cur, kl_size, (1.0, 0.5)[s])
            _, want_old, n_old = _host_records(eh, s, old, kl_size, 2.0)
            assert n == len(kl) and n_old == len(first[s][0]) and np.array_equal(raw(first[s][0]), want_old[:n_old])
            assert np.array_equal(store[s][:n], want[:n]) and hdr[s]["kline_num"] == n
            assert not np.array_equal(want[:min(n, n_old)], want_old[:min(n, n_old)])
            rec, h = both[s]
            assert h == hdr[s] and np.array_equal(raw(rec), store[s][:n])
            assert np.array_equal(raw(eh.net_keylines(s)[0]), store[s][:n])
    finally:
        eh.close()


def test_argument_and_state_errors():
    eh = edgehip.EdgeHip(edgehip.euroc_params(64, 48), nseq=2, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        assert lib.edgehip_net_pack(ctx, 0, -1, None) == ERR_STATE
        assert lib.edgehip_download_net_keylines(ctx, 0, None, None) == ERR_STATE
        assert lib.edgehip_upload_net_keylines(ctx, 0, None, 0) == ERR_STATE
        assert lib.edgehip_net_keylines_device(ctx, 0, 1, None, None) == ERR_STATE
        assert lib.edgehip_net_enable(ctx, -1) == ERR_ARG
        assert lib.edgehip_net_enable(ctx, 50001) == ERR_ARG
        assert lib.edgehip_net_pack(ctx, 0, -1, None) == ERR_STATE   # a refused enable leaves the store off
        eh.net_enable(10)
        for slot, pair in ((2, -1), (-1, -1), (0, 2), (0, 0)):
            assert lib.edgehip_net_pack(ctx, slot, pair, None) == ERR_ARG
        assert lib.edgehip_net_pack(ctx, 0, 1, None) == ERR_STATE    # a pair slot on a context without the stereo fields
        assert lib.edgehip_download_net_keylines(ctx, 2, None, None) == ERR_ARG
        assert lib.edgehip_upload_net_keylines(ctx, 0, None, 11) == ERR_ARG
        assert lib.edgehip_net_keylines_device(ctx, 1, 2, None, None) == ERR_ARG
        assert lib.edgehip_net_enable(None, 4) == ERR_ARG
        eh.net_pack(0)   # still usable: empty slots pack to empty stores
        rec, h = eh.net_keylines(1)
        assert len(rec) == 0 and (h["kline_num"], h["km_num"], h["k"]) == (0, 0, 1.0)
        eh.net_enable(0)
        assert lib.edgehip_net_pack(ctx, 0, -1, None) == ERR_STATE
    finally:
        eh.close()
