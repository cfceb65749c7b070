"""GPU: the compressed edge map on the device (edgehip_edgemap_compress, rebvo_amd/csrc/edgemap_compress.hip) against the compiled
reference's records (tests/golden/edgemap/, for the crafted lists) and against the serial host restatement rebvo_compress_edgemap (which
tests/test_edgemap_cpu.py holds equal to the reference byte for byte).  Fails, not skips, when the library lacks the entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import edgemap_crafted as crafted

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4
W, H = crafted.W, crafted.H
CAP_RECORDS = 2 * crafted.MAX_POINTS + 1     # 641 records = 3205 B per sequence: sequences start inside a 16-byte word
BATCH = ["cut_twice", "kn_0", "merge_rewalk", "points_27", "scale", "mixed", "cycle_5", "kn_1", "identical", "xy_clamp"]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return crafted.build_host_tool(tmp_path_factory.mktemp("edgemap_gpu"))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(crafted.ROOT, "tests", "golden", "edgemap", "crafted.npz"))


@pytest.fixture(scope="module")
def one():
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=crafted.MAX_POINTS), nseq=1, nslots=2)
    eh.edgemap_enable(CAP_RECORDS)
    yield eh
    eh.close()


def as_bytes(rec):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 5)


def whole_store(eh):
    import torch
    rec = torch.empty((eh.nseq, eh.edgemap_cap, 5), dtype=torch.uint8, device="cuda")
    cnt = torch.empty((eh.nseq,), dtype=torch.int32, device="cuda")
    eh.edgemap_into(rec, cnt)
    return rec.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("name", crafted.names())
def test_crafted_list_alone(one, gold, name):
    kl, p = crafted.case(name)
    want = gold[f"{name}__records"].reshape(-1, 5)
    one.upload_keylines(0, 0, kl)
    one.edgemap_compress(0, crafted.params_struct(p), [p["scale"]])
    rec, status = one.download_edgemap(0)
    assert status == 0
    assert len(rec) == len(want), (name, len(rec), len(want))
    assert np.array_equal(as_bytes(rec), want), name


@pytest.mark.parametrize("nseq", [3, 7])
def test_ragged_batches_equal_the_runs_alone(gold, nseq):
    """crafted lists of different lengths side by side, a scale per sequence; twice, the second time with the lists dealt the other way
    round, so that shorter record lists land on longer ones: per sequence the records are the fixture's, and every byte of the store
    behind a sequence's records is what it was before the call."""
    names = BATCH[:nseq]
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=crafted.MAX_POINTS), nseq=nseq, nslots=2)
    try:
        eh.edgemap_enable(CAP_RECORDS)
        before, cnt = whole_store(eh)
        assert not before.any() and not cnt.any()                  # the store comes zeroed
        for order in (names, names[::-1]):
            scales = []
            for s, name in enumerate(order):
                kl, p = crafted.case(name)
                assert {k: p[k] for k in p if k != "scale"} == {k: crafted.DEFAULTS[k] for k in p if k != "scale"}
                scales.append(p["scale"])
                eh.upload_keylines(s, 0, kl)
            eh.edgemap_compress(0, crafted.params_struct(crafted.DEFAULTS), scales)
            store, cnt = whole_store(eh)
            got = eh.download_edgemaps(list(range(nseq)))
            for s, name in enumerate(order):
                want = gold[f"{name}__records"].reshape(-1, 5)
                assert cnt[s] == len(want) and got[s][1] == 0, (name, cnt[s])
                assert np.array_equal(store[s][:len(want)], want), name
                assert np.array_equal(as_bytes(got[s][0]), want), name
                assert np.array_equal(store[s][len(want):], before[s][len(want):]), (name, "bytes behind the records")
            before = store
        assert len({len(gold[f"{n}__records"]) for n in names}) >= 2
    finally:
        eh.close()


def test_billboard_frames_equal_host_restatement(tool):
    """upload_rgb + process_frame + edgemap_compress on the newest and on the old slot: the records equal rebvo_compress_edgemap run on
    the KeyLines edgehip_download_keylines returns for the same slot."""
    g = np.load(os.path.join(crafted.ROOT, "tests", "golden", "billboard_256x192.npz"))
    over = dict(eval(str(g["over"])))
    frames = g["frames"]
    params = edgehip.euroc_params(256, 192, **over)
    ppx, ppy, zfx, zfy = (np.float32(v) for v in (params.ppx, params.ppy, params.zfx, params.zfy))
    cam = (float(ppx), float(ppy), float(zfx), float(zfy), float((zfx + zfy) / np.float32(2)))
    p = dict(min_line_len=3, max_line_len=50, max_angle=0.3, match_n_t=1, rho_rel_max=2.0, scale=1.0)
    eh = edgehip.EdgeHip(params, nseq=2, nslots=3)
    try:
        eh.edgemap_enable(2 * eh.cap)
        fitted = 0
        for k in range(len(frames)):
            rgb = np.repeat(frames[k][:, :, None], 3, axis=2)
            eh.upload_rgb(eh.next_slot(), np.stack([rgb, rgb[:, ::-1].copy()]))
            eh.process_frame(np.full(2, 0.05 * k))
            if k not in (3, 5, 6):
                continue
            for slot, scales in ((eh.cur_slot(), [1.0, 1.3]), ((eh.cur_slot() - 1) % 3, [0.7, 1.0])):
                eh.edgemap_compress(slot, crafted.params_struct(p), scales)
                got = eh.download_edgemaps([0, 1])
                for s in range(2):
                    kl, _ = eh.download_keylines(s, slot, want_mask=False)
                    q = dict(p, scale=scales[s])
                    want = crafted.host_run(tool, kl, q, 2 * eh.cap, cam)
                    assert len(kl) > 1000 and want["count"] > 100 and want["status"] == 0
                    assert got[s][1] == 0 and len(got[s][0]) == want["count"], (k, slot, s, len(got[s][0]), want["count"])
                    assert np.array_equal(as_bytes(got[s][0]), want["records"]), (k, slot, s)
                    fitted += int((want["records"][:, 4] < 255).sum())
        assert fitted > 100                                         # not only degenerate fits
    finally:
        eh.close()


def _long_list(n):
    """n KeyLines in chains of 61 with a turn every 13, depths from a slow ramp: more than 16384 KeyLines take the component keys out of LDS"""
    parts, left, j = [], n, 0
    while left > 0:
        m = min(61, left)
        parts.append(crafted._run(m, 20 + (j * 7) % 600, 20 + (j * 13) % 300, 1.5, 0.5, rho=0.8 + 0.001 * (j % 50), turn_at=tuple(range(13, m, 13)), turn=0.5))
        left -= m
        j += 1
    kl = crafted._cat(*parts)
    kl["n_id"][60::61] = np.where(np.arange(len(kl["n_id"][60::61])) % 3 == 0, 5, -1)   # every third chain runs into chain 0
    return crafted._finish(kl)


@pytest.mark.parametrize("n", [16384, 16385, 17000])
def test_lists_around_the_lds_key_limit(tool, n):
    kl = _long_list(n)
    p = dict(crafted.DEFAULTS, max_line_len=50)
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=17000), nseq=1, nslots=2)
    try:
        eh.edgemap_enable(2 * 17000)
        eh.upload_keylines(0, 0, kl)
        eh.edgemap_compress(0, crafted.params_struct(p))
        rec, status = eh.download_edgemap(0)
        want = crafted.host_run(tool, kl, p, 2 * 17000)
        assert want["count"] > 1000 and status == want["status"] == 0
        assert len(rec) == want["count"] and np.array_equal(as_bytes(rec), want["records"])
        eh.profile_enable(True)                                     # the timed form: labelling and sort as two launches
        eh.edgemap_compress(0, crafted.params_struct(p))
        rec2, status2 = eh.download_edgemap(0)
        assert status2 == 0 and rec2.tobytes() == rec.tobytes() and len(eh.edgemap_ms()) == 4
    finally:
        eh.close()


def test_out_of_range_links_and_small_capacity(tool, gold):
    """a list with links outside [-1, kn) between two crafted lists: its status bit, its records equal to the host restatement's (the
    links read as -1), the neighbours exact; then a store too small for one sequence only; the context stays usable."""
    good_a, good_b = "mixed", "cut_middle"
    kl, p = crafted.case("merge_masked")
    bad = kl.copy()
    bad["n_id"][3], bad["n_id"][12], bad["p_id"][17], bad["p_id"][0] = len(kl), 2 ** 31 - 1, -2, len(kl) + 9
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=crafted.MAX_POINTS), nseq=3, nslots=2)
    try:
        eh.edgemap_enable(CAP_RECORDS)
        for s, k in enumerate((crafted.case(good_a)[0], bad, crafted.case(good_b)[0])):
            eh.upload_keylines(s, 0, k)
        eh.edgemap_compress(0, crafted.params_struct(p))
        got = eh.download_edgemaps([0, 1, 2])
        want = crafted.host_run(tool, bad, p, CAP_RECORDS)
        assert want["status"] == edgehip.EDGEMAP_BAD_LINK and want["count"] > 0
        assert got[1][1] == edgehip.EDGEMAP_BAD_LINK and np.array_equal(as_bytes(got[1][0]), want["records"])
        for s, name in ((0, good_a), (2, good_b)):
            assert got[s][1] == 0 and np.array_equal(as_bytes(got[s][0]), gold[f"{name}__records"].reshape(-1, 5)), name
        # room for cut_middle's 3 records and the bad list's, not for mixed's 9
        n_mixed = len(gold["mixed__records"].reshape(-1, 5))
        assert max(want["count"], 3) < n_mixed
        eh.edgemap_enable(n_mixed - 1)
        eh.edgemap_compress(0, crafted.params_struct(p))
        got = eh.download_edgemaps([0, 1, 2])
        assert got[0][1] == edgehip.EDGEMAP_OVERFLOW and len(got[0][0]) == 0
        assert got[1][1] == edgehip.EDGEMAP_BAD_LINK and np.array_equal(as_bytes(got[1][0]), want["records"])
        assert got[2][1] == 0 and np.array_equal(as_bytes(got[2][0]), gold[f"{good_b}__records"].reshape(-1, 5))
        # and the context goes on: the good list in place of the bad one
        eh.edgemap_enable(CAP_RECORDS)
        eh.upload_keylines(1, 0, kl)
        eh.edgemap_compress(0, crafted.params_struct(p))
        rec, status = eh.download_edgemap(1)
        assert status == 0 and np.array_equal(as_bytes(rec), gold["merge_masked__records"].reshape(-1, 5))
    finally:
        eh.close()


def test_frame_path_is_untouched():
    """two contexts over the same frames, one with the store enabled and a compression of both slots between the frames: nav records and
    KeyLines bit-identical (the feature only reads)."""
    frames = [f for f, _, _ in synth.billboard_sequence(376, 240, 5)]
    p = edgehip.euroc_params(376, 240)
    a, b = edgehip.EdgeHip(p, nseq=2, nslots=3), edgehip.EdgeHip(p, nseq=2, nslots=3)
    try:
        b.edgemap_enable(2 * b.cap)
        q = crafted.params_struct(dict(crafted.DEFAULTS, max_line_len=50))
        for k in range(4):
            for eh in (a, b):
                eh.upload_rgb(eh.next_slot(), np.stack([frames[k], frames[k + 1]]))
                eh.process_frame(np.full(2, 0.05 * k))
            if k:
                b.edgemap_compress(b.cur_slot(), q)
                b.edgemap_compress((b.cur_slot() - 1) % 3, q, [1.5, 0.5])
                assert all(len(r) > 50 and st == 0 for r, st in b.download_edgemaps([0, 1]))
            na, nb = a.read_nav(), b.read_nav()
            for s in range(2):
                assert bytes(na[s]) == bytes(nb[s]), (k, s)
        for s in range(2):
            for slot in range(3):
                assert a.download_keylines(s, slot, want_mask=False)[0].tobytes() == b.download_keylines(s, slot, want_mask=False)[0].tobytes()
    finally:
        a.close()
        b.close()


def test_error_returns():
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=crafted.MAX_POINTS), nseq=1, nslots=2)
    try:
        lib, ctx = eh.lib, eh.ctx
        ok = crafted.params_struct(crafted.DEFAULTS)
        ms = (C.c_float * 4)()
        cnt = C.c_int32(0)
        assert lib.edgehip_edgemap_compress(ctx, 0, C.byref(ok), None) == ERR_STATE        # not enabled
        assert lib.edgehip_download_edgemap(ctx, 0, None, C.byref(cnt), None) == ERR_STATE
        assert lib.edgehip_edgemap_device(ctx, 0, 1, None, None) == ERR_STATE
        assert lib.edgehip_edgemap_ms(ctx, ms) == ERR_STATE
        assert lib.edgehip_edgemap_enable(ctx, -1) == ERR_ARG
        assert lib.edgehip_edgemap_enable(ctx, 16) == 0
        eh.edgemap_cap = 16                                                                 # (what EdgeHip.edgemap_enable records)
        for over in (dict(min_line_len=-1), dict(max_line_len=0), dict(x_scaling=-0.5)):
            assert lib.edgehip_edgemap_compress(ctx, 0, C.byref(crafted.params_struct(dict(crafted.DEFAULTS, **over))), None) == ERR_ARG, over
        assert lib.edgehip_edgemap_compress(ctx, 2, C.byref(ok), None) == ERR_ARG           # slot out of range
        assert lib.edgehip_edgemap_compress(ctx, 0, None, None) == ERR_ARG
        assert lib.edgehip_download_edgemap(ctx, 1, None, C.byref(cnt), None) == ERR_ARG    # sequence out of range
        assert lib.edgehip_edgemap_compress(ctx, 0, C.byref(ok), None) == 0
        assert lib.edgehip_edgemap_ms(ctx, ms) == ERR_STATE                                 # not under edgehip_profile_enable
        eh.profile_enable(True)
        assert lib.edgehip_edgemap_compress(ctx, 0, C.byref(ok), None) == 0
        assert lib.edgehip_edgemap_ms(ctx, ms) == 0 and all(v >= 0 for v in ms)
        rec, status = eh.download_edgemap(0)                                                # (the timed form: labelling and sort as two launches)
        assert status == 0 and len(rec) == 0
        assert lib.edgehip_edgemap_enable(ctx, 0) == 0                                      # frees
        assert lib.edgehip_edgemap_compress(ctx, 0, C.byref(ok), None) == ERR_STATE
    finally:
        eh.close()
