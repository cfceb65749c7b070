"""GPU: the dense depth fill (edgehip_depth_fill, rebvo_amd/csrc/depth_fill.hip) against the reference's own grids
(tests/golden/depth_fill/*.npz) and the numpy restatement (tests/depth_fill_port.py), bit for bit.  Fails, not skips, when the
library lacks the entry points."""
import os
import subprocess

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import depth_fill_port as port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(a, b):
    """Bit for bit, except that a NaN the arithmetic creates equals any NaN: the GPU's default NaN is positive, x86 SSE's negative."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_grid(got, want, what):
    rho, s_rho, fixed = got
    assert rho.shape == want[0].shape, what
    assert same_bits(rho, want[0]).all(), (what, "rho", int((~same_bits(rho, want[0])).sum()))
    assert same_bits(s_rho, want[1]).all(), (what, "s_rho", int((~same_bits(s_rho, want[1])).sum()))
    assert np.array_equal(fixed, np.asarray(want[2], bool)), (what, "fixed")


def to_records(fields):
    n = len(fields["rho"])
    kl = np.zeros(n, edgehip.KEYLINE_DTYPE)
    for f in port.FIELDS:
        kl[f] = fields[f]
    kl["m_id"] = -1
    return kl


@pytest.mark.parametrize("name", ["376x240", "752x480"])
def test_teacher_forced_golden(name):
    """The fixture lists through edgehip_upload_keylines, a different list per sequence of one context; every golden case's grid
    from the sequence that holds its list, the port's grid from the others."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "depth_fill", f"{name}.npz"))
    w, h = int(z["w"]), int(z["h"])
    names = sorted({k[2] for k in z.files if k.startswith("kl") and k.endswith("_rho")})
    lists = {n: {f: z[f"kl{n}_{f}"] for f in port.FIELDS} for n in names}
    seq_lists = [lists[n] for n in names]
    # one more list per file: the first one in reverse order (other cells fold other KeyLines first)
    seq_lists.append({f: v[::-1].copy() for f, v in lists[names[0]].items()})
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=len(seq_lists), nslots=2)
    try:
        for s, kl in enumerate(seq_lists):
            eh.upload_keylines(s, 1, to_records(kl))
        for i, (lst, bw, bh, it, mode, disc, m) in enumerate(z["cases"]):
            v = float(z[f"case{i}_thresh_rel_rho"])
            assert eh.depth_fill_enable(int(bw), int(it), v, int(m), int(mode), int(disc), block_h=int(bh)) == (w // bw, h // bh)
            eh.depth_fill(1)
            grids = eh.download_depth_grids(list(range(len(seq_lists))))
            for s, kl in enumerate(seq_lists):
                if s < len(names) and names[s] == chr(lst):
                    want = (z[f"case{i}_rho"], z[f"case{i}_s_rho"], z[f"case{i}_fixed"])
                else:
                    want = port.depth_fill(kl, w, h, int(bw), int(bh), int(it), v, int(m), int(mode), int(disc))
                assert_grid(grids[s], want, (name, i, s))
            assert_grid(eh.download_depth_grid(len(seq_lists) - 1), want, (name, i, "single"))
    finally:
        eh.close()


def _pool(w, h, n):
    import torch
    mono = np.stack([np.ascontiguousarray(f[:, :, 0]) for f, _, _ in synth.billboard_sequence(w, h, n)])
    t = torch.empty(mono.size + 16, dtype=torch.uint8, device="cuda")
    t[:mono.size] = torch.from_numpy(mono.reshape(-1)).cuda()
    return t, mono


@pytest.mark.parametrize("block", [10, 5])
def test_1024_sequences_after_every_frame(block):
    """1024 sequences at 752x480 through edgehip_process_frame, the fill after every frame (on the OLD slot, which holds the turned
    rho / s_rho beside its arrays, and on the newest slot); sequences 0, 511 and 1023 against the port on that slot's KeyLines."""
    w, h, nseq, frames = 752, 480, 1024, 4
    pool, _ = _pool(w, h, frames + 2)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
    try:
        eh.depth_fill_enable(block, 10, 1.0, 2, 0, 1)   # ThreshMatchNum 2: four frames give KeyLines matched twice
        for k in range(frames):
            idx = np.array([k + (s % 3) for s in range(nseq)], np.int32)
            eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), frames + 2, idx)
            eh.process_frame(np.full(nseq, 0.05 * k))
            cur = eh.cur_slot()
            slots = [cur] if k == 0 else [(cur - 1) % 3, cur]
            for slot in slots:
                eh.depth_fill(slot)
                grids = eh.download_depth_grids([0, 511, 1023])
                for j, s in enumerate((0, 511, 1023)):
                    kl, _ = eh.download_keylines(s, slot, want_mask=False)
                    assert_grid(grids[j], port.depth_fill(kl, w, h, block, block, 10, 1.0, 2, 0, 1), (k, slot, s))
            if k == frames - 1:
                assert grids[0][2].sum() > 50   # matched KeyLines reached the grid
    finally:
        eh.close()


def test_fill_is_read_only():
    """Nav records and KeyLine lists bit-identical with the fill on (after every frame, both slots) and off."""
    w, h, nseq, frames = 376, 240, 4, 6
    pool, _ = _pool(w, h, frames + 3)
    runs = []
    for fill in (True, False):
        eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
        try:
            if fill:
                eh.depth_fill_enable(5, 10, 1.0, 5, 2, 0)
            navs = []
            for k in range(frames):
                idx = np.array([k + s % 3 for s in range(nseq)], np.int32)
                eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), frames + 3, idx)
                eh.process_frame(np.full(nseq, 0.05 * k))
                if fill:
                    eh.depth_fill((eh.cur_slot() - 1) % 3)
                    eh.depth_fill(eh.cur_slot())
                navs.append(b"".join(bytes(n) for n in eh.read_nav()))
            kls = [eh.download_keylines(s, slot)[0].tobytes() for s in range(nseq) for slot in range(3)]
            runs.append((navs, kls))
        finally:
            eh.close()
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1]


def test_argument_and_state_errors():
    import ctypes as C
    eh = edgehip.EdgeHip(edgehip.euroc_params(64, 48), nseq=2, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        gw, gh = C.c_int32(0), C.c_int32(0)
        assert lib.edgehip_depth_fill(ctx, 0) == ERR_STATE
        assert lib.edgehip_depth_fill_size(ctx, C.byref(gw), C.byref(gh)) == ERR_STATE
        assert lib.edgehip_download_depth_grid(ctx, 0, None, None, None) == ERR_STATE
        P = edgehip.DepthFillParams
        for bad in (P(0, 5, 10, 1.0, 5, 0, 1), P(5, 0, 10, 1.0, 5, 0, 1), P(65, 5, 10, 1.0, 5, 0, 1), P(5, 49, 10, 1.0, 5, 0, 1),
                    P(5, 5, -1, 1.0, 5, 0, 1), P(5, 5, 10, 1.0, 5, 3, 1), P(5, 5, 10, 1.0, 5, -1, 1)):
            assert lib.edgehip_depth_fill_enable(ctx, C.byref(bad)) == ERR_ARG
        assert lib.edgehip_depth_fill(ctx, 0) == ERR_STATE   # a refused enable leaves the fill off
        assert eh.depth_fill_enable(64, 0, block_h=48) == (1, 1)
        assert lib.edgehip_depth_fill(ctx, 2) == ERR_ARG
        assert lib.edgehip_depth_fill(ctx, -1) == ERR_ARG
        eh.depth_fill(0)   # an empty slot: ResetData's grid
        rho, s_rho, fixed = eh.download_depth_grid(1)
        assert rho.tolist() == [[1.0]] and s_rho.tolist() == [[40.0]] and not fixed.any()
        assert lib.edgehip_download_depth_grid(ctx, 2, None, None, None) == ERR_ARG
        assert lib.edgehip_download_depth_grids_batch(ctx, 0, None, None, None, None) == ERR_ARG
        assert eh.depth_fill_enable(None) is None
        assert lib.edgehip_depth_fill(ctx, 0) == ERR_STATE
        assert lib.edgehip_depth_fill_enable(None, None) == ERR_ARG
    finally:
        eh.close()


def _rows(rows):
    """KeyLine fields from (cx, cy, rho, s_rho, rho0, m_num, p_id, n_id) rows (tests/test_depth_fill_cpu.py's hand cases)."""
    a = np.array(rows, np.float64).reshape(-1, 8)
    return {"c_p": a[:, :2].astype(np.float32), "rho": a[:, 2], "s_rho": a[:, 3], "rho0": a[:, 4],
            "m_num": a[:, 5].astype(np.int32), "p_id": a[:, 6].astype(np.int32), "n_id": a[:, 7].astype(np.int32)}


HAND = [   # (w, h, block, iter_num, discard, rows): what each pins in the kernel
    (20, 20, 10, 0, 1, [(3, 3, float("nan"), 1.0, 1.0, 9, 0, 0)]),                       # NaN rho: not skipped, not weak, folded
    (20, 20, 10, 2, 0, [(3, 3, -2.0, 0.5, 3.0, 9, 0, 0), (13, 3, 1.0, 0.1, 1.0, 1, 0, 0)]),   # rho < 0 with discard 0 takes rho0; a weak one
    (20, 20, 10, 0, 1, [(3, 3, -2.0, 0.5, 3.0, 9, 0, 0)]),                               # ... and with discard 1 is dropped
    (25, 20, 10, 0, 1, [(21.0, 3.0, 1.0, 0.1, 1.0, 9, 0, 0)]),                           # x == gw on row 0: wraps to (0, 1)
    (25, 20, 10, 3, 1, [(21.0, 13.0, 1.0, 0.1, 1.0, 9, 0, 0), (4.0, 4.0, 2.0, 0.1, 1.0, 9, 0, 0)]),   # x == gw on the last row: dropped
    (16, 64, 16, 3, 1, [(5.0, 25.0, 2.0, 0.1, 1.0, 9, 0, 0)]),                           # a 1-wide grid (no coarse-fine level; images are >= 16 wide)
    (20, 20, 10, 1, 1, [(3, 3, 1.0, float("inf"), 1.0, 9, 0, 0), (13, 13, float("inf"), 1.0, 1.0, 9, 0, 0)]),   # non-finite values
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_cases_on_the_device(case):
    w, h, block, it, disc, rows = HAND[case]
    kl = _rows(rows)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=2, nslots=2)
    try:
        eh.upload_keylines(1, 0, to_records(kl))   # sequence 0 keeps an empty list
        eh.depth_fill_enable(block, it, 1.0, 5, 0, disc)
        eh.depth_fill(0)
        want = port.depth_fill(kl, w, h, block, block, it, 1.0, 5, 0, disc)
        assert_grid(eh.download_depth_grid(1), want, ("hand", case))
        assert_grid(eh.download_depth_grid(0), port.depth_fill(_rows([]), w, h, block, block, it, 1.0, 5, 0, disc), ("empty", case))
    finally:
        eh.close()


def _read_grids(path, w, h):
    out = []
    with open(path, "rb") as f:
        while True:
            hdr = f.read(16)
            if not hdr:
                return out
            p_id, kn, gw, gh = np.frombuffer(hdr, np.int32)
            kl = np.frombuffer(f.read(168 * kn), edgehip.KEYLINE_DTYPE).copy()
            grid = None
            if gw:
                n = int(gw) * int(gh)
                rho = np.frombuffer(f.read(8 * n), np.float64).reshape(gh, gw)
                s_rho = np.frombuffer(f.read(8 * n), np.float64).reshape(gh, gw)
                fixed = np.frombuffer(f.read(n), np.uint8).reshape(gh, gw).astype(bool)
                grid = (rho, s_rho, fixed)
            out.append((int(p_id), kl, grid))


def test_batch_group_callbacks_carry_the_grid_of_their_own_edge_map(tmp_path):
    """8 rebvo::REBVO objects in one batch group (&GPU BatchGroup) with &DepthFiller and output callbacks (surface_replay): every
    callback's PipeBuffer::depth_grid equals the port run on that callback's own ef."""
    from rebvo_amd.config import write_global_config
    exe = os.path.join(ROOT, "rebvo_amd", "lib", "surface_replay")
    if not os.path.exists(exe):
        pytest.fail("surface_replay not built — run __graft_entry__.build()")
    w, h, n_obj, n_fr = 376, 240, 8, 7
    frames = [f for f, _, _ in synth.billboard_sequence(w, h, 6)]
    np.stack(frames).tofile(tmp_path / "frames.rgb24")
    cfg = tmp_path / "cfg"
    write_global_config(cfg, edgehip.euroc_params(w, h), gpu=dict(group="df", size=n_obj))
    with open(cfg, "a") as f:
        f.write("\n&DepthFiller\nPixelBlockSize=10\nThreshRelRho=1\nThreshMatchNum=2\nIterNum=10\nBoundMode=1\nDiscard=0\n")
    prefix = tmp_path / "g"
    r = subprocess.run([exe, str(cfg), str(tmp_path / "frames.rgb24"), str(len(frames)), str(n_obj), str(n_fr), "1.0", "0.05",
                        "--group", "df", "--grid-dump", str(prefix)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    fixed_seen = 0
    for i in range(n_obj):
        recs = _read_grids(f"{prefix}.{i}.grid", w, h)
        assert len(recs) == n_fr - 1, (i, len(recs))
        for p_id, kl, grid in recs:
            assert grid is not None and len(kl) > 100, (i, p_id)
            assert_grid(grid, port.depth_fill(kl, w, h, 10, 10, 10, 1.0, 2, 1, 0), (i, p_id))
            fixed_seen += int(grid[2].sum())
    assert fixed_seen > 0


def test_batch_group_refuses_a_member_with_other_fill_parameters(tmp_path):
    """Members of one group whose &DepthFiller parameters differ (block size, fill off, Discard) are refused at Init(); the same
    parameters join (rebvo_group_depth_fill_selftest)."""
    import ctypes as C
    from rebvo_amd.config import write_global_config
    lib = C.CDLL(os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so"))
    lib.rebvo_group_depth_fill_selftest.restype = C.c_int
    lib.rebvo_group_depth_fill_selftest.argtypes = [C.c_char_p]
    cfg = tmp_path / "cfg"
    write_global_config(cfg, edgehip.euroc_params(376, 240))
    assert lib.rebvo_group_depth_fill_selftest(str(cfg).encode()) == 0
