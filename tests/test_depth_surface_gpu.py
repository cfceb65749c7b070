"""GPU: the depth surface (edgehip_depth_surface, rebvo_amd/csrc/depth_surface.hip) against the reference's own results
(tests/golden/depth_surface/*.npz) and the numpy restatement (tests/depth_surface_port.py), bit for bit.  Fails, not skips, when
the library lacks the entry points."""
import glob
import os

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import depth_fill_port as fport
from tests import depth_surface_port as port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "depth_surface")
ERR_ARG, ERR_STATE = -1, -4
SENTINEL64 = 0x7FF4DEADBEEF0001   # tools/depth_surface_ref_driver.cpp
SENTINEL32 = 0x7FA0DEAD


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    """Bit for bit, except that a NaN the arithmetic creates equals any NaN: the GPU's default NaN is positive, x86 SSE's negative."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    ok = same_bits(got, want)
    assert ok.all(), (what, int((~ok).sum()), got[~ok][:4], want[~ok][:4])


def assert_surface(got, want, what):
    for k in ("point", "dist", "normal", "area"):
        assert_same(got[k], want[k], (what, k))
    assert bits(np.float64(got["min_dist"])) == bits(np.float64(want["min_dist"])), (what, got["min_dist"], want["min_dist"])


def to_records(fields):
    kl = np.zeros(len(fields["rho"]), edgehip.KEYLINE_DTYPE)
    for f in fport.FIELDS:
        kl[f] = fields[f]
    kl["m_id"] = -1
    return kl


def reference_surface(g):
    """The fixture's surface; the cells the reference never writes (its sentinel) must be NaN."""
    out = {k: g[k] for k in ("point", "dist", "min_dist", "normal", "area")}
    out["normal"] = np.where(bits(g["normal"]) == SENTINEL64, np.nan, g["normal"])
    out["area"] = np.where(bits(g["area"]) == SENTINEL32, np.float32(np.nan), g["area"]).astype(np.float32)
    return out


@pytest.mark.parametrize("name", ["376x240", "752x480"])
def test_teacher_forced_golden(name):
    """The fixture lists through edgehip_upload_keylines, the fill, then the surface in both image modes: every case against the
    reference's own results (whole images where the fixtures hold them, else the pixel sample and the borders)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "depth_fill", f"{name}.npz"))
    w, h = int(z["w"]), int(z["h"])
    names = sorted({k[2] for k in z.files if k.startswith("kl") and k.endswith("_rho")})
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=len(names), nslots=2)
    try:
        for s, n in enumerate(names):
            eh.upload_keylines(s, 1, to_records({f: z[f"kl{n}_{f}"] for f in fport.FIELDS}))
        for i, (lst, bw, bh, it, mode, disc, m) in enumerate(z["cases"]):
            g = np.load(os.path.join(GOLD, f"{name}_case{i}.npz"))
            s = names.index(chr(lst))
            eh.depth_fill_enable(int(bw), int(it), float(z[f"case{i}_thresh_rel_rho"]), int(m), int(mode), int(disc), block_h=int(bh))
            eh.depth_fill(1)
            for image_mode in (1, 2):
                eh.depth_surface_enable(True, image_mode)
                eh.depth_surface()
                assert_surface(eh.download_depth_surface(s), reference_surface(g), (name, i))
                rho, s_rho = eh.download_depth_image(s)
                whole = os.path.join(GOLD, f"{name}_case{i}_image{image_mode}.npz")
                if os.path.exists(whole):
                    ref = np.load(whole)
                    assert_same(rho, ref["rho"], (name, i, image_mode, "rho"))
                    assert_same(s_rho, ref["s_rho"], (name, i, image_mode, "s_rho"))
                if "sample" in g.files:
                    px, py = g["sample"][:, 0], g["sample"][:, 1]
                    assert_same(rho[py, px], g["image"][2 * image_mode - 2], (name, i, image_mode, "rho sample"))
                    assert_same(s_rho[py, px], g["image"][2 * image_mode - 1], (name, i, image_mode, "s_rho sample"))
    finally:
        eh.close()


def _pool(w, h, n):
    import torch
    mono = np.stack([np.ascontiguousarray(f[:, :, 0]) for f, _, _ in synth.billboard_sequence(w, h, n)])
    t = torch.empty(mono.size + 16, dtype=torch.uint8, device="cuda")
    t[:mono.size] = torch.from_numpy(mono.reshape(-1)).cuda()
    return t


def _check_against_port(eh, seqs, w, h, block, image_mode, what):
    grids = eh.download_depth_grids(seqs)
    surfs = eh.download_depth_surfaces(seqs)
    imgs = eh.download_depth_images(seqs)
    cam = port.camera(eh.p.ppx, eh.p.ppy, eh.p.zfx, eh.p.zfy)
    for j, s in enumerate(seqs):
        rho, s_rho, _ = grids[j]
        assert_surface(surfs[j], port.surface(rho, block, block, cam), (what, s))
        want = port.image(rho, s_rho, w, h, block, block, image_mode)
        assert_same(imgs[j][0], want[0], (what, s, "rho"))
        assert_same(imgs[j][1], want[1], (what, s, "s_rho"))
    return grids, imgs


@pytest.mark.parametrize("block,image_mode", [(10, 1), (5, 2)])
def test_1024_sequences_live_replay(block, image_mode):
    """1024 sequences at 752x480 through edgehip_process_frame, the fill and the surface after every frame; sequences 0, 511 and
    1023 against the port on the downloaded grid; depth_image_into a torch tensor equals the host download."""
    import torch
    w, h, nseq, frames = 752, 480, 1024, 3
    pool = _pool(w, h, frames + 2)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
    try:
        eh.depth_fill_enable(block, 10, 1.0, 2, 0, 1)
        eh.depth_surface_enable(True, image_mode)
        for k in range(frames):
            idx = np.array([k + (s % 3) for s in range(nseq)], np.int32)
            eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), frames + 2, idx)
            eh.process_frame(np.full(nseq, 0.05 * k))
            eh.depth_fill(eh.cur_slot())
            eh.depth_surface()
            grids, imgs = _check_against_port(eh, [0, 511, 1023], w, h, block, image_mode, (block, k))
        assert grids[0][2].sum() > 50
        rt = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
        st = torch.empty((3, h, w), dtype=torch.float32, device="cuda")
        eh.depth_image_into(rt, st, first=1021)
        assert np.array_equal(bits(rt[2].cpu().numpy()), bits(imgs[2][0]))
        assert np.array_equal(bits(st[2].cpu().numpy()), bits(imgs[2][1]))
        lo, hi = eh.download_depth_images([1021, 1022])
        assert np.array_equal(bits(rt[0].cpu().numpy()), bits(lo[0])) and np.array_equal(bits(st[1].cpu().numpy()), bits(hi[1]))
    finally:
        eh.close()


def test_surface_does_not_change_tracking_or_grids():
    """Nav records and fill grids bit-identical with the surface (and the image) run after every frame and without it."""
    w, h, nseq, frames = 376, 240, 4, 5
    pool = _pool(w, h, frames + 3)
    runs = []
    for surf in (True, False):
        eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=nseq, nslots=3)
        try:
            eh.depth_fill_enable(5, 10, 1.0, 2, 0, 1)
            if surf:
                eh.depth_surface_enable(True, 2)
            navs, grids = [], []
            for k in range(frames):
                idx = np.array([k + s % 3 for s in range(nseq)], np.int32)
                eh.bind_grey8_indexed(eh.next_slot(), pool.data_ptr(), frames + 3, idx)
                eh.process_frame(np.full(nseq, 0.05 * k))
                eh.depth_fill(eh.cur_slot())
                if surf:
                    eh.depth_surface()
                navs.append(b"".join(bytes(n) for n in eh.read_nav()))
                grids.append(b"".join(a.tobytes() for g in eh.download_depth_grids(list(range(nseq))) for a in g))
            runs.append((navs, grids))
        finally:
            eh.close()
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1]


def test_argument_and_state_errors():
    import ctypes as C
    eh = edgehip.EdgeHip(edgehip.euroc_params(64, 48), nseq=2, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    P = edgehip.DepthSurfaceParams
    try:
        assert lib.edgehip_depth_surface_enable(ctx, C.byref(P(1, 0))) == ERR_STATE   # the fill is off
        assert lib.edgehip_depth_surface(ctx) == ERR_STATE
        eh.depth_fill_enable(8, 2)
        for bad in (P(1, 3), P(1, -1), P(0, 7)):
            assert lib.edgehip_depth_surface_enable(ctx, C.byref(bad)) == ERR_ARG
        assert lib.edgehip_depth_surface(ctx) == ERR_STATE                             # not enabled
        assert lib.edgehip_depth_surface_enable(ctx, C.byref(P(0, 0))) == 0            # both off: nothing enabled
        assert lib.edgehip_depth_surface(ctx) == ERR_STATE
        eh.depth_surface_enable(True, 0)
        assert lib.edgehip_depth_surface(ctx) == ERR_STATE                             # no fill since the fill's enable
        assert lib.edgehip_download_depth_image(ctx, 0, None, None) == ERR_STATE       # the image is off
        assert lib.edgehip_depth_image_device(ctx, 0, 1, None, None) == ERR_STATE
        eh.depth_fill(0)
        eh.depth_surface()
        s = eh.download_depth_surface(1)   # an empty list: rho 1 everywhere
        assert s["point"].shape == (6, 8, 3) and np.isfinite(s["point"]).all() and s["min_dist"] < 1e20
        assert lib.edgehip_download_depth_surface(ctx, 2, None, None, None, None, None) == ERR_ARG
        assert lib.edgehip_download_depth_surfaces_batch(ctx, 0, None, None, None, None, None, None) == ERR_ARG
        eh.depth_surface_enable(False, 1)
        assert lib.edgehip_download_depth_surface(ctx, 0, None, None, None, None, None) == ERR_STATE   # the surface is off
        eh.depth_surface()
        assert lib.edgehip_depth_image_device(ctx, 1, 2, None, None) == ERR_ARG
        eh.depth_fill_enable(8, 5)          # the same blocks: the products stay, and read the next fill's grids
        assert lib.edgehip_depth_surface(ctx) == ERR_STATE
        eh.depth_fill(0)
        eh.depth_surface()
        eh.depth_fill_enable(4, 2)          # other blocks: the products are freed
        eh.depth_fill(0)
        assert lib.edgehip_depth_surface(ctx) == ERR_STATE
        eh.depth_surface_enable(True, 2)
        eh.depth_surface()
        assert eh.depth_fill_enable(None) is None   # disabling the fill frees them too
        assert lib.edgehip_depth_surface(ctx) == ERR_STATE
        assert lib.edgehip_download_depth_image(ctx, 0, None, None) == ERR_STATE
        assert lib.edgehip_depth_surface_enable(ctx, None) == 0
    finally:
        eh.close()


def test_degenerate_grids_hold_nan_where_nothing_is_written():
    """A 1-wide grid: calcSurfNormals and calcSurfArea never write; every normal and area is NaN, points and images as the port."""
    w, h = 16, 64
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=1, nslots=2)
    try:
        eh.depth_fill_enable(16, 3)
        eh.depth_fill(0)
        eh.depth_surface_enable(True, 1)
        eh.depth_surface()
        s = eh.download_depth_surface(0)
        assert np.isnan(s["normal"]).all() and np.isnan(s["area"]).all()
        rho, s_rho, _ = eh.download_depth_grid(0)
        cam = port.camera(eh.p.ppx, eh.p.ppy, eh.p.zfx, eh.p.zfy)
        assert_surface(s, port.surface(rho, 16, 16, cam), "1-wide")
        r, sr = eh.download_depth_image(0)
        want = port.image(rho, s_rho, w, h, 16, 16, 1)
        assert_same(r, want[0], "1-wide rho")
        assert_same(sr, want[1], "1-wide s_rho")
    finally:
        eh.close()


def test_width_not_a_multiple_of_four():
    """w % 4 != 0 (the image's per-pixel stores) with a partial column and row of cells, both image modes, against the port."""
    w, h, bw = 25, 20, 7
    kl = {"c_p": np.array([[3, 3], [17, 12], [22, 4]], np.float32), "rho": np.array([1.0, 2.5, 0.7]), "s_rho": np.array([0.1, 0.2, 0.1]),
          "rho0": np.ones(3), "m_num": np.full(3, 9, np.int32), "p_id": np.zeros(3, np.int32), "n_id": np.zeros(3, np.int32)}
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=2, nslots=2)
    try:
        eh.upload_keylines(1, 0, to_records(kl))
        eh.depth_fill_enable(bw, 4)
        eh.depth_fill(0)
        cam = port.camera(eh.p.ppx, eh.p.ppy, eh.p.zfx, eh.p.zfy)
        for image_mode in (1, 2):
            eh.depth_surface_enable(True, image_mode)
            eh.depth_surface()
            for s in (0, 1):
                rho, s_rho, _ = eh.download_depth_grid(s)
                assert_surface(eh.download_depth_surface(s), port.surface(rho, bw, bw, cam), (image_mode, s))
                r, sr = eh.download_depth_image(s)
                want = port.image(rho, s_rho, w, h, bw, bw, image_mode)
                assert_same(r, want[0], (image_mode, s, "rho"))
                assert_same(sr, want[1], (image_mode, s, "s_rho"))
    finally:
        eh.close()


def test_fixture_set_is_complete():
    assert len(glob.glob(os.path.join(GOLD, "*_case*.npz"))) == 20


def _read_surfaces(path):
    out = []
    with open(path, "rb") as f:
        while True:
            hdr = f.read(28)
            if not hdr:
                return out
            p_id, gw, gh, has_surf, w, h, mode = (int(v) for v in np.frombuffer(hdr, np.int32))
            pose = np.frombuffer(f.read(8 * 13), np.float64)
            rec = {"p_id": p_id, "Pose": pose[:9].reshape(3, 3), "Pos": pose[9:12], "K": pose[12], "mode": mode}
            G, N = gw * gh, w * h
            if gw:
                rec["rho"] = np.frombuffer(f.read(8 * G), np.float64).reshape(gh, gw)
                rec["s_rho"] = np.frombuffer(f.read(8 * G), np.float64).reshape(gh, gw)
            if has_surf:
                rec["surface"] = dict(point=np.frombuffer(f.read(24 * G), np.float64).reshape(gh, gw, 3),
                                      normal=np.frombuffer(f.read(24 * G), np.float64).reshape(gh, gw, 3),
                                      dist=np.frombuffer(f.read(8 * G), np.float64).reshape(gh, gw),
                                      min_dist=float(np.frombuffer(f.read(8), np.float64)[0]),
                                      area=np.frombuffer(f.read(4 * G), np.float32).reshape(gh, gw))
            if mode:
                rec["image"] = (np.frombuffer(f.read(4 * N), np.float32).reshape(h, w), np.frombuffer(f.read(4 * N), np.float32).reshape(h, w))
            out.append(rec)


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode().splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    n = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    v = np.frombuffer(data[end:], np.float32)
    assert v.size == 6 * n
    return v.reshape(n, 6)


def test_batch_group_callbacks_carry_surface_and_image(tmp_path):
    """8 rebvo::REBVO objects in one batch group with &DepthFiller Surface = 1, DenseImage = 1 and output callbacks (surface_replay):
    every callback's PipeBuffer::depth_surface / depth_image equals the port run on its own depth_grid; --ply writes the finite
    points, with normals, in the world frame (Pose * p * K + Pos, recomputed here)."""
    import subprocess
    from rebvo_amd.config import write_global_config
    exe = os.path.join(ROOT, "rebvo_amd", "lib", "surface_replay")
    if not os.path.exists(exe):
        pytest.fail("surface_replay not built — run __graft_entry__.build()")
    w, h, n_obj, n_fr = 376, 240, 8, 6
    frames = [f for f, _, _ in synth.billboard_sequence(w, h, 6)]
    np.stack(frames).tofile(tmp_path / "frames.rgb24")
    cfg = tmp_path / "cfg"
    p = edgehip.euroc_params(w, h)
    write_global_config(cfg, p, gpu=dict(group="ds", size=n_obj))
    with open(cfg, "a") as f:
        f.write("\n&DepthFiller\nPixelBlockSize=10\nThreshRelRho=1\nThreshMatchNum=2\nIterNum=10\nSurface=1\nDenseImage=1\n")
    prefix, ply = tmp_path / "s", tmp_path / "ply"
    ply.mkdir()
    r = subprocess.run([exe, str(cfg), str(tmp_path / "frames.rgb24"), str(len(frames)), str(n_obj), str(n_fr), "1.0", "0.05",
                        "--group", "ds", "--surface-dump", str(prefix), "--ply", str(ply), "--ply-every", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    cam = port.camera(p.ppx, p.ppy, p.zfx, p.zfy)
    plys = 0
    for i in range(n_obj):
        recs = _read_surfaces(f"{prefix}.{i}.surf")
        assert len(recs) == n_fr - 1, (i, len(recs))
        for k, rec in enumerate(recs):
            assert "surface" in rec and rec["mode"] == 1, (i, rec["p_id"])
            assert_surface(rec["surface"], port.surface(rec["rho"], 10, 10, cam), (i, rec["p_id"]))
            want = port.image(rec["rho"], rec["s_rho"], w, h, 10, 10, 1)
            assert_same(rec["image"][0], want[0], (i, rec["p_id"], "rho"))
            assert_same(rec["image"][1], want[1], (i, rec["p_id"], "s_rho"))
            path = ply / f"obj{i}_{rec['p_id']}.ply"
            assert path.exists() == (k % 2 == 0), (i, k)
            if not path.exists():
                continue
            v = _read_ply(path)
            P = rec["surface"]["point"].reshape(-1, 3)
            Nm = rec["surface"]["normal"].reshape(-1, 3)
            fin = np.isfinite(P).all(1)
            assert len(v) == int(fin.sum()) > 0
            Pose = rec["Pose"]
            world = np.zeros((int(fin.sum()), 3))
            nrm = np.zeros_like(world)
            for a in range(3):
                s = np.zeros(len(world))
                t = np.zeros(len(world))
                for b in range(3):
                    s = s + Pose[a, b] * P[fin, b]
                    t = t + Pose[a, b] * Nm[fin, b]
                world[:, a] = s * rec["K"] + rec["Pos"][a]
                nrm[:, a] = t
            assert np.array_equal(v[:, :3], world.astype(np.float32))
            assert same_bits(v[:, 3:], nrm.astype(np.float32)).all()
            plys += 1
    assert plys >= n_obj * 2


def test_batch_group_refuses_a_member_with_other_surface_keys(tmp_path):
    """Members of one group whose &DepthFiller Surface / DenseImage differ are refused at Init(); the same keys join
    (rebvo_group_depth_surface_selftest)."""
    import ctypes as C
    from rebvo_amd.config import write_global_config
    lib = C.CDLL(os.path.join(ROOT, "rebvo_amd", "lib", "librebvohost.so"))
    lib.rebvo_group_depth_surface_selftest.restype = C.c_int
    lib.rebvo_group_depth_surface_selftest.argtypes = [C.c_char_p]
    cfg = tmp_path / "cfg"
    write_global_config(cfg, edgehip.euroc_params(376, 240))
    assert lib.rebvo_group_depth_surface_selftest(str(cfg).encode()) == 0
