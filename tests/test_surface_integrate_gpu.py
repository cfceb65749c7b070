"""GPU: the cross-view surface integration (edgehip_surface_*, rebvo_amd/csrc/surface_integrate.hip) against the reference's own
results (tests/golden/surface_integrate/*.npz) and the numpy restatement (tests/surface_integrate_port.py), flag for flag.  Fails, not
skips, when the library lacks the entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from rebvo_amd import edgehip, synth
from tests import depth_fill_port as fport
from tests import surface_integrate_port as port
from tests.test_surface_integrate_cpu import NAMES, load

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_MEMORY, ERR_STATE = -1, -3, -4


def upload(eh, views, slots=None):
    for k, v in enumerate(views):
        if v is not None:
            eh.surface_view_upload(k if slots is None else slots[k], v["rho"], v["s_rho"], v["Pose"], v["Pos"], v["K"])


def assert_flags(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name", NAMES)
def test_teacher_forced_golden(name):
    """A fixture's views uploaded, then its cuts in order (a cut without reset accumulates): every flag of every view equals the
    reference's after every cut — main.cpp:192's all-views cut, :201's single-view cut on top, and the others; edgehip_surface_space is
    analizeSpaceSize bit for bit."""
    g, views, cuts, ref, cam = load(name)
    eh = edgehip.EdgeHip(edgehip.euroc_params(int(g["w"]), int(g["h"])), nseq=1, nslots=2)
    try:
        assert eh.depth_fill_enable(int(g["bw"]), 1, block_h=int(g["bh"])) == g["rho"].shape[:0:-1]
        eh.surface_views_enable(len(views), g["n"])
        upload(eh, views)
        o, s = eh.surface_space()
        assert o.tobytes() == g["space_origin"].tobytes() and s.tobytes() == g["space_size"].tobytes(), (o, s)
        for c, (reset, cast) in enumerate(cuts):
            eh.surface_integrate(g["origin"], g["size"], cast, accumulate=not reset)
            got = eh.download_surface_visibility(list(range(len(views))))
            for k in range(len(views)):
                assert_flags(got[k], ref[c, k], (name, c, k))
        assert_flags(eh.download_surface_visibility(1), ref[-1, 1], (name, "single download"))
    finally:
        eh.close()


def to_records(fields):
    kl = np.zeros(len(fields["rho"]), edgehip.KEYLINE_DTYPE)
    for f in fport.FIELDS:
        kl[f] = fields[f]
    kl["m_id"] = -1
    return kl


def ring_poses(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        a, d = 2 * np.pi * k / n + rng.uniform(-0.1, 0.1), rng.uniform(0.8, 1.2)
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        out.append((R, -R @ np.array([0, 0, d]) + rng.uniform(-0.05, 0.05, 3), float(rng.uniform(0.8, 1.2))))
    return out


def padded_box(views, bw, bh, cam, pad=0.05):
    o, s = port.space(views, bw, bh, cam)
    lo, hi = o.copy(), o + s
    for v in views:
        lo, hi = np.minimum(lo, v["Pos"]), np.maximum(hi, v["Pos"])
    return lo - pad * (hi - lo), (hi - lo) * (1 + 2 * pad)


def test_through_the_pipeline_capture_equals_upload():
    """upload_keylines, depth_fill and surface_view_capture from the sequences of one context — the fill's grids never leave the
    device — equal uploading the downloaded grids of the same sequences into other slots, and the port on those grids."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "depth_fill", "376x240.npz"))
    w, h, b = 376, 240, 10
    lists = ["A", "B", "A", "B"]
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=len(lists), nslots=2)
    try:
        for s, n in enumerate(lists):
            kl = to_records({f: z[f"kl{n}_{f}"] for f in fport.FIELDS})
            eh.upload_keylines(s, 1, kl[: len(kl) - 40 * s])   # four different lists
        eh.depth_fill_enable(b, 10, 1.0, 5, 0, 1)
        eh.depth_fill(1)
        eh.surface_views_enable(8, (64, 64, 64))
        poses = ring_poses(len(lists), 7)
        for s, (R, pos, K) in enumerate(poses):
            eh.surface_view_capture(s, s, R, pos, K)
        grids = eh.download_depth_grids(list(range(len(lists))))
        assert len({g[0].tobytes() for g in grids}) == len(lists)
        cam = port.camera(eh.p.ppx, eh.p.ppy, eh.p.zfx, eh.p.zfy)
        views = [port.view(grids[s][0], grids[s][1], *poses[s]) for s in range(len(lists))]
        o, sz = padded_box(views, b, b, cam)
        so, ss = eh.surface_space()
        po, ps = port.space(views, b, b, cam)
        assert so.tobytes() == po.tobytes() and ss.tobytes() == ps.tobytes()
        eh.surface_integrate(o, sz)
        captured = eh.download_surface_visibility([0, 1, 2, 3])
        want, st = port.integrate(views, o, sz, (64, 64, 64), b, b, cam)
        assert st["ray_steps_outside"] == 0 and st["samples_outside"] == 0
        assert 0.02 < 1 - np.mean(want) < 0.98
        for k in range(4):
            assert_flags(captured[k], want[k], ("captured", k))
        # the same grids by upload, in other slots
        for k in range(4):
            eh.surface_view_clear(k)
        upload(eh, views, slots=[4, 5, 6, 7])
        eh.surface_integrate(o, sz)
        uploaded = eh.download_surface_visibility([4, 5, 6, 7])
        for k in range(4):
            assert_flags(uploaded[k], captured[k], ("uploaded", k))
    finally:
        eh.close()


def facing_walls(eh, b):
    """Two cameras that face each other, each with a flat wall behind the other's: the hand-made scene of the CPU tests, on the
    context's camera and grid."""
    gw, gh = eh.depth_fill_size()
    rho, s = np.full((gh, gw), 0.5), np.full((gh, gw), 0.02)
    turn = np.diag([-1.0, 1.0, -1.0])
    return [port.view(rho, s, np.eye(3), (0, 0, -1.5), 1.0), port.view(rho, s, turn, (0, 0, 1.5), 1.0)]


def run_both(eh, views, o, s, n, b, cast=None, what=""):
    cam = port.camera(eh.p.ppx, eh.p.ppy, eh.p.zfx, eh.p.zfy)
    upload(eh, views)
    eh.surface_integrate(o, s, cast)
    want, st = port.integrate(views, o, s, n, b, b, cam, cast)
    got = eh.download_surface_visibility([k for k, v in enumerate(views) if v is not None])
    for g, k in zip(got, [k for k, v in enumerate(views) if v is not None]):
        assert_flags(g, want[k], (what, k))
    return want, st


def test_departures_against_the_port():
    """A view outside the box, cells with rho = 0 / NaN / negative / inf, and rays with rho + s_rho = 0: as the port (dropped samples
    and steps, no samples, no steps)."""
    w, h, b, n = 376, 240, 10, (40, 40, 40)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=1, nslots=2)
    try:
        eh.depth_fill_enable(b, 1)
        eh.surface_views_enable(2, n)
        o, s = np.array([-4.0, -4.0, -4.0]), np.array([8.0, 8.0, 8.0])
        views = facing_walls(eh, b)
        base, st = run_both(eh, views, o, s, n, b, what="base")
        assert st["ray_steps_outside"] == 0 and st["samples_outside"] == 0 and not base[0].all() and not base[1].all()
        # the box holds nothing of the scene; then only camera 0's half of it
        far, st = run_both(eh, views, np.full(3, 10.0), np.full(3, 2.0), n, b, what="far box")
        assert far[0].all() and far[1].all() and st["samples_outside"] == st["samples"]
        _, st = run_both(eh, views, o, np.array([8.0, 8.0, 5.0]), n, b, what="half box")
        assert st["ray_steps_outside"] > 0 and st["voxels_marked"] > 0
        # cells without samples
        rho = views[1]["rho"].copy()
        rho[10, 18], rho[11, 18], rho[12, 18], rho[13, 18] = 0.0, np.nan, -0.5, np.inf
        bad = [views[0], port.view(rho, views[1]["s_rho"], views[1]["Pose"], views[1]["Pos"], 1.0)]
        got, _ = run_both(eh, bad, o, s, n, b, what="bad rho")
        assert not base[1][10:14, 18].any() and got[1][10:14, 18].all()
        # rays without length: all of view 0's, then one of them
        s0 = -views[0]["rho"]
        got, st = run_both(eh, [port.view(views[0]["rho"], s0, np.eye(3), views[0]["Pos"], 1.0), views[1]], o, s, n, b, cast=[0], what="no rays")
        assert st["voxels_marked"] == 0 and got[1].all()
        s0 = views[0]["s_rho"].copy()
        s0[12, 18] = -views[0]["rho"][12, 18]
        got, st = run_both(eh, [port.view(views[0]["rho"], s0, np.eye(3), views[0]["Pos"], 1.0), views[1]], o, s, n, b, cast=[0], what="one ray less")
        assert st["voxels_marked"] > 0 and not got[1].all()
    finally:
        eh.close()


def test_accumulate_subsets_clear_and_recapture():
    """accumulate 0 / 1, cast_views subsets, a cleared view is skipped (casts nothing, is not tested, cannot be downloaded), and a
    view captured again is visible again."""
    w, h, b, n = 376, 240, 10, (40, 40, 40)
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=1, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        eh.depth_fill_enable(b, 1)
        eh.depth_fill(0)                       # an empty list: rho 1, s_rho 40 everywhere
        eh.surface_views_enable(3, n)
        cam = port.camera(eh.p.ppx, eh.p.ppy, eh.p.zfx, eh.p.zfy)
        o, s = np.array([-4.0, -4.0, -4.0]), np.array([8.0, 8.0, 8.0])
        a, c = facing_walls(eh, b)
        views = [a, None, c]                   # slot 1 stays empty
        upload(eh, views)
        eh.surface_integrate(o, s, [0])
        v0 = eh.download_surface_visibility([0, 2])
        want0, _ = port.integrate(views, o, s, n, b, b, cam, [0])
        assert v0[0].all() and not v0[1].all()
        assert_flags(v0[1], want0[2], "cast [0]")
        eh.surface_integrate(o, s, [2, 1], accumulate=True)      # the empty slot in the list is skipped
        v1 = eh.download_surface_visibility([0, 2])
        want1, _ = port.integrate(views, o, s, n, b, b, cam, [2], vis=want0)
        assert_flags(v1[0], want1[0], "accumulated 0")
        assert_flags(v1[1], want1[2], "accumulated 2")
        assert not v1[0].all() and np.array_equal(v1[1], v0[1])
        eh.surface_integrate(o, s, [2])                           # accumulate = 0 resets first
        v2 = eh.download_surface_visibility([0, 2])
        assert np.array_equal(v2[0], v1[0]) and v2[1].all()
        eh.surface_integrate(o, s, [], accumulate=False)          # nobody casts: everything visible
        assert all(v.all() for v in eh.download_surface_visibility([0, 2]))
        assert lib.edgehip_download_surface_visibility(ctx, 1, None) == ERR_STATE   # an empty slot
        # a cleared view casts nothing and is not tested
        eh.surface_integrate(o, s)
        both = eh.download_surface_visibility([0, 2])
        assert not both[0].all() and not both[1].all()
        eh.surface_view_clear(2)
        eh.surface_integrate(o, s)
        assert eh.download_surface_visibility(0).all()
        assert lib.edgehip_download_surface_visibility(ctx, 2, None) == ERR_STATE
        so, ss = eh.surface_space()
        po, ps = port.space([a], b, b, cam)
        assert so.tobytes() == po.tobytes() and ss.tobytes() == ps.tobytes()
        # back by capture (the fill's grid of sequence 0 with c's pose): visible again, whatever the slot held before
        upload(eh, [None, None, c])
        eh.surface_integrate(o, s)
        assert not eh.download_surface_visibility(2).all()
        eh.surface_view_capture(0, 2, c["Pose"], c["Pos"], 1.0)
        assert eh.download_surface_visibility(2).all()
        rho, s_rho, _ = eh.download_depth_grid(0)
        eh.surface_integrate(o, s)
        want, _ = port.integrate([a, None, port.view(rho, s_rho, c["Pose"], c["Pos"], 1.0)], o, s, n, b, b, cam)
        got = eh.download_surface_visibility([0, 2])
        assert_flags(got[0], want[0], "recaptured 0")
        assert_flags(got[1], want[2], "recaptured 2")
    finally:
        eh.close()


def test_argument_state_and_memory_errors():
    """ERR_STATE while the fill is off, ERR_ARG for a capacity or dimension < 1, ERR_MEMORY for a plane the device cannot hold; after
    every error the context still runs a frame and a fill.  Re-sizing or disabling the fill frees the store."""
    w, h = 376, 240
    eh = edgehip.EdgeHip(edgehip.euroc_params(w, h), nseq=1, nslots=3)
    lib, ctx = eh.lib, eh.ctx
    P = edgehip.SurfaceViewsParams
    frames = [f for f, _, _ in synth.billboard_sequence(w, h, 4)]
    state = {"k": 0, "fill": False}

    def still_works():
        k = state["k"]
        eh.upload_rgb(eh.next_slot(), frames[k % len(frames)])
        eh.process_frame(0.05 * k)
        assert eh.read_nav()[0].kn > 0
        if state["fill"]:
            eh.depth_fill(eh.cur_slot())
            assert np.isfinite(eh.download_depth_grid(0)[0]).all()
        state["k"] += 1

    try:
        d3 = (C.c_double * 3)(1, 1, 1)
        assert lib.edgehip_surface_views_enable(ctx, C.byref(P(4, 8, 8, 8))) == ERR_STATE   # the fill is off
        assert lib.edgehip_surface_integrate(ctx, d3, d3, 0, None, 0) == ERR_STATE
        assert lib.edgehip_surface_space(ctx, d3, d3) == ERR_STATE
        assert lib.edgehip_surface_view_clear(ctx, 0) == ERR_STATE
        still_works()
        eh.depth_fill_enable(10, 5)
        state["fill"] = True
        for bad in (P(0, 8, 8, 8), P(-1, 8, 8, 8), P(4, 0, 8, 8), P(4, 8, -3, 8), P(4, 8, 8, 0), P(1025, 8, 8, 8)):
            assert lib.edgehip_surface_views_enable(ctx, C.byref(bad)) == ERR_ARG
            assert lib.edgehip_surface_space(ctx, d3, d3) == ERR_STATE                      # nothing was enabled
        still_works()
        assert lib.edgehip_surface_views_enable(ctx, C.byref(P(4, 16000, 16000, 16000))) == ERR_MEMORY   # 16 TB of voxels
        assert lib.edgehip_last_error()
        assert lib.edgehip_surface_space(ctx, d3, d3) == ERR_STATE
        still_works()
        eh.surface_views_enable(4, 8)
        assert lib.edgehip_surface_view_capture(ctx, 0, 4, d3, d3, C.c_double(1)) == ERR_ARG   # view out of range
        assert lib.edgehip_surface_view_capture(ctx, 1, 0, d3, d3, C.c_double(1)) == ERR_ARG   # sequence out of range
        assert lib.edgehip_surface_view_clear(ctx, -1) == ERR_ARG
        one = (C.c_int32 * 1)(7)
        assert lib.edgehip_surface_integrate(ctx, d3, d3, 1, one, 0) == ERR_ARG                # casting view out of range
        zero = (C.c_double * 3)(1, 0, 1)
        assert lib.edgehip_surface_integrate(ctx, d3, zero, 0, None, 0) == ERR_ARG             # a box without volume
        assert lib.edgehip_surface_integrate(ctx, None, d3, 0, None, 0) == ERR_ARG
        eh.surface_view_capture(0, 0, np.eye(3), np.zeros(3), 1.0)
        eh.surface_integrate([-9, -9, -9], [18, 18, 18])
        assert eh.download_surface_visibility(0).all()                                         # a single view hides nothing
        still_works()
        eh.depth_fill_enable(10, 3)            # the same blocks: the store stays
        assert eh.download_surface_visibility(0).all()
        eh.depth_fill_enable(5, 3)             # other blocks: freed
        assert lib.edgehip_surface_space(ctx, d3, d3) == ERR_STATE
        eh.surface_views_enable(2, 8)
        assert lib.edgehip_surface_view_capture(ctx, 0, 0, d3, d3, C.c_double(1)) == ERR_STATE  # no fill since the fill's enable
        eh.depth_fill_enable(None)             # disabling the fill frees it too
        state["fill"] = False
        assert lib.edgehip_surface_space(ctx, d3, d3) == ERR_STATE
        assert lib.edgehip_surface_views_enable(ctx, None) == 0
        still_works()
    finally:
        eh.close()


def test_500_cubed_with_64_slots():
    """kf_visualizer's 500 x 500 x 500 grid with 64 view slots: the 752x480 scene's eight views spread over the slots, in the
    fixture's box; every flag equals the port's.  (2 GB are not needed: the plane is 4 B per voxel, 500 MB.)"""
    g, views, cuts, ref, cam = load("752x480_b10")
    slots = [0, 9, 18, 27, 36, 45, 54, 63]
    n = (500, 500, 500)
    eh = edgehip.EdgeHip(edgehip.euroc_params(752, 480), nseq=1, nslots=2)
    try:
        eh.depth_fill_enable(10, 1)
        eh.surface_views_enable(64, n)
        upload(eh, views, slots)
        eh.surface_integrate(g["origin"], g["size"])
        got = eh.download_surface_visibility(slots)
        sparse = [None] * 64
        for k, s in enumerate(slots):
            sparse[s] = views[k]
        want, st = port.integrate(sparse, g["origin"], g["size"], n, 10, 10, cam)
        assert st["ray_steps_outside"] == 0 and st["samples_outside"] == 0
        hid = 1 - np.mean([want[s] for s in slots])
        print(f"500^3: {st['voxels_marked']} voxels marked, {st['samples']} samples, hidden {hid:.3f}")
        assert 0.05 < hid < 0.95
        for k, s in enumerate(slots):
            assert_flags(got[k], want[s], ("500^3", s))
        eh.surface_integrate(g["origin"], g["size"], [63], accumulate=True)   # nothing new on top
        again = eh.download_surface_visibility(slots)
        assert all(np.array_equal(a, b) for a, b in zip(again, got))
    finally:
        eh.close()
