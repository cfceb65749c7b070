"""GPU: the exhaustive cross-view ray check (edgehip_surface_ray_cross, k_sv_ray_cross in rebvo_amd/csrc/surface_integrate.hip) against
the reference's own flags (tests/golden/surface_ray_cross/*.npz) and the numpy restatement (tests/surface_ray_cross_port.py), flag for
flag, nothing excluded.  The 37x24 grid (888 cells) leaves a ragged last wave and a partial ray tile; the 75x48 grid (3600 cells)
crosses several tiles and blocks.  Fails, not skips, when the library lacks the entry point."""
import ctypes as C

import numpy as np
import pytest

from rebvo_amd import edgehip
from tests import surface_ray_cross_port as port
from tests.test_surface_ray_cross_cpu import NAMES, load

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4


def context(fx, capacity=None, n=1):
    eh = edgehip.EdgeHip(edgehip.euroc_params(fx["w"], fx["h"]), nseq=1, nslots=2)
    gh, gw = fx["views"][0]["rho"].shape
    assert eh.depth_fill_enable(fx["bw"], 1, block_h=fx["bh"]) == (gw, gh)
    eh.surface_views_enable(len(fx["views"]) if capacity is None else capacity, n)
    return eh


def upload(eh, views, slots=None):
    for k, v in enumerate(views):
        if v is not None:
            eh.surface_view_upload(k if slots is None else slots[k], v["rho"], v["s_rho"], v["Pose"], v["Pos"], v["K"])


def assert_flags(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.argwhere(got != want)[:4])


def call_abi(eh, pairs, accumulate):
    if pairs is None:
        return eh.lib.edgehip_surface_ray_cross(eh.ctx, -1, None, None, int(accumulate))
    t = (C.c_int32 * max(len(pairs), 1))(*[p[0] for p in pairs])
    h = (C.c_int32 * max(len(pairs), 1))(*[p[1] for p in pairs])
    return eh.lib.edgehip_surface_ray_cross(eh.ctx, len(pairs), t, h, int(accumulate))


def run_steps(fx, name, through, ocgrid_steps, n):
    """Every step of a fixture in order; a step that falls from the OcGrid cut's flags runs edgehip_surface_integrate first (the cut
    the surface_integrate fixture recorded, in its box and voxel grid) and accumulates on it."""
    eh = context(fx, n=n)
    try:
        upload(eh, fx["views"])
        every = list(range(len(fx["views"])))
        done = 0
        for i, (start, absent, pairs) in enumerate(fx["steps"]):
            if start == 2 and not ocgrid_steps:
                continue
            if absent >= 0:
                eh.surface_view_clear(absent)
            if start == 2:
                eh.surface_integrate(fx["src"]["origin"], fx["src"]["size"])
                for k, g in zip(every, eh.download_surface_visibility(every)):
                    assert_flags(g, fx["ocgrid"][k], (name, i, k, "OcGrid cut"))
            if start == 0:
                assert done == i, "an accumulating step needs the step before it"
            if through == "abi":
                assert call_abi(eh, pairs, start != 1) == 0, eh.lib.edgehip_last_error()
            else:
                eh.surface_ray_cross(pairs, accumulate=start != 1)
            keep = [k for k in every if k != absent]
            for k, g in zip(keep, eh.download_surface_visibility(keep)):
                assert_flags(g, fx["ref"][i, k], (name, through, i, k))
            if absent >= 0:
                assert eh.lib.edgehip_download_surface_visibility(eh.ctx, absent, None) == ERR_STATE
                upload(eh, [v if k == absent else None for k, v in enumerate(fx["views"])])
            done = i + 1
    finally:
        eh.close()


@pytest.mark.parametrize("through", ["abi", "python"])
@pytest.mark.parametrize("name", NAMES)
def test_every_step_equals_the_reference(name, through):
    """Every step of every fixture, through the C ABI and through EdgeHip.surface_ray_cross: every flag of every view equals the
    reference's after every step."""
    fx = load(name)
    run_steps(fx, name, through, True, 1 if fx["src"] is None else fx["src"]["n"])


@pytest.mark.parametrize("name", ["376x240_b10", "crafted"])
def test_store_with_a_1x1x1_plane(name):
    """The check needs no voxel plane: the store enabled with nx = ny = nz = 1 gives the same flags (the steps that fall from an OcGrid
    cut are left to the test above)."""
    run_steps(load(name), name, "abi", False, 1)


def test_argument_and_state_errors():
    """ERR_STATE before the store is enabled; ERR_ARG for ids out of range, a pair with t == h and inconsistent lists; an error changes
    no flag; pairs that name an empty slot are skipped; accumulate keeps, accumulate = 0 resets."""
    fx = load("376x240_b10")
    eh = edgehip.EdgeHip(edgehip.euroc_params(fx["w"], fx["h"]), nseq=1, nslots=2)
    lib, ctx = eh.lib, eh.ctx
    try:
        assert call_abi(eh, None, 0) == ERR_STATE                  # neither the fill nor the store
        eh.depth_fill_enable(fx["bw"], 1)
        assert call_abi(eh, [(0, 1)], 0) == ERR_STATE
        eh.surface_views_enable(6, 1)
        assert call_abi(eh, None, 0) == 0                          # nothing stored: nothing to do
        upload(eh, fx["views"])                                    # slots 0..3; 4 and 5 stay empty
        assert call_abi(eh, [(0, 3)], 0) == 0
        first = eh.download_surface_visibility(0)
        assert_flags(first, fx["ref"][1, 0], "one pair")
        for bad in ([(0, 6)], [(6, 0)], [(-1, 0)], [(0, -1)], [(1, 0), (2, 2)], [(5, 5)]):
            assert call_abi(eh, bad, 0) == ERR_ARG, bad
            assert lib.edgehip_last_error()
        one = (C.c_int32 * 1)(0)
        assert lib.edgehip_surface_ray_cross(ctx, 1, None, one, 0) == ERR_ARG
        assert lib.edgehip_surface_ray_cross(ctx, 1, one, None, 0) == ERR_ARG
        assert lib.edgehip_surface_ray_cross(ctx, -1, one, one, 0) == ERR_ARG
        assert lib.edgehip_surface_ray_cross(ctx, -1, one, None, 0) == ERR_ARG
        with pytest.raises(edgehip.EdgeHipError):
            eh.surface_ray_cross([(1, 1)])
        assert_flags(eh.download_surface_visibility(0), first, "errors change nothing")   # not even the reset of accumulate = 0
        assert call_abi(eh, [(0, 4), (5, 0), (4, 5)], 1) == 0      # empty slots: skipped
        assert_flags(eh.download_surface_visibility(0), first, "skipped pairs")
        assert call_abi(eh, [], 1) == 0
        assert_flags(eh.download_surface_visibility(0), first, "an empty list keeps")
        eh.surface_ray_cross([], accumulate=False)
        assert eh.download_surface_visibility(0).all()             # an empty list after a reset: all visible
        eh.surface_ray_cross([(0, 3), (0, 3), (0, 3)])             # the same pair more than once: the same bytes, the same value
        assert_flags(eh.download_surface_visibility(0), first, "repeated pair")
        # a longer list than any before (the pair buffer grows), then the frame path still runs
        eh.surface_ray_cross(port.all_pairs(fx["views"]) * 3)
        for k, g in enumerate(eh.download_surface_visibility([0, 1, 2, 3])):
            assert_flags(g, fx["ref"][0, k], ("grown list", k))
    finally:
        eh.close()


def test_all_pairs_of_64_views():
    """64 uploaded views — the 752x480 scene's eight, repeated with shifted poses — and the all-pairs launch (4032 pairs): the flags of
    a sample of eight views, one of each base view and of each repeat, equal the port's over their 63 hidders."""
    fx = load("752x480_b10")
    rng = np.random.default_rng(64)
    views = []
    for k in range(64):
        b = fx["views"][k % 8]
        shift = np.zeros(3) if k < 8 else rng.uniform(-0.25, 0.25, 3)
        views.append(port.view(b["rho"], b["s_rho"], b["Pose"], b["Pos"] + shift, b["K"]))
    sample = [0, 9, 18, 27, 36, 45, 54, 63]
    eh = context(fx, capacity=64)
    try:
        upload(eh, views)
        eh.surface_ray_cross()
        got = eh.download_surface_visibility(sample)
    finally:
        eh.close()
    hid = []
    for g, t in zip(got, sample):
        want = port.ray_cross(views, [(t, h) for h in range(64) if h != t], fx["bw"], fx["bh"], fx["cam"], cull=True)[t]
        hid.append(round(1 - float(want.mean()), 3))
        assert_flags(g, want, ("64 views", t))
    print("64 views: hidden share of the sampled views", hid)
    assert 0 < min(hid) < 0.95          # both outcomes among the sample
