"""build_field's t-ranges on crafted KeyLine lists (GPU): the rasteriser tests a KeyLine's samples against its tile only at the two
ends of the range and, up to radius 127, reads the range from the bin entry (k_field_bin / k_field_raster, stage_b.hip; the argument:
tests/test_field_interval_cpu.py).  A 96 x 80 image — 2 x 2 tiles of 64 x 64, the right and the bottom ones clipped — with three
sequences of different lengths in one launch: a crafted list, an empty one and one that fills a bin to its capacity.  The {dist, ikl}
field (debug_planes) and the 16-bit KeyLine-index plane the tracker gathers are compared for equality with the reference's
build_field (global_tracker.cpp:61-105) and with the CPU port."""
import numpy as np
import pytest

from helpers import require_ref, to_edgehip_kl
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu

W, H, CAP = 96, 80, 384
RADII = (4, 40, 127, 128)          # 127: the last radius of the packed bin entry, 128: the first of the bare one


def crafted_list(r, seed):
    """(c_p, u_m) rows of the crafted sequence and the index ranges of its groups."""
    rs = np.random.RandomState(seed)
    rows, groups = [], {}

    def add(name, items):
        groups[name] = (len(rows), len(rows) + len(items))
        rows.extend(items)

    # an END sample exactly on k + 0.5 (x = 63.5 -> 64: the next tile; 95.5 -> 96 and 79.5 -> 80: outside the image), and one inside the range
    on_border = []
    for j in (r - 1, -r, 0, min(3, r - 1)):
        for k in (63, 95):
            for y in (10.0, 63.0, 64.0, 79.0):
                on_border += [(k + 0.5 - j, y, 1.0, 0.0), (k + 0.5 + j, y, -1.0, 0.0)]
        for k in (63, 79):
            for x in (10.0, 63.0, 64.0, 95.0):
                on_border += [(x, k + 0.5 - j, 0.0, 1.0), (x, k + 0.5 + j, 0.0, -1.0)]
    add("on_border", on_border)
    # a coordinate of exactly -0.5 in the tiles at column / row 0: round() says -1, outside
    half = []
    for j in (0, 1, r - 1, -r):
        half += [(-0.5 - j, 20.0, 1.0, 0.0), (-0.5 - j, 70.0, 1.0, 0.0), (20.0, -0.5 - j, 0.0, 1.0), (80.0, -0.5 - j, 0.0, 1.0)]
    half += [(-0.5, 30.0, 0.0, 1.0), (-0.5, 30.0, 5e-7, 1.0), (40.0, -0.5, 1.0, 0.0), (70.0, -0.5, -1.0, -5e-7), (-0.5, -0.5, 0.6, 0.8)]
    add("minus_half", half)
    # axis-parallel: |u| below, on and just above the 1e-6 gate, centres on both sides of the tile / image border
    gate = np.float32(1e-6)
    small = [0.0, 9e-7, -9e-7, float(gate), float(np.nextafter(gate, np.float32(1))), 1.1e-6, -1.1e-6, 1e-3, -1e-3]
    flat = []
    for s in small:
        for off in (63.49, 63.5, 63.51, 64.49, 95.49, 95.5):
            flat.append((off, rs.uniform(5, 75), s, 1.0))
        for off in (63.49, 63.5, 63.51, 64.49, 79.49, 79.5):
            flat.append((rs.uniform(5, 90), off, -1.0, s))
    add("axis_parallel", flat)
    # fully outside one tile of its bounding box: an anti-diagonal next to the corner where the four tiles meet misses tile (0, 0),
    # its mirror image misses tile (1, 1)
    d = float(np.float32(np.sqrt(0.5)))
    add("misses_a_tile", [(66.0, 66.0, d, -d), (66.5, 65.5, -d, d), (61.0, 61.0, d, -d), (60.5, 61.5, -d, d), (70.0, 70.0, d, -d)])
    # ties on |t| at a pixel: identical KeyLines, a crossing at t = 0, two collinear ones at equal distance: the larger id wins
    ties = [(30.0, 30.0, 1.0, 0.0), (30.0, 30.0, 0.0, 1.0), (30.0, 30.0, 1.0, 0.0), (28.0, 50.0, 1.0, 0.0), (32.0, 50.0, 1.0, 0.0),
            (70.0, 66.0, d, d), (70.0, 66.0, d, d), (70.0, 70.0, 0.0, 1.0), (74.0, 66.0, -1.0, 0.0)]
    add("ties", ties)
    # filler: any direction and length up to 1, centres over the whole image
    n = 60
    ang = rs.uniform(0, 2 * np.pi, n)
    ln = np.where(rs.rand(n) < 0.5, 1.0, rs.uniform(0.05, 1.0, n))
    add("random", list(zip(rs.uniform(0, W - 1, n), rs.uniform(0, H - 1, n), np.cos(ang) * ln, np.sin(ang) * ln)))
    return np.array(rows, np.float64), groups


def full_bin_list(seed):
    """CAP KeyLines whose centre pixel is in tile (0, 0): that tile's bin holds every one of them — bin_cap entries."""
    rs = np.random.RandomState(seed)
    ang = rs.uniform(0, 2 * np.pi, CAP)
    return np.stack([rs.uniform(4, 59, CAP), rs.uniform(4, 59, CAP), np.cos(ang), np.sin(ang)], 1)


def as_keylines(oracle, rows):
    kls = np.zeros(len(rows), oracle.KEYLINE_DTYPE)
    if len(rows):
        kls["c_p"] = rows[:, 0:2].astype(np.float32)
        kls["u_m"] = rows[:, 2:4].astype(np.float32)
        kls["n_m"] = 5.0
        kls["m_m"] = kls["u_m"] * kls["n_m"][:, None]
        kls["rho"], kls["s_rho"] = 1.0, 1.0
        px = np.clip(np.round(rows[:, 0]), 0, W - 1).astype(np.int64)
        py = np.clip(np.round(rows[:, 1]), 0, H - 1).astype(np.int64)
        kls["p_inx"] = py * W + px
    return kls


@pytest.fixture(scope="module")
def lists():
    oracle = require_ref()
    out = {}
    for r in RADII:
        rows, groups = crafted_list(r, 40 + r)
        assert 100 <= len(rows) <= CAP
        seqs = [as_keylines(oracle, rows), as_keylines(oracle, np.zeros((0, 4))), as_keylines(oracle, full_bin_list(7 + r))]
        fields = {}
        for kind in ("ref", "port"):
            orc = oracle.Oracle(kind, oracle.euroc_params(W, H, max_points=CAP))
            fs = []
            for kl in seqs:
                orc.set_keylines(0, kl, None, 0.0)
                orc.build_field(0, r, 0.0)
                fs.append(orc.field(0))
            fields[kind] = fs
        out[r] = dict(seqs=seqs, groups=groups, fields=fields)
    return out


def test_the_lists_hold_the_cases(lists):
    for r in RADII:
        c = lists[r]
        ref = c["fields"]["ref"]
        assert [len(k) for k in c["seqs"]] == [len(c["seqs"][0]), 0, CAP] and len(c["seqs"][0]) not in (0, CAP)
        assert (ref[1][..., 1] == -1).all()                                   # the empty sequence: an empty field
        for kind in ("ref", "port"):
            for a, b in zip(ref, c["fields"][kind]):
                assert np.array_equal(a[..., 1], b[..., 1])
        f = ref[0]
        # ties: of two identical KeyLines only the later one is in the field; the crossing pixel belongs to the later KeyLine at distance 0
        a, _ = c["groups"]["ties"]
        assert not (f[..., 1] == a).any() and f[30, 30, 1] == a + 2 and f[30, 30, 0] == 0
        assert f[50, 30, 1] == a + 4 and f[50, 30, 0] == 2                     # equal distance from both: the larger id
        # x = 63.5 is pixel 64: the horizontal KeyLine whose LAST sample (t = r - 1) sits there owns it unless a nearer one took it
        assert f[10, 64, 1] >= 0 and f[10, 63, 1] >= 0
        # every tile of the image is written, also the clipped ones
        for ys, xs in ((slice(0, 64), slice(0, 64)), (slice(0, 64), slice(64, W)), (slice(64, H), slice(0, 64)), (slice(64, H), slice(64, W))):
            assert (f[ys, xs, 1] >= 0).any()
        # every KeyLine of the full-bin sequence has its centre pixel in tile (0, 0)
        kl = c["seqs"][2]
        assert ((np.round(kl["c_p"]) >= 0) & (np.round(kl["c_p"]) < 64)).all()


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("debug", [1, 0], ids=["dist_and_ikl", "plane16"])
def test_build_field_ranges(lists, r, debug):
    """debug = 1: the {dist, ikl} field; debug = 0: the 16-bit KeyLine-index plane (download_field then reports dist = -1)."""
    c = lists[r]
    eh = edgehip.EdgeHip(edgehip.euroc_params(W, H, max_points=CAP, debug_planes=debug), nseq=3, nslots=2)
    try:
        for _ in range(2):            # twice: the second launch starts from the bin counts the first one left
            for s, kl in enumerate(c["seqs"]):
                eh.upload_keylines(s, 1, to_edgehip_kl(kl), None, 0.0)
            eh.build_field(1, r, 0.0)
            for s in range(3):
                got = eh.download_field(s)
                for kind in ("ref", "port"):
                    want = c["fields"][kind][s]
                    bad = np.argwhere(got[..., 1] != want[..., 1])
                    assert len(bad) == 0, (r, s, kind, "ikl differs at (y, x)", bad[:8].tolist())
                    m = want[..., 1] >= 0
                    if debug:
                        assert np.array_equal(got[..., 0][m], want[..., 0][m]), (r, s, kind, "dist differs")
                    else:
                        assert (got[..., 0][m] == -1).all()
    finally:
        eh.close()
