"""GPU: stage A on the crafted images of tests/stage_a_crafted.py against the compiled reference, bit for bit.

What tests/test_stage_a_crafted_cpu.py shows to be present in the set — pixels exactly on each gate's threshold, NaN and half-pixel
offsets, exact-zero DoG values inside fitted windows, successors claimed by several KeyLines, zero gradient components, every
NextPoint probe, cuts on the first / a middle / the last KeyLine, the three clamp states — runs here through the three detector
paths (EDGEHIP_LEVEL_MODE 0: k_detect behind the multi-pass levels, 2: behind k_level, 3: k_stage_a_fused, the latter also in
its instantiation without debug planes).  Every parameter set runs its images as one batch in a seeded shuffled order, and three
of them alone.  Floats are compared through their bytes: -0 and +0 are different results here.

reTunedThresh is compared wherever kn > 0, max_dog == min_dog included: there the reference converts a NaN to int, but clamps the
index into the histogram whatever comes out and returns max_dog - i * 0 / n = max_dog for every i (edge_finder.cpp:392-403), so
its value does not hang on the conversion.  Out of domain and not run: dog_thresh = 0 (a NaN KeyLine indexes the mask in
join_edges), and reTunedThresh at kn == 0 (edge_finder.cpp:376 reads kl[0] of an empty list)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from rebvo_amd import edgehip
import stage_a_crafted as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (EDGEHIP_LEVEL_MODE, debug planes)
PATHS = [("0", True), ("2", True), ("3", True), ("3", False)]
PATH_IDS = ["multipass", "k_level", "fused", "fused_noplanes"]


def _need_ref():
    from oracle import oracle
    if not oracle.available("ref"):
        pytest.fail("oracle/_ref/libreforacle.so not built" " — a broken snapshot, not a reason to skip: run __graft_entry__.build(), where the reference tree is present")


def _same(eh, seq, slot, ref, planes, what):
    kl, mask = eh.download_keylines(seq, slot)
    st = eh.get_state(seq)
    assert len(kl) == ref["kn"], f"{what}: kn {len(kl)} vs {ref['kn']}"
    assert st.tresh == ref["tresh"] and st.l_kl_num == ref["lkl"], f"{what}: threshold state {st.tresh}, {st.l_kl_num} vs {ref['tresh']}, {ref['lkl']}"
    if planes:
        for name in ("img0", "img1", "dog"):
            assert eh.download_plane(seq, name).tobytes() == ref["planes"][name].tobytes(), f"{what}: plane {name}"
        for name in ("dx", "dy"):
            a, b = eh.download_plane(seq, name)[2:-2, 2:-2], ref["planes"][name][2:-2, 2:-2]
            assert a.tobytes() == b.tobytes(), f"{what}: plane {name}"
    if not np.array_equal(mask, ref["mask"]):
        d = np.argwhere(mask != ref["mask"])
        pytest.fail(f"{what}: img_mask_kl differs at {len(d)} pixels, first (y, x) = {d[0].tolist()}: {mask[tuple(d[0])]} vs {ref['mask'][tuple(d[0])]}")
    for fld in sc.STAGE_A_FIELDS:
        if kl[fld].tobytes() != ref["kl"][fld].tobytes():
            a, b = (np.ascontiguousarray(v[fld]).reshape(len(kl), -1) for v in (kl, ref["kl"]))
            i = int(np.nonzero((a.view(np.uint8) != b.view(np.uint8)).any(1))[0][0])
            pytest.fail(f"{what}: KeyLine.{fld} differs, first at {i} (pixel {int(ref['kl']['p_inx'][i])}): {a[i]} vs {b[i]}")
    if ref["kn"] > 0:
        assert np.float32(st.retuned_thresh).tobytes() == np.float32(ref["retuned"]).tobytes(), f"{what}: reTunedThresh"


def _ctx(over, nseq, planes, **more):
    return edgehip.EdgeHip(edgehip.euroc_params(sc.W, sc.H, debug_planes=1 if planes else 0, **over, **more), nseq=nseq, nslots=2)


@pytest.mark.parametrize("mode,planes", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("group", sc.GROUPS)
def test_crafted_images_bit_exact(group, mode, planes, monkeypatch):
    _need_ref()
    monkeypatch.setenv("EDGEHIP_LEVEL_MODE", mode)
    ims = sc.images()
    for label, over, names in sc.param_sets(group):
        rng = np.random.default_rng(len(label) + len(names))
        order = [names[i] for i in rng.permutation(len(names))]
        eh = _ctx(over, len(order), planes)
        eh.upload_rgb(0, np.stack([ims[n] for n in order]))
        eh.stage_a(0)
        for s, n in enumerate(order):
            _same(eh, s, 0, sc.ref_case(over, n), planes, f"{label} {n} (sequence {s} of {len(order)})")
        eh.close()
        eh = _ctx(over, 1, planes)
        for k, n in enumerate(order[:3]):    # alone (auto_gain = 0: nothing carries over from the frame before)
            eh.upload_rgb(k % 2, ims[n])
            eh.stage_a(k % 2)
            _same(eh, 0, k % 2, sc.ref_case(over, n), planes, f"{label} {n} (alone)")
        eh.close()


@pytest.mark.parametrize("nseq", [1, len(sc.IMAGE_NAMES)])
def test_each_mode_runs_its_own_kernels_at_this_size(nseq, monkeypatch):
    """The three modes are three code paths at 104 x 50 and these batch sizes, not one path under three names: mode 0 is k_detect
    behind the multi-pass levels (neither dispatch threshold of the auto mode is reached), 2 is k_detect behind k_level, 3 the
    one-kernel stage A (it would quietly fall back if the size did not suit it)."""
    want = {"0": dict(detect=True, level=False, fused=False, avg=True), "2": dict(detect=True, level=True, fused=False, avg=False),
            "3": dict(detect=False, level=False, fused=True, avg=False)}
    frames = np.stack([sc.images()[n] for n in sc.IMAGE_NAMES[:nseq]])
    for mode, w in want.items():
        monkeypatch.setenv("EDGEHIP_LEVEL_MODE", mode)
        eh = _ctx(sc.BASE, nseq, True)
        eh.profile_enable(True)
        eh.upload_rgb(0, frames)
        eh.stage_a(0)
        calls = {k: v[1] for k, v in eh.profile_read().items()}
        eh.close()
        got = dict(detect=calls["A.detect"] > 0, level=calls["A.level"] > 0, fused=calls["A.fused"] > 0, avg=calls["A.avg_rowscan"] > 0)
        assert got == w, (mode, calls)


@pytest.mark.parametrize("mode", ["0", "3"], ids=["multipass", "fused"])
@pytest.mark.parametrize("name", sorted(sc.sequences()))
def test_threshold_law_sequences(name, mode, monkeypatch):
    """auto_gain > 0, frame after frame in one context: the threshold on max_thresh, on min_thresh, strictly inside, held on a
    clamp for two frames, and l_kl_num through 0 (which of these each sequence holds is asserted in the CPU test)."""
    _need_ref()
    monkeypatch.setenv("EDGEHIP_LEVEL_MODE", mode)
    over, frames = sc.sequences()[name]
    ref = sc.run_oracle("ref", over, frames)
    eh = _ctx(over, 1, True)
    for k, f in enumerate(frames):
        eh.upload_rgb(k % 2, f)
        eh.stage_a(k % 2)
        _same(eh, 0, k % 2, ref[k], True, f"{name} frame {k}")
    eh.close()


WINDOW_IMAGES = ["vstep_up", "vstep_down", "hstep_up", "hstep_down", "diag_up", "diag_down", "anti_up", "anti_down", "checker4",
                 "ramp_h", "ramp_v", "ramp_d"]


@pytest.mark.parametrize("pos_neg", [0.4, 1.0])
@pytest.mark.parametrize("ws", [1, 3])
def test_other_plane_fit_windows(tmp_path, ws, pos_neg, monkeypatch):
    """DetectorPlaneFitSize 1 and 3 (3x3 and 7x7 windows; the scanned area and the sign count change with them).  The reference
    runs in a process of its own per window: it caches the pseudo inverse of the first window size it sees."""
    _need_ref()
    monkeypatch.setenv("EDGEHIP_LEVEL_MODE", "0")
    over = dict(sc.BASE, plane_fit_size=ws, pos_neg_thresh=pos_neg)
    frames = [sc.images()[n] for n in WINDOW_IMAGES]
    inp, outp = tmp_path / "in.npz", tmp_path / "out.npz"
    np.savez(inp, frames=np.stack(frames), w=sc.W, h=sc.H, over=json.dumps(over))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stage_a_ref_runner.py"), str(inp), str(outp)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = np.load(outp)
    eh = _ctx(over, len(frames), True)
    eh.upload_rgb(0, np.stack(frames))
    eh.stage_a(0)
    total = 0
    for k, n in enumerate(WINDOW_IMAGES):
        kl, mask = eh.download_keylines(k, 0)
        st = eh.get_state(k)
        kn = int(ref[f"kn_{k}"])
        assert len(kl) == kn, (n, len(kl), kn)
        assert st.tresh == float(ref[f"tresh_{k}"]) and st.l_kl_num == int(ref[f"lkl_{k}"]), n
        assert eh.download_plane(k, "dog").tobytes() == ref[f"dog_{k}"].tobytes(), n
        assert np.array_equal(mask, ref[f"mask_{k}"]), f"{n}: img_mask_kl differs"
        for fld in sc.STAGE_A_FIELDS:
            assert kl[fld].tobytes() == ref[f"kl_{k}"][fld].tobytes(), f"{n}: KeyLine.{fld} differs"
        if kn > 0:
            assert np.float32(st.retuned_thresh).tobytes() == np.float32(ref[f"retuned_{k}"]).tobytes(), n
        total += kn
    eh.close()
    assert total > 1000
