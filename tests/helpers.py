"""Shared helpers of the GPU parity tests."""
import numpy as np


def to_edgehip_kl(kl):
    """oracle KEYLINE_DTYPE and edgehip KEYLINE_DTYPE are the same 168-byte layout."""
    from rebvo_amd import edgehip
    return np.frombuffer(np.ascontiguousarray(kl).tobytes(), dtype=edgehip.KEYLINE_DTYPE).copy()


def oracle_pair(w, h, n_warm, seq="billboard", seed=None, traj_seed=None, frames=None, **over):
    """Run the reference oracle for n_warm full frames, then stage A of the next frame.

    seed / traj_seed: the scene's and the trajectory's seed (None = synth's defaults); frames: the n_warm + 1 frames themselves,
    in place of a synthetic sequence.  Returns (orc, slot_old, slot_new, nav_of_last_full_frame, frames)."""
    from oracle import oracle
    from rebvo_amd import synth
    orc = oracle.Oracle("ref", oracle.euroc_params(w, h, **over))
    if frames is not None:
        frames = list(frames)
        assert len(frames) == n_warm + 1
    elif seq == "billboard":
        kw = {k: v for k, v in (("seed", seed), ("traj_seed", traj_seed)) if v is not None}
        frames = [f for f, _, _ in synth.billboard_sequence(w, h, n_warm + 1, **kw)]
    else:
        kw = {} if seed is None else {"seed": seed}
        frames = list(synth.rects_sequence(w, h, n_warm + 1, **kw))
    nav = None
    for k in range(n_warm):
        _, nav = orc.process_frame(frames[k], 0.05 * k)
    slot_old = (n_warm - 1) % 8
    slot_new = n_warm % 8
    orc.stage_a(slot_new, frames[n_warm], nav.tresh, nav.kn)
    return orc, slot_old, slot_new, nav, frames


def inject_pair(eh, orc, slot_old, slot_new, seq=0, gslot_old=0, gslot_new=1):
    eh.upload_keylines(seq, gslot_old, to_edgehip_kl(orc.keylines(slot_old)), orc.mask(slot_old), orc.retuned(slot_old))
    eh.upload_keylines(seq, gslot_new, to_edgehip_kl(orc.keylines(slot_new)), orc.mask(slot_new), orc.retuned(slot_new))


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


from rebvo_amd.config import write_global_config  # noqa: E402,F401  (the writer lives with the package: bench.py uses it too)


def needs_experiments():
    """Tests of the alternative kernels that measured slower than the defaults (round 4 verdict, item 10): those kernels and their
    EDGEHIP_* switches exist only in a library built with `make -C rebvo_amd/csrc EXPERIMENTS=1` (edgehip_experiments() == 1)."""
    import pytest
    from rebvo_amd import edgehip
    if not edgehip.load_library().edgehip_experiments():
        pytest.skip("alternative kernel behind `make EXPERIMENTS=1`: not in the default build")


def require_ref():
    """GPU parity tests need oracle/_ref (the reference compiled in place; it travels to the GPU box prebuilt).  Its absence
    is a broken snapshot, not a reason to go green by skipping."""
    import pytest
    from oracle import oracle
    if not oracle.available("ref"):
        pytest.fail("oracle/_ref/libreforacle.so is missing: run `make -C oracle` where the reference tree is present (the GPU box "
                    "receives the prebuilt library with the snapshot)")
    return oracle


def tri(k, n):
    p = 2 * (n - 1)
    k = k % p
    return k if k < n else p - k


def hetero_sequence(s, w=752, h=480, scenes=6, pool=12):
    """Sequence `s` of bench.py's heterogeneous batch: scene s % 6 (its own texture and trajectory), started at phase
    (s // 6) of the scene's 12-frame pool.  Returns frame_of(k)."""
    from rebvo_amd import edgehip, synth
    p = edgehip.euroc_params(w, h)
    intr = dict(fx=float(p.zfx), fy=float(p.zfy), cx=float(p.ppx), cy=float(p.ppy))
    frames = [f for f, _, _ in synth.billboard_sequence(w, h, pool, seed=101 + 7 * (s % scenes), traj_seed=29 + (s % scenes), **intr)]
    ph = (s // scenes) % (2 * (pool - 1))
    return lambda k: frames[tri(k + ph, pool)]


def depths_agree(kg, kr, same):
    """Depth maps of the device (kg) and the reference (kr) on the KeyLines with identical matches: |d rho| <= 1e-5 |rho| + 1e-7 +
    1e-5 s_rho.  The last term: the EKF's gain for a KeyLine that knows nothing about its depth (s_rho of the order of rho or above) is
    close to 1 and its measurement divides by u . (V_xy zf - V_z q0) (edge_tracker.cpp:978-1003), small when the edge runs along the
    epipolar line — a velocity that differs by 1e-9 of the step moves such a depth by 1e-5 of its value and 1e-5 of its own sigma
    (one KeyLine of 16 000 at 1280 x 720, tools/experiments/exp_pipeline_closeness.py)."""
    d = np.abs(kg["rho"][same] - kr["rho"][same])
    return bool(np.all(d <= 1e-5 * np.abs(kr["rho"][same]) + 1e-7 + 1e-5 * kr["s_rho"][same]))


# ---- the donors of tests/test_whole_batch_vs_ref_gpu.py (preconditions: tests/test_whole_batch_donors_cpu.py) -------------------
# (name, scene, scene seed, trajectory seed, detector_thresh).  auto_gain = 0 keeps the threshold where it is put, so the reference's
# own detector yields lists from a few hundred KeyLines to the cap; the detector's settings reach neither side's stage B / C calls.
DONOR_SPECS = [
    ("bb11_t010", "billboard", 11, 13, 0.010),
    ("bb101_t003", "billboard", 101, 29, 0.003),     # dense: reaches the default cap at 752 x 480
    ("bb108_t170", "billboard", 108, 30, 0.170),     # sparse: about a thousand KeyLines at 752 x 480
    ("rects7_t020", "rects", 7, None, 0.020),
    ("bb115_t005", "billboard", 115, 31, 0.005),
    ("bb122_t180", "billboard", 122, 32, 0.180),     # a few hundred
    ("bb129_t002", "billboard", 129, 33, 0.002),
    ("bb108_t180", "billboard", 108, 30, 0.180),     # a few hundred
]
DEGENERATE_DONORS = ("blank_new", "blank_old", "scene_cut")
_donor_frames = {}


def _donor_sequence(w, h, scene, seed, traj_seed, n):
    from rebvo_amd import synth
    key = (w, h, scene, seed, traj_seed, n)
    if key not in _donor_frames:
        if scene == "billboard":
            _donor_frames[key] = [f for f, _, _ in synth.billboard_sequence(w, h, n, seed=seed, traj_seed=traj_seed)]
        else:
            _donor_frames[key] = list(synth.rects_sequence(w, h, n, seed=seed))
    return _donor_frames[key]


def whole_batch_donors(w, h, max_points, n_warm=3):
    """The donor states of the ragged-batch test: for each, the reference after n_warm full frames and stage A of the next one.
    Eight textured donors (DONOR_SPECS) and three degenerate ones: `blank_new` (the new frame is blank: kn = 0 in the new slot),
    `blank_old` (blank warm-up frames, then texture: the old list is empty) and `scene_cut` (old and new list from different
    scenes).  All share max_points.  Returns a list of dicts(name, orc, so, sn, nav, kn_old, kn_new)."""
    out = []
    common = dict(max_points=max_points, auto_gain=0.0, min_thresh=1e-4)
    specs = [(n, sc, sd, ts, th, None) for n, sc, sd, ts, th in DONOR_SPECS]
    a = _donor_sequence(w, h, "billboard", 11, 13, n_warm + 1)
    b = _donor_sequence(w, h, "billboard", 101, 29, n_warm + 1)
    blank = np.full_like(a[0], 40)
    specs += [("blank_new", None, None, None, 0.010, a[:n_warm] + [blank]),
              ("blank_old", None, None, None, 0.010, [blank] * n_warm + [a[n_warm]]),
              ("scene_cut", None, None, None, 0.010, a[:n_warm] + [b[n_warm]])]
    for name, scene, seed, traj_seed, thresh, frames in specs:
        if frames is None:
            frames = _donor_sequence(w, h, scene, seed, traj_seed, n_warm + 1)
        orc, so, sn, nav, _ = oracle_pair(w, h, n_warm, frames=frames, detector_thresh=thresh, **common)
        out.append(dict(name=name, orc=orc, so=so, sn=sn, nav=nav, kn_old=orc.kn(so), kn_new=orc.kn(sn)))
    return out


def deal_donors(donors, B, seed=7):
    """donor_of[s] for a batch of B sequences, fixed by `seed`: sequences 0, 63, 64 and B - 1 hold four different donors, each
    degenerate donor sits between two textured ones, every donor occurs at least three times."""
    names = [d["name"] for d in donors]
    full = [i for i, n in enumerate(names) if n not in DEGENERATE_DONORS]
    empty = [i for i, n in enumerate(names) if n in DEGENERATE_DONORS]
    rs = np.random.RandomState(seed)
    deal = np.array([full[k % len(full)] for k in rs.permutation(B)])      # every textured donor B // 8 times or more
    deal[[0, 63, 64, B - 1]] = full[:4]                                    # four different donors at the 64-sequence seam and the ends
    fixed = {0, 63, 64, B - 1}
    spots = [s for s in range(2, B - 2, 2) if not ({s - 1, s, s + 1} & fixed)]   # even positions: two of them are never neighbours
    for j, s in enumerate(rs.choice(spots, 3 * len(empty), replace=False)):
        deal[s] = empty[j % len(empty)]
    return deal


def check_donor_preconditions(donors, deal, cap, small_cap):
    """What the ragged batch needs of its donors and of the deal (asserted on the CPU, before anything runs on the device)."""
    names = [d["name"] for d in donors]
    by = dict(zip(names, donors))
    assert by["blank_new"]["kn_new"] == 0 and by["blank_new"]["kn_old"] > 0
    assert by["blank_old"]["kn_old"] == 0 and by["blank_old"]["kn_new"] > 0
    assert by["scene_cut"]["kn_old"] > 0 and by["scene_cut"]["kn_new"] > 0
    full = [d for d in donors if d["name"] not in DEGENERATE_DONORS]
    assert len(full) >= 8
    assert all(0 < d["kn_old"] <= cap and 0 < d["kn_new"] <= cap for d in full)
    kns = sorted(d["kn_old"] for d in full)
    assert kns[0] < 1200 and kns[-1] >= min(cap, 8000), kns            # from a few hundred KeyLines to the cap (or the densest scene)
    if small_cap:
        assert sum(d["kn_old"] == cap and d["kn_new"] == cap for d in full) >= 2, kns
        assert sum(0 < d["kn_old"] < cap // 4 and 0 < d["kn_new"] < cap // 4 for d in full) >= 2, kns
    B = len(deal)
    assert len({int(deal[s]) for s in (0, 63, 64, B - 1)}) == 4
    assert all(names[deal[s]] not in DEGENERATE_DONORS for s in (0, 63, 64, B - 1))
    for s in range(B):
        if names[deal[s]] in DEGENERATE_DONORS:
            assert 0 < s < B - 1 and names[deal[s - 1]] not in DEGENERATE_DONORS and names[deal[s + 1]] not in DEGENERATE_DONORS, s
    assert min(np.bincount(deal, minlength=len(donors))) >= 3


def skipped_keyline_pair(w=376, h=240, n_warm=4, frac=0.01, seed=3):
    """A donor pair whose old list has a seeded 1 % of KeyLines with s_rho = 0 and m_num = 0: with match_num_thresh = 2 and a
    FrameCount of 2 or more, TryVelRot skips them by match count (global_tracker.cpp:356), and a kernel that still divides such a
    KeyLine's zero row by its s_rho gets 0 / 0.  Returns (orc, slot_old, slot_new, nav, indices)."""
    orc, so, sn, nav, _ = oracle_pair(w, h, n_warm)
    kl = orc.keylines(so)
    idx = np.sort(np.random.RandomState(seed).choice(len(kl), max(1, int(len(kl) * frac)), replace=False))
    kl["s_rho"][idx] = 0.0
    kl["m_num"][idx] = 0
    orc.set_keylines(so, kl, orc.mask(so), orc.retuned(so))
    return orc, so, sn, nav, idx


_hetero_pools = {}


def hetero_batch(B, w=752, h=480, scenes=6, pool=12):
    """The frames of sequences 0 .. B - 1 of bench.py's heterogeneous batch (hetero_sequence(s) for every s) from ONE pool per scene:
    returns frame_of(k) -> uint8 [B, h, w, 3]."""
    from rebvo_amd import edgehip, synth
    key = (w, h, scenes, pool)
    if key not in _hetero_pools:
        p = edgehip.euroc_params(w, h)
        intr = dict(fx=float(p.zfx), fy=float(p.zfy), cx=float(p.ppx), cy=float(p.ppy))
        _hetero_pools[key] = np.stack([np.stack([f for f, _, _ in synth.billboard_sequence(w, h, pool, seed=101 + 7 * c, traj_seed=29 + c, **intr)])
                                       for c in range(scenes)])
    frames = _hetero_pools[key]
    s = np.arange(B)
    scene, ph = s % scenes, (s // scenes) % (2 * (pool - 1))
    return lambda k: frames[scene, [tri(k + int(q), pool) for q in ph]]
