"""Shared helpers of the GPU parity tests."""
import numpy as np


def to_edgehip_kl(kl):
    """oracle KEYLINE_DTYPE and edgehip KEYLINE_DTYPE are the same 168-byte layout."""
    from rebvo_amd import edgehip
    return np.ascontiguousarray(kl).view(edgehip.KEYLINE_DTYPE).copy()          # (a view: an empty list stays a list)


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


# ---- crafted KeyLine lists for the mapping kernels (tests/test_mapping_crafted_cpu.py, tests/test_mapping_crafted_gpu.py) --------
RHO_MAX, RHO_MIN, RHO_INIT = 20.0, 1e-3, 1.0                      # edge_finder.h:38-40
MAPPING_LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 12287, 12288, 12289, 16383, 16384, 16385)
RESCALE_REGIONS = ((0, 12288), (12288, 16384), (16384, 1 << 30))  # k_rescale<512,12,4>: registers, LDS, streamed
MAPPING_STAGES = ("regularize", "ekf_raw", "ekf", "regularize_ekf", "rescale", "rescale_div", "rescale_after_ekf")
EKF_ARGS = (1e-4, 1.6968e-04, 1.0)                                # ReshapeQAbsolute, ReshapeQRelative, LocationUncertainty


def so3_exp(w):
    """exp of a rotation vector (Rodrigues), as the stage C tests build the rotation of rotate_keylines."""
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-9:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def cut_list(kl, mask, n):
    """The first n KeyLines of a list as a list of its own: neighbours beyond the cut become -1, match ids (indices into the OLD
    list, of which the mapping stages read the sign only) are folded into [0, n), the mask forgets the KeyLines that left."""
    k = kl[:n].copy()
    for f in ("n_id", "p_id"):
        k[f][k[f] >= n] = -1
    k["m_id"] = np.where(k["m_id"] >= 0, k["m_id"] % n, -1)
    m = mask.copy()
    m[m >= n] = -1
    return k, m


def indices_inside(kl):
    n = len(kl)
    return all(bool(np.all((kl[f] == -1) | ((kl[f] >= 0) & (kl[f] < n)))) for f in ("n_id", "p_id", "m_id"))


def _tile_list(kl, n):
    """kl repeated up to n KeyLines, the neighbour indices of every copy re-based into that copy (-1 where the copy is cut)."""
    parts, k0 = [], len(kl)
    for base in range(0, n, k0):
        c = kl[:min(k0, n - base)].copy()
        for f in ("n_id", "p_id"):
            c[f] = np.where((c[f] >= 0) & (c[f] < len(c)), c[f] + base, -1)
        parts.append(c)
    return np.concatenate(parts)


def _set_gradient(kl, idx, mx, my, n_m):
    """m_m, n_m as given (n_m is a stored field: Regularize_1_iter divides by it as it stands) and u_m = m_m / |m_m| in float."""
    mx, my = np.broadcast_to(np.float32(mx), idx.shape), np.broadcast_to(np.float32(my), idx.shape)
    kl["m_m"][idx] = np.stack([mx, my], 1)
    nn = np.sqrt(mx * mx + my * my, dtype=np.float32)
    with np.errstate(all="ignore"):
        kl["u_m"][idx] = np.stack([mx / nn, my / nn], 1)
    kl["n_m"][idx] = np.float32(n_m)


def _ekf_update(kl, i, V, zf, s_rho):
    """(rho, v_rho) of UpdateInverseDepthKalmanARLU before its limits (edge_tracker.cpp:982-1028) for the KeyLines i with s_rho as
    given: the same expressions in the same order, one rounding each (numpy's element-wise operations do not fuse)."""
    q, q0 = kl["p_m"][i].astype(np.float64), kl["p_m_0"][i].astype(np.float64)
    rho = kl["rho"][i]
    with np.errstate(all="ignore"):
        v_rho = s_rho * s_rho
        ux, uy = kl["m_m0"][i, 0].astype(np.float64) / kl["n_m0"][i], kl["m_m0"][i, 1].astype(np.float64) / kl["n_m0"][i]
        Y = ux * (q[:, 0] - q0[:, 0]) + uy * (q[:, 1] - q0[:, 1])
        H = ux * (V[0] * zf - V[2] * q0[:, 0]) + uy * (V[1] * zf - V[2] * q0[:, 1])
        rho_p = 1 / (1.0 / rho + V[2])
        F = 1 / (1 + rho * V[2])
        F = F * F
        p_p = F * v_rho * F + EKF_ARGS[0] * EKF_ARGS[0]
        e = Y - H * rho_p
        S = H * p_p * H + EKF_ARGS[2] * EKF_ARGS[2]
        K = p_p * H * (1 / S)
        return rho_p + K * e, (1 - K * H) * p_p


def crafted_mapping_lists(w, h, cap, seed=5, per_edit=100):
    """Crafted inputs of Regularize_1_iter, UpdateInverseDepthKalman and EstimateReScalingOpt.  The base is the reference's own new-slot
    list after Minimizer_RV, FordwardMatch, rotate_keylines and directed_matching on the billboard scene (the recipe of
    test_stage_c_chain) with max_points = cap, tiled up to cap KeyLines where the detector gives fewer.  Every variant edits disjoint
    fixed-seed subsets of it; mask and retuned value stay.  No index field ever leaves [-1, kn).

    Returns dict(orc, slot, V, RVel, RW0, mask, retuned, kn, variants = {name: KeyLines}, edits = {name: {edit: indices}}).
    `edits` of "regularize" holds the CENTRE KeyLines: the edited fields are mostly their neighbours'."""
    orc, so, sn, nav, _ = oracle_pair(w, h, 4, max_points=cap)
    q = orc.quantile(so)
    orc.build_field(sn, 40, orc.retuned(sn))
    res = orc.minimizer_rv(sn, so, nav.V[:], nav.W[:], 0.5, 5, 2, 2.0, q, 0, 2)
    V, RVel, RW0 = res["V"], res["RVel"], res["RW0"]
    orc.forward_match(so, sn)
    R0 = so3_exp(res["W"])
    orc.rotate_keylines(so, R0)
    orc.directed_matching(sn, so, V, RVel, R0.T, 1.0, 45.0, 40.0, 2.0)
    mask, retuned = orc.mask(sn), orc.retuned(sn)
    base = orc.keylines(sn)
    kn = cap if w >= 752 else len(base)            # the small image keeps the detector's own length
    base = _tile_list(base, kn)
    base["m_id"] = np.where(base["m_id"] >= 0, base["m_id"] % kn, -1)
    mask[mask >= kn] = -1
    rs = np.random.RandomState(seed)
    S = per_edit
    variants, edits = {"plain": base.copy()}, {"plain": {}}
    nextf = lambda a, b: np.nextafter(np.float64(a), np.float64(b))

    # ---- EKF ----
    kl = base.copy()
    matched = np.nonzero(kl["m_id"] >= 0)[0]
    names = ("rho_max", "rho_min", "n_m0_zero", "rho_pole", "rho_zero", "nan", "s_rho_inf", "at_max", "at_min", "huge_s_rho_max",
             "huge_s_rho_min")
    size = [2 * S if n.startswith("huge") else S for n in names]
    at = np.concatenate([[0], np.cumsum(size)])
    assert len(matched) >= at[-1], (len(matched), S)
    pick = rs.permutation(matched)
    e = {n: np.sort(pick[at[j]:at[j + 1]]) for j, n in enumerate(names)}
    # a quarter of every edit loses its match: the quarter is taken from the permutation, so it is spread over the whole list and
    # every cut length holds its share
    un = np.sort(np.concatenate([pick[at[j]:at[j + 1]][:size[j] // 4] for j in range(len(names))]))
    zf = float((np.float32(orc.p.zfx) + np.float32(orc.p.zfy)) / np.float32(2))       # cam_model keeps the focal lengths as floats
    # huge_s_rho_*: the same displacements on KeyLines with an s_rho of 1e12 to 2e12.  There K * H rounds to 1 or to a double next to
    # it; where it rounds above 1, v_rho is negative and s_rho = sqrt(v_rho) is NaN while rho is finite and beyond a limit: only the
    # ORDER of the else-if chain (edge_tracker.cpp:1035-1048) decides between the clamp (s_rho stays NaN) and the reset.  Which s_rho
    # rounds that way is found per KeyLine with the update's own arithmetic (_ekf_update) among 512 candidates.
    for n, sign in (("rho_max", 1.0), ("rho_min", -1.0), ("huge_s_rho_max", 1.0), ("huge_s_rho_min", -1.0)):
        i = e[n]
        u = kl["m_m0"][i].astype(np.float64) / kl["n_m0"][i][:, None]
        q0 = kl["p_m_0"][i].astype(np.float64)
        H = u[:, 0] * (V[0] * zf - V[2] * q0[:, 0]) + u[:, 1] * (V[1] * zf - V[2] * q0[:, 1])
        d = sign * np.where(H < 0, -1.0, 1.0) * rs.uniform(500, 5000, len(i))     # Y / H far beyond RHO_MAX, or far below 0
        kl["p_m"][i] = (q0 + d[:, None] * u).astype(np.float32)
    for n in ("huge_s_rho_max", "huge_s_rho_min"):
        i = e[n]
        s = np.full(len(i), 1e12)
        found = np.zeros(len(i), bool)
        for k in range(512):
            cand = 1e12 * (1 + k / 512.0)
            rho_c, v_c = _ekf_update(kl, i, V, zf, cand)
            hit = ~found & (v_c < 0) & np.isfinite(rho_c) & ((rho_c < RHO_MIN) | (rho_c > RHO_MAX))
            s[hit], found = cand, found | hit
        kl["s_rho"][i] = s
    kl["n_m0"][e["n_m0_zero"]] = 0.0
    lo = hi = -1.0 / V[2]                                                        # the doubles around -1 / V[2]: one of them has
    cand = [lo]                                                                  # 1 / rho + V[2] == 0, the prediction's pole
    for _ in range(16):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cand += [lo, hi]
    pole = [c for c in cand if 1.0 / c + V[2] == 0]
    assert pole, "no double rho with 1 / rho + V[2] == 0"
    kl["rho"][e["rho_pole"]] = pole[0]
    kl["rho"][e["rho_zero"]] = 0.0
    kl["rho"][e["nan"]], kl["s_rho"][e["nan"]] = np.nan, np.nan
    kl["s_rho"][e["s_rho_inf"]] = np.inf
    kl["rho"][e["at_max"]], kl["s_rho"][e["at_max"]] = RHO_MAX, RHO_MAX
    kl["rho"][e["at_min"]], kl["s_rho"][e["at_min"]] = RHO_MIN, RHO_MIN
    kl["m_id"][un] = -1
    kl["rho0"][un], kl["s_rho0"][un] = rs.uniform(0.1, 9.0, len(un)), rs.uniform(0.1, 9.0, len(un))
    e["unmatched"] = un
    variants["ekf"], edits["ekf"] = kl, e

    # ---- regularize: centres whose (centre, next, previous) triples are disjoint ----
    kl = base.copy()
    ar = np.arange(kn)
    ok = (kl["n_id"] >= 0) & (kl["p_id"] >= 0) & (kl["n_id"] != kl["p_id"]) & (kl["n_id"] != ar) & (kl["p_id"] != ar)
    names = ("nb_n_m_zero_n", "nb_n_m_zero_p", "nb_alpha_nan", "no_next", "no_prev", "next_is_prev", "next_is_self", "prev_is_self",
             "gate_on", "gate_above", "gate_below", "alpha_on", "alpha_below", "alpha_above", "alpha_one", "nb_s_rho_zero", "own_s_rho_zero")
    Sr = min(S, 64)
    used, centres = np.zeros(kn, bool), []
    for i in rs.permutation(np.nonzero(ok)[0]):
        t = [i, kl["n_id"][i], kl["p_id"][i]]
        if not used[t].any():
            used[t] = True
            centres.append(i)
            if len(centres) == Sr * len(names):
                break
    assert len(centres) == Sr * len(names), len(centres)
    centres = np.array(centres)
    e = {n: np.sort(centres[j * Sr:(j + 1) * Sr]) for j, n in enumerate(names)}
    N, P = (lambda n: kl["n_id"][e[n]]), (lambda n: kl["p_id"][e[n]])
    kl["n_m"][N("nb_n_m_zero_n")] = 0
    kl["n_m"][P("nb_n_m_zero_p")] = 0
    for n in ("nb_n_m_zero_n", "nb_n_m_zero_p"):                                 # (inside the depth gate, so that alpha is reached)
        for j in (N(n), P(n)):
            kl["rho"][j], kl["s_rho"][j] = 1.0, 0.5
    _set_gradient(kl, N("nb_alpha_nan"), 0, 0, 0)                                # 0 / 0
    for j in (N("nb_alpha_nan"), P("nb_alpha_nan")):                             # (inside the depth gate, so that alpha is reached)
        kl["rho"][j], kl["s_rho"][j] = 1.0, 0.5
    kl["n_id"][e["no_next"]] = -1
    kl["p_id"][e["no_prev"]] = -1
    kl["n_id"][e["next_is_prev"]] = kl["p_id"][e["next_is_prev"]]
    kl["rho"][P("next_is_self")] = kl["rho"][e["next_is_self"]]                  # (d = 0 and both s_rho > 0: inside the depth gate)
    kl["rho"][N("prev_is_self")] = kl["rho"][e["prev_is_self"]]
    for n, other in (("next_is_self", P), ("prev_is_self", N)):
        assert np.all(kl["s_rho"][e[n]] > 0) and np.all(kl["s_rho"][other(n)] > 0)
    kl["n_id"][e["next_is_self"]] = e["next_is_self"]
    kl["p_id"][e["prev_is_self"]] = e["prev_is_self"]
    # the depth gate d^2 > s_n^2 + s_p^2 (edge_tracker.cpp:106) on Pythagorean triples scaled by powers of two: every product exact
    for n in ("gate_on", "gate_above", "gate_below"):
        c = e[n]
        a, b, hyp = np.array([(3, 4, 5), (5, 12, 13), (8, 15, 17)], np.float64)[rs.randint(0, 3, len(c))].T
        sc = 2.0 ** rs.randint(-7, -3, len(c))
        rho_p = 1.0 + rs.randint(0, 8, len(c)) / 8.0
        rho_n = rho_p + hyp * sc
        assert np.all(rho_n - rho_p == hyp * sc)
        if n != "gate_on":
            rho_n = np.nextafter(rho_n, np.inf if n == "gate_above" else -np.inf)
        kl["rho"][P(n)], kl["rho"][N(n)] = rho_p, rho_n
        kl["s_rho"][P(n)], kl["s_rho"][N(n)] = a * sc, b * sc
        _set_gradient(kl, N(n), 3, 4, 5)
        _set_gradient(kl, P(n), 3, 4, 5)
    # alpha = thresh = 0.5 as a float quotient: (x * 1 + 0 * 0) / (1 * 2) with x = 1 and its float neighbours
    for n, x in (("alpha_on", np.float32(1)), ("alpha_below", np.nextafter(np.float32(1), np.float32(0))),
                 ("alpha_above", np.nextafter(np.float32(1), np.float32(2)))):
        _set_gradient(kl, N(n), 1, 0, 1)
        _set_gradient(kl, P(n), x, 0, 2)
        for j in (N(n), P(n)):
            kl["rho"][j], kl["s_rho"][j] = 1.0, 0.5
    # at alpha == thresh the weights wrn and wrp are 0 and a regularized KeyLine would equal a skipped one within an ulp.  With an own
    # s_rho of 0, wr is infinite: regularized is NaN (inf / inf), skipped keeps its bits, so "on" and "below" show in rho and s_rho.
    kl["s_rho"][e["alpha_on"]] = kl["s_rho"][e["alpha_below"]] = 0.0
    _set_gradient(kl, N("alpha_one"), 3, 4, 5)
    _set_gradient(kl, P("alpha_one"), 3, 4, 5)
    # a neighbour's s_rho = 0 is reached behind the depth gate and alpha: equal depths (d = 0) and equal gradients (alpha = 1), so
    # wrn = alpha / 0 is infinite for every one of them and the regularized values are inf / inf
    _set_gradient(kl, N("nb_s_rho_zero"), 3, 4, 5)
    _set_gradient(kl, P("nb_s_rho_zero"), 3, 4, 5)
    kl["rho"][N("nb_s_rho_zero")] = kl["rho"][P("nb_s_rho_zero")]
    assert np.all(kl["s_rho"][P("nb_s_rho_zero")] > 0)
    kl["s_rho"][N("nb_s_rho_zero")] = 0.0
    kl["s_rho"][e["own_s_rho_zero"]] = 0.0
    variants["regularize"], edits["regularize"] = kl, e

    # ---- rescale: on the list as the reference's own regularize + EKF leave it; edits in each of the kernel's storage regions ----
    orc.set_keylines(sn, base, mask, retuned)
    orc.regularize(sn, 0.5)
    orc.ekf(sn, V, RVel, RW0, *EKF_ARGS)
    mapped = orc.keylines(sn)
    kl = mapped.copy()
    rejected, counted = ("s_rho0_zero", "s_rho0_neg", "s_rho0_negzero", "s_rho_above", "m_num_zero"), ("s_rho_at", "s_rho_below", "m_num_neg")
    e = {n: [] for n in rejected + counted}
    Sq = 64
    for lo, hi in RESCALE_REGIONS:
        hi = min(hi, kn)
        if hi - lo < 4 * Sq * len(e):
            continue
        pick = lo + rs.permutation(hi - lo)[:Sq * len(e)]
        for j, n in enumerate(e):
            e[n].append(pick[j * Sq:(j + 1) * Sq])
    e = {n: np.sort(np.concatenate(v)) for n, v in e.items()}
    every = np.concatenate(list(e.values()))
    kl["s_rho0"][every], kl["s_rho"][every], kl["m_num"][every] = rs.uniform(0.2, 2, len(every)), rs.uniform(0.2, 2, len(every)), 3
    kl["rho"][every], kl["rho0"][every] = rs.uniform(0.2, 3, len(every)), rs.uniform(0.2, 3, len(every))
    kl["s_rho0"][e["s_rho0_zero"]] = 0.0
    kl["s_rho0"][e["s_rho0_neg"]] = -0.5
    kl["s_rho0"][e["s_rho0_negzero"]] = -0.0
    kl["s_rho"][e["s_rho_above"]] = nextf(RHO_MAX, np.inf)
    kl["m_num"][e["m_num_zero"]] = 0
    kl["s_rho"][e["s_rho_at"]] = RHO_MAX
    kl["s_rho"][e["s_rho_below"]] = nextf(RHO_MAX, 0)
    kl["m_num"][e["m_num_neg"]] = -1                                             # compared as unsigned (edge_tracker.cpp:1119): counts
    variants["rescale"], edits["rescale"] = kl, e
    kl = mapped.copy()                                                           # nothing counts: rTr0 = 0, Kp = 1, RKp = inf
    kl["m_num"][ar % 4 == 0] = 0
    kl["s_rho0"][ar % 4 == 1] = 0.0
    kl["s_rho0"][ar % 4 == 2] = -0.0
    kl["s_rho"][ar % 4 == 3] = nextf(RHO_MAX, np.inf)
    variants["rescale_none"], edits["rescale_none"] = kl, {}
    assert all(indices_inside(v) for v in variants.values())
    return dict(orc=orc, slot=sn, V=V, RVel=RVel, RW0=RW0, mask=mask, retuned=retuned, kn=kn, variants=variants, edits=edits)


def mapping_lengths(kn):
    return [n for n in MAPPING_LENGTHS if n < kn] + [kn]


def mapping_stages(orc, slot, kl, mask, retuned, V, RVel, RW0):
    """Every mapping stage through one oracle (reference or port), each from the injected state.  Returns {stage: dict(input, kl, Kp,
    RKp, r_num)}: `input` is what the stage starts from, `kl` the list after it."""
    out = {}

    def run(stage, start, reg=False, ekf=False, rescale=None):
        orc.set_keylines(slot, start, mask, retuned)
        o = dict(input=start)
        if reg:
            o["r_num"] = orc.regularize(slot, 0.5)
        if ekf:
            orc.ekf(slot, V, RVel, RW0, *EKF_ARGS)
        if rescale is not None:
            o["Kp"], o["RKp"] = orc.rescale(slot, RHO_MAX, 1, rescale)
        o["kl"] = orc.keylines(slot)
        out[stage] = o

    run("regularize", kl, reg=True)
    run("ekf_raw", kl, ekf=True)
    run("ekf", out["regularize"]["kl"], ekf=True)
    run("regularize_ekf", kl, reg=True, ekf=True)
    run("rescale", kl, rescale=False)
    run("rescale_div", kl, rescale=True)
    run("rescale_after_ekf", out["regularize_ekf"]["kl"], rescale=False)
    return out


DEPTH_FIELDS = ("rho", "s_rho", "rho0", "s_rho0")


def depth_state_mismatches(got, want):
    """rho, s_rho, rho0, s_rho0 of EVERY KeyLine within rtol 1e-12 (atol 0, NaN equals NaN), and the branch outcomes as sets: the
    KeyLines at RHO_MAX, at RHO_MIN, reset to (RhoInit, RHO_MAX) and NaN must be the same KeyLines."""
    if len(got) != len(want):
        return [f"list length {len(got)} vs {len(want)}"]
    bad = []
    for f in DEPTH_FIELDS:
        ok = np.isclose(got[f], want[f], rtol=1e-12, atol=0, equal_nan=True)
        if not ok.all():
            i = np.nonzero(~ok)[0]
            bad.append(f"KeyLine.{f}: {len(i)} differ, first {i[:4]}: {got[f][i[:4]]} vs {want[f][i[:4]]}")
    sets = (("rho == RHO_MAX", lambda k: k["rho"] == RHO_MAX), ("rho == RHO_MIN", lambda k: k["rho"] == RHO_MIN),
            ("(rho, s_rho) == (1, 20)", lambda k: (k["rho"] == RHO_INIT) & (k["s_rho"] == RHO_MAX)),
            ("rho NaN", lambda k: np.isnan(k["rho"])), ("s_rho NaN", lambda k: np.isnan(k["s_rho"])))
    for name, f in sets:
        a, b = f(got), f(want)
        if not np.array_equal(a, b):
            bad.append(f"set {name}: {a.sum()} vs {b.sum()} KeyLines, first difference at {np.nonzero(a != b)[0][:4]}")
    return bad


def scalar_close(got, want, rel=1e-10):
    """_close_or_both_nonfinite of the ragged-batch test for Kp / P_Kp."""
    got, want = float(got), float(want)
    if np.isfinite(want) != np.isfinite(got):
        return False
    return (not np.isfinite(want)) or abs(got - want) <= rel * abs(want)
