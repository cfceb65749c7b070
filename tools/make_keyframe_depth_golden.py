#!/usr/bin/env python3
"""Generate tests/golden/keyframe_depth/*.npz from the REFERENCE's own kfvo::mapKFUsingIDK, translateDepth_F2KF, translateDepth_KF2F and
translateDepth_New2Old.

Build machine only (needs the reference tree and oracle/_ref/libreforacle.so from `make -C oracle`):
    python tools/make_keyframe_depth_golden.py --ref /path/to/reference

tools/keyframe_depth_ref_driver.cpp is compiled into a temporary directory outside the repository, with the reference's kfvo.cpp included
(nothing is written under oracle/ or into the repository).  One departure from "in place": the file's helpers isnan(double&) /
isinf(double&) call themselves under a current libstdc++, so the driver includes a copy made in that temporary directory in which the two
calls name std::isnan / std::isinf (build_driver).  A fixture holds, per KeyLine, only the numbers the rules read
or write (p_m, u_m as float32; rho, s_rho as float64; m_num; the link), the poses, the arguments, the reference's outputs and its seconds.
NOTHING IS WRITTEN unless, for every case, the plain-numpy port (tests/keyframe_depth_port.py) equals the reference bit for bit on every
rho / s_rho (NaN as a class), exactly on every m_num, count and K, and the reference left every other byte of its records alone.  rTr and
rTr0 are locals of optimizeScaleBack: the fixture's are the port's, tied to the reference through K = rTr / rTr0 (port and reference sum
in the same order).  Every written list is recorded as a digest (tests/keyframe_depth_port.py: digest), and as arrays where the size
allows: everywhere in crafted.npz, for the optim_scale cases (which a device compares by tolerance) in chained.npz.

  crafted.npz   70x50, lists of 0, 1, 5, 65, 257, 600 and 1030 KeyLines: the frame list is the key-frame list moved by a known pose with 0.3 px
                of noise, 20 % of the links dropped in each direction; the four large pairs are the compared ones (at least half of their
                linked KeyLines leave mapKLUsingIDK through no clamp).  Further pairs of 65, inputs with recorded outputs: a NaN rho on a
                linked KeyLine, a half turn about y (s_rho < 0), a quarter turn about y with p_m = (0, 0) (rotateQs returns zeros), every
                frame KeyLine behind the camera (optimizeScaleBack falls back to 1), and a link out of range (no reference output: it
                reads out of bounds).  Lists of 4, 2 and 1 key frames from three consecutive moves, iters = 1 and 3.
  chained.npz   frames 2 and 3 of synth.billboard_sequence (256x192) against frame 0 as key frame, links as
                tests/golden/keyframe_constraint/chained.npz builds them; one list of 3 from frames 0, 2, 3.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import keyframe_depth_port as port  # noqa: E402
import make_keyframe_constraint_golden as cg  # noqa: E402
from rebvo_amd import synth  # noqa: E402
from rebvo_amd.edgehip import KEYLINE_DTYPE  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_depth")
SIZE_LIMIT = 1000000
MAP_ARGS = ((0.0, 0.0, 1.0), (1e-3, 5e-2, 2.0))
# (call, direction, optim_scale, (q_abs, q_rel, loc_unc))
CALLS = [("map", 0, 0, MAP_ARGS[0]), ("map", 0, 0, MAP_ARGS[1]), ("translate", 0, 0, (0, 0, 0)), ("translate", 0, 1, (0, 0, 0)),
         ("translate", 1, 0, (0, 0, 0))]
REQUIRED = ("branch_min", "branch_max", "branch_nonfinite", "branch_negative", "branch_none", "min_with_nan_s_rho", "rotate_zeros", "scale_behind",
            "scale_fallback_pairs")


def build_driver(ref, tmp):
    inc = os.path.join(ROOT, "oracle", "_ref", "inc")
    lib = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(lib, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(cg.PRELUDE)
    # kfvo.cpp:10-17: the helpers isnan(double&) / isinf(double&) call themselves where <cmath> has no such macro: mapKLUsingIDK would
    # never return.  The driver includes this copy, in which those two calls name the std:: functions (checked: one place each).
    with open(os.path.join(ref, "src", "mtracklib", "kfvo.cpp")) as f:
        src = f.read()
    for fn in ("isnan", "isinf"):
        assert src.count(f"return {fn}(tmp);") == 1, fn
        src = src.replace(f"return {fn}(tmp);", f"return std::{fn}(tmp);")
    with open(os.path.join(tmp, "kfvo_terminating.cpp"), "w") as f:
        f.write(src)
    exe = os.path.join(tmp, "kf_depth_driver")
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre,
           "-I" + inc, "-I" + os.path.join(ref, "include"), "-I" + ref, "-I" + tmp,
           os.path.join(ROOT, "tools", "keyframe_depth_ref_driver.cpp"), os.path.join(ref, "src", "mtracklib", "keyframe.cpp"),
           os.path.join(ref, "src", "visualizer", "depth_filler.cpp"),
           "-L" + lib, "-Wl,-rpath," + lib, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, mode, flag, kfs, cam, args=(0, 0, 0)):
    """kfs: [(records, Pose, Pos, K)] -> dict(count, K, seconds, records=[the records as the call left them])"""
    payload = np.array([mode, len(kfs), flag, 0], np.int32).tobytes()
    payload += np.array([cam["ppx"], cam["ppy"], cam["zfx"], cam["zfy"]], np.float32).tobytes()
    payload += np.array([cam["w"], cam["h"]], np.int32).tobytes()
    payload += np.array(args, np.float64).tobytes()
    for rec, Pose, Pos, K in kfs:
        payload += np.array([len(rec), 0], np.int32).tobytes()
        payload += np.concatenate([np.ravel(Pose), np.ravel(Pos), [K]]).astype(np.float64).tobytes()
        payload += rec.tobytes()
    with tempfile.NamedTemporaryFile(prefix="kf_depth_out_") as f:
        subprocess.run([exe, f.name], input=payload, check=True, stdout=subprocess.DEVNULL)
        out = open(f.name, "rb").read()
    assert len(out) == 24 + 168 * sum(len(k[0]) for k in kfs), len(out)
    head = np.frombuffer(out, np.int32, 2, 0)
    res = np.frombuffer(out, np.float64, 2, 8)
    recs, at = [], 24
    for rec, _, _, _ in kfs:
        recs.append(np.frombuffer(out, KEYLINE_DTYPE, len(rec), at).copy())
        at += 168 * len(rec)
    return dict(count=int(head[0]), K=np.float64(res[0]), seconds=float(res[1]), records=recs)


def only_depth_moved(before, after, with_m_num):
    """the reference wrote rho, s_rho (and m_num) and no other byte"""
    back = after.copy()
    for k in ("rho", "s_rho") + (("m_num",) if with_m_num else ()):
        back[k] = before[k]
    return back.tobytes() == before.tobytes()


def pair_records(pair):
    return (port.records(pair["kf"], KEYLINE_DTYPE, dict(m_id_f=pair["kf"]["m_id_f"])),
            port.records(pair["fr"], KEYLINE_DTYPE, dict(m_id_kf=pair["fr"]["m_id_kf"])))


def check_pair_case(exe, pair, cam, call, direction, optim, args, name, stats):
    """-> the reference's outputs (with the port's rTr, rTr0), after the port was held against them"""
    kf_rec, fr_rec = pair_records(pair)
    kfs = [(kf_rec, pair["kf_Pose"], pair["kf_Pos"], float(pair["kf_K"])), (fr_rec, pair["Pose"], pair["Pos"], float(pair["K"]))]
    trace = {}
    if call == "map":
        ref = run_ref(exe, 0, 0, kfs, cam, args)
        rho, s_rho, count, guard = port.map_depth(pair, *args, trace=trace)
        got = dict(rho=rho, s_rho=s_rho, m_num=np.array(pair["kf"]["m_num"], np.int32), count=count, guard=guard, K=np.float64(0), rTr=np.float64(0), rTr0=np.float64(0))
        written, untouched = 0, 1
    else:
        ref = run_ref(exe, 2 if direction else 1, optim, kfs, cam)
        got = port.translate(pair, direction, bool(optim), trace)
        written, untouched = (1, 0) if direction else (0, 1)
        assert ref["count"] == got["count"], (name, "count", ref["count"], got["count"])
        assert ref["K"] == got["K"], (name, "K", ref["K"], got["K"])
    assert got["guard"] == 0, (name, "guard")
    before = (kf_rec, fr_rec)
    out = ref["records"][written]
    assert ref["records"][untouched].tobytes() == before[untouched].tobytes(), (name, "the other list changed")
    assert only_depth_moved(before[written], out, call == "translate" and not direction), (name, "another field changed")
    assert port.same_bits(out["rho"], got["rho"]), (name, "rho", np.nonzero(out["rho"] != got["rho"])[0][:5])
    assert port.same_bits(out["s_rho"], got["s_rho"]), (name, "s_rho", np.nonzero(out["s_rho"] != got["s_rho"])[0][:5])
    assert np.array_equal(out["m_num"], got["m_num"]), (name, "m_num")
    if call == "map":
        b = trace["branch"]
        for j, k in enumerate(port.BRANCHES):
            stats["branch_" + k] = stats.get("branch_" + k, 0) + int((b == j).sum())
        # the classes, on the REFERENCE's outputs
        r, s = out["rho"][trace["idx"]], out["s_rho"][trace["idx"]]
        assert (r[b == 0] == port.RHO_MIN).all() and (r[b == 1] == port.RHO_MAX).all(), name
        assert ((r[(b == 2) | (b == 3)] == port.RHO_INIT) & (s[(b == 2) | (b == 3)] == port.RHO_MAX)).all(), name
        nm = int((np.isnan(s) & (r == port.RHO_MIN)).sum())
        assert nm == trace["min_with_nan_s_rho"], name
        stats["min_with_nan_s_rho"] = stats.get("min_with_nan_s_rho", 0) + nm
        stats["rotate_zeros"] = stats.get("rotate_zeros", 0) + trace["rotate_zeros"]
        none_share = float((b == 4).mean()) if len(b) else 1.0
        if pair["kind"] == "compared":
            assert none_share >= 0.5, (name, "linked KeyLines through no clamp", none_share)
    else:
        none_share = -1.0
        if optim:
            stats["scale_behind"] = stats.get("scale_behind", 0) + trace["scale_behind"]
            if trace["scale_links"] > 0 and trace["scale_behind"] == trace["scale_links"]:
                assert ref["K"] == 1.0, name
                stats["scale_fallback_pairs"] = stats.get("scale_fallback_pairs", 0) + 1
    return dict(rho=out["rho"], s_rho=out["s_rho"], m_num=out["m_num"], count=got["count"], K=ref["K"] if call == "translate" else np.float64(0),
                rTr=got["rTr"], rTr0=got["rTr0"], seconds=ref["seconds"], none_share=none_share)


def chain_records(chain):
    return [(port.records(k["kl"], KEYLINE_DTYPE, dict(m_id_f=k["kl"]["m_id_f"])), k["Pose"], k["Pos"], float(k["K"])) for k in chain]


def check_list_case(exe, chain, cam, iters, name):
    kfs = chain_records(chain)
    ref = run_ref(exe, 3, iters, kfs, cam)
    got, count, guard = port.list_translate(chain, iters, float(cam["zfm"]))
    assert guard == 0, name
    for i, (k, out) in enumerate(zip(got, ref["records"])):
        assert only_depth_moved(kfs[i][0], out, True), (name, i)
        assert port.same_bits(out["rho"], k["kl"]["rho"]) and port.same_bits(out["s_rho"], k["kl"]["s_rho"]), (name, i, "rho / s_rho")
        assert np.array_equal(out["m_num"], k["kl"]["m_num"]), (name, i, "m_num")
    if len(chain):
        assert ref["records"][-1].tobytes() == kfs[-1][0].tobytes(), (name, "the newest position changed")
    return dict(records=ref["records"], count=count, seconds=ref["seconds"])


def rot(ax, ay, az):
    return synth._so3_exp(np.array([ax, ay, az], np.float64))


def random_list(rs, n, cam, specials=True):
    w, h = int(cam["w"]), int(cam["h"])
    pp = np.array([cam["ppx"], cam["ppy"]], np.float64)
    pix = np.stack([rs.uniform(2, w - 3, n), rs.uniform(2, h - 3, n)], 1)
    ang = rs.uniform(0, 2 * np.pi, n)
    lst = dict(p_m=(pix - pp).astype(np.float32), u_m=np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32), rho=rs.uniform(0.3, 1.5, n),
               s_rho=rs.uniform(0.02, 0.4, n), m_num=rs.randint(0, 40, n).astype(np.int32))
    if specials and n >= 65:   # KeyLines at the ends of the depth range and with no depth information: the update can leave through a clamp
        k = max(3, n // 40)
        pick = rs.choice(n, 3 * k, replace=False)
        lst["rho"][pick[:k]], lst["s_rho"][pick[:k]] = 0.0015, 0.5
        lst["rho"][pick[k:2 * k]], lst["s_rho"][pick[k:2 * k]] = 19.9, 5.0
        lst["rho"][pick[2 * k:]], lst["s_rho"][pick[2 * k:]] = 0.002, 1e12
    return lst, ang


def move_list(rs, lst, ang, cam, Rt, tt, drop=True):
    """The list seen from a camera moved by (Rt, tt), with 0.3 px of noise, a few KeyLines of its own and a few behind the camera
    -> (frame list, its angles, m_id_f of `lst`, m_id_kf of the frame list)"""
    n, zfm = len(lst["rho"]), float(cam["zfm"])
    p_m, rho = lst["p_m"].astype(np.float64), lst["rho"]
    x = np.stack([p_m[:, 0] / rho / zfm, p_m[:, 1] / rho / zfm, 1 / rho], 1)
    y = x @ Rt.T + tt
    q = np.stack([y[:, 0] / y[:, 2] * zfm, y[:, 1] / y[:, 2] * zfm], 1) + rs.normal(0, 0.3, (n, 2))
    extra = 7 if n >= 5 else 0
    fr, fang = random_list(rs, n + extra, cam, specials=False)
    perm = rs.permutation(n + extra)[:n]
    fr["p_m"][perm] = q
    a2 = ang + rs.normal(0, 0.05, n)
    fr["u_m"][perm] = np.stack([np.cos(a2), np.sin(a2)], 1)
    fang[perm] = a2
    fr["rho"][perm] = 1 / y[:, 2]
    if n >= 65:
        fr["rho"][perm[rs.choice(n, max(1, n // 100), replace=False)]] *= -1
    m_id_f = perm.astype(np.int32)
    m_id_kf = np.full(n + extra, -1, np.int32)
    m_id_kf[perm] = np.arange(n)
    if n >= 65 and drop:
        m_id_f[rs.rand(n) < 0.2] = -1
        m_id_kf[rs.rand(n + extra) < 0.2] = -1
    return fr, fang, m_id_f, m_id_kf


MOVES = [((0.02, -0.03, 0.015), (0.05, -0.03, 0.02)), ((-0.015, 0.02, 0.01), (0.04, 0.02, -0.01)), ((0.01, 0.025, -0.02), (-0.03, 0.04, 0.015))]


def crafted_pair(rs, n, cam, kind="compared", Rt=None, tt=None, KP=None):
    Rt = rot(*MOVES[0][0]) if Rt is None else Rt
    tt = np.array(MOVES[0][1]) if tt is None else tt
    kf, ang = random_list(rs, n, cam)
    fr, _, m_id_f, m_id_kf = move_list(rs, kf, ang, cam, Rt, tt)
    KP = rot(0.1, -0.2, 0.05) if KP is None else KP
    KPos = np.array([0.3, -0.1, 0.2])
    Pose = cg.port.matmul(KP, Rt.T)
    Pos = KPos - cg.port.matvec(Pose, tt)
    return dict(kf=dict(kf, m_id_f=m_id_f), fr=dict(fr, m_id_kf=m_id_kf), kf_Pose=KP, kf_Pos=KPos, kf_K=np.float64(1.1), Pose=Pose, Pos=Pos,
                K=np.float64(1.05), zfm=float(cam["zfm"]), kind=kind)


def crafted_chain(rs, n, cam, length=4):
    """`length` key frames from consecutive moves: entry i's m_id_f index entry i + 1's KeyLines"""
    lst, ang = random_list(rs, n, cam)
    Pose, Pos = rot(0.1, -0.2, 0.05), np.array([0.3, -0.1, 0.2])
    Ks = [1.1, 1.05, 0.97, 1.02]
    chain = []
    for i in range(length):
        if i + 1 < length:
            Rt, tt = rot(*MOVES[i % 3][0]), np.array(MOVES[i % 3][1])
            nxt, nang, m_id_f, _ = move_list(rs, lst, ang, cam, Rt, tt)
        else:
            m_id_f = np.full(len(lst["rho"]), -1, np.int32)
        chain.append(dict(kl=dict(lst, m_id_f=m_id_f), Pose=Pose, Pos=Pos, K=np.float64(Ks[i % 4])))
        if i + 1 < length:
            Pose = cg.port.matmul(Pose, Rt.T)
            Pos = Pos - cg.port.matvec(Pose, tt)
            lst, ang = nxt, nang
    return chain


def pack(pairs, cam, cases, refs, lists, list_cases, list_refs, stats, arrays=lambda case: True):
    rec = {f"cam_{k}": np.asarray(v) for k, v in cam.items()}
    rec["n_pairs"], rec["n_cases"], rec["n_lists"], rec["n_list_cases"] = (np.int32(len(x)) for x in (pairs, cases, lists, list_cases))
    for j, p in enumerate(pairs):
        pre = f"p{j}_"
        for k in port.LIST_FIELDS:
            rec[pre + "kf_" + k], rec[pre + "fr_" + k] = p["kf"][k], p["fr"][k]
        rec[pre + "kf_m_id_f"], rec[pre + "fr_m_id_kf"] = p["kf"]["m_id_f"].astype(np.int32), p["fr"]["m_id_kf"].astype(np.int32)
        for k in ("kf_Pose", "kf_Pos", "kf_K", "Pose", "Pos", "K"):
            rec[pre + k] = np.asarray(p[k], np.float64)
        rec[pre + "kind"] = np.array(p["kind"])
    rec["case_pair"] = np.array([c[0] for c in cases], np.int32)
    rec["case_call"] = np.array([c[1] for c in cases])
    rec["case_direction"] = np.array([c[2] for c in cases], np.int32)
    rec["case_optim"] = np.array([c[3] for c in cases], np.int32)
    rec["case_args"] = np.array([c[4] for c in cases], np.float64).reshape(len(cases), 3)
    rec["ref_count"] = np.array([r["count"] for r in refs], np.int32)
    for k in ("K", "rTr", "rTr0", "seconds", "none_share"):
        rec["ref_" + k] = np.array([r[k] for r in refs], np.float64)
    rec["ref_digest"] = np.array([port.digest(r["rho"], r["s_rho"], r["m_num"]) for r in refs])
    for c, (case, r) in enumerate(zip(cases, refs)):
        if arrays(case):
            rec[f"case{c}_rho"], rec[f"case{c}_s_rho"], rec[f"case{c}_m_num"] = r["rho"], r["s_rho"], r["m_num"]
    for j, chain in enumerate(lists):
        rec[f"l{j}_len"] = np.int32(len(chain))
        for i, k in enumerate(chain):
            for f in port.LIST_FIELDS + ("m_id_f",):
                rec[f"l{j}_{i}_{f}"] = k["kl"][f]
            rec[f"l{j}_{i}_Pose"], rec[f"l{j}_{i}_Pos"], rec[f"l{j}_{i}_K"] = (np.asarray(k[f], np.float64) for f in ("Pose", "Pos", "K"))
    rec["lcase_list"] = np.array([c[0] for c in list_cases], np.int32)
    rec["lcase_iters"] = np.array([c[1] for c in list_cases], np.int32)
    rec["lref_count"] = np.array([r["count"] for r in list_refs], np.int32)
    rec["lref_seconds"] = np.array([r["seconds"] for r in list_refs], np.float64)
    for c, r in enumerate(list_refs):
        rec[f"lcase{c}_digests"] = np.array([port.digest(o["rho"], o["s_rho"], o["m_num"]) for o in r["records"]])
        if arrays(None):
            for i, o in enumerate(r["records"]):
                rec[f"lcase{c}_{i}_rho"], rec[f"lcase{c}_{i}_s_rho"], rec[f"lcase{c}_{i}_m_num"] = o["rho"].copy(), o["s_rho"].copy(), o["m_num"].copy()
    keys = sorted(stats)
    rec["stat_names"], rec["stat_values"] = np.array(keys), np.array([stats[k] for k in keys], np.int64)
    return rec


def run_all(exe, pairs, cam, name, stats):
    cases, refs = [], []
    for j, p in enumerate(pairs):
        if p["kind"] == "link_out_of_range":
            continue
        for call, d, opt, args in CALLS:
            cases.append((j, call, d, opt, args))
            refs.append(check_pair_case(exe, p, cam, call, d, opt, args, f"{name} pair {j} ({p['kind']}) {call} dir {d} optim {opt} {args}", stats))
    return cases, refs


TIMING = dict(w=752, h=480, kn=16000, positions=8, iters=3, seed=7)


def timing_inputs(params):
    """tools/keyframe_depth_timing.py's inputs: a pair and a list of TIMING["positions"] key frames of TIMING["kn"] KeyLines at 752x480 with
    the crafted lists' noise and dropped links (about 80 % linked) -> (pair, chain, cam)."""
    cam = cg.camera(TIMING["w"], TIMING["h"], params.ppx, params.ppy, params.zfx, params.zfy)
    rs = np.random.RandomState(TIMING["seed"])
    return crafted_pair(rs, TIMING["kn"], cam), crafted_chain(rs, TIMING["kn"], cam, TIMING["positions"]), cam


def timing_reference(exe):
    """The reference's one-core seconds (the median of 3 runs of each function alone) for the timing inputs."""
    from rebvo_amd import edgehip
    pair, chain, cam = timing_inputs(edgehip.euroc_params(TIMING["w"], TIMING["h"]))
    kf_rec, fr_rec = pair_records(pair)
    kfs = [(kf_rec, pair["kf_Pose"], pair["kf_Pos"], float(pair["kf_K"])), (fr_rec, pair["Pose"], pair["Pos"], float(pair["K"]))]
    rec = {}
    for tag, mode, flag, args in (("map", 0, 0, MAP_ARGS[1]), ("f2kf", 1, 0, (0, 0, 0)), ("f2kf_optim", 1, 1, (0, 0, 0)), ("kf2f", 2, 0, (0, 0, 0))):
        rec["timing_ref_seconds_" + tag] = np.float64(np.median([run_ref(exe, mode, flag, kfs, cam, args)["seconds"] for _ in range(3)]))
    ckfs = chain_records(chain)
    rec["timing_ref_seconds_list"] = np.float64(np.median([run_ref(exe, 3, TIMING["iters"], ckfs, cam)["seconds"] for _ in range(3)]))
    rec["timing_kn"], rec["timing_positions"], rec["timing_iters"] = np.int32(TIMING["kn"]), np.int32(TIMING["positions"]), np.int32(TIMING["iters"])
    rec["timing_linked_share"] = np.float64((pair["kf"]["m_id_f"] >= 0).mean())
    print("timing reference:", {k: float(v) for k, v in rec.items()})
    return rec


def crafted(exe):
    cam = cg.camera(70, 50, 34.3, 25.6, 60.0, 62.0)
    sizes = [0, 1, 5, 65, 257, 600, 1030]
    quarter = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    half = np.array([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])
    for seed in range(40):
        rs = np.random.RandomState(seed)
        pairs = [crafted_pair(rs, n, cam, "compared" if n >= 65 else "few_links") for n in sizes]
        pairs[0]["kind"] = "no_links"
        nan = crafted_pair(rs, 65, cam, "nan_rho")
        for lst, col in ((nan["kf"], "m_id_f"), (nan["fr"], "m_id_kf")):
            lst["rho"][np.nonzero(lst[col] >= 0)[0][3]] = np.nan
        turn_h = crafted_pair(rs, 65, cam, "half_turn", Rt=half, KP=np.eye(3))
        turn_q = crafted_pair(rs, 65, cam, "quarter_turn", Rt=quarter, KP=np.eye(3))
        turn_q["kf"]["p_m"][np.nonzero(turn_q["kf"]["m_id_f"] >= 0)[0][:3]] = 0.0
        behind = crafted_pair(rs, 65, cam, "all_behind")
        behind["fr"]["rho"] = -np.abs(behind["fr"]["rho"])
        oob = crafted_pair(rs, 65, cam, "link_out_of_range")
        oob["kf"]["m_id_f"][np.nonzero(oob["kf"]["m_id_f"] >= 0)[0][5]] = len(oob["fr"]["rho"]) + 2
        oob["fr"]["m_id_kf"][np.nonzero(oob["fr"]["m_id_kf"] >= 0)[0][5]] = len(oob["kf"]["rho"])
        pairs += [nan, turn_h, turn_q, behind, oob]
        stats = {}
        try:
            cases, refs = run_all(exe, pairs, cam, f"crafted seed {seed}", stats)
        except AssertionError as e:
            if "through no clamp" in str(e):
                print(f"crafted seed {seed}: {e}")
                continue
            raise
        missing = [k for k in REQUIRED if stats.get(k, 0) == 0]
        if not missing:
            break
        print(f"crafted seed {seed}: populations missing {missing}: {stats}")
    else:
        raise SystemExit("crafted: no seed populates every branch")
    chain = crafted_chain(rs, 257, cam, 4)
    lists = [chain, chain[:2], chain[:1]]
    list_cases = [(j, it) for j in range(3) for it in (1, 3)]
    list_refs = [check_list_case(exe, lists[j], cam, it, f"crafted list {j} iters {it}") for j, it in list_cases]
    # the read-before-update rule must be visible: walking downwards gives other bits
    other, _, _ = port.list_translate(chain, 1, float(cam["zfm"]), successors_first=True)
    assert not port.same_bits(other[0]["kl"]["rho"], list_refs[0]["records"][0]["rho"]), "the list cannot tell the two walks apart"
    rec = pack(pairs, cam, cases, refs, lists, list_cases, list_refs, stats)
    rec["seed"] = np.int32(seed)
    rec.update(timing_reference(exe))
    shares = [r["none_share"] for c, r in zip(cases, refs) if c[1] == "map" and pairs[c[0]]["kind"] == "compared"]
    print(f"crafted: seed {seed}, {len(cases)} cases, {len(list_cases)} list cases, stats {stats}, share of linked KeyLines through no clamp "
          f"in the compared map cases {np.round(shares, 3).tolist()}")
    return rec


def chained(exe, ref_root, tmp):
    pairs, cam, frames = cg.chained_pairs(ref_root, tmp)
    for p, k in zip(pairs, (2, 3)):
        p["kf"]["m_num"], p["fr"]["m_num"] = frames[0]["kl"]["m_num"].astype(np.int32), frames[k]["kl"]["m_num"].astype(np.int32)
    stats = {}
    cases, refs = run_all(exe, pairs, cam, "chained", stats)
    # frames 0, 2, 3 as a list: frame 0's links are the first pair's; frame 2's are frame 3's matches into it, turned round (lowest index wins)
    f2, f3 = frames[2], frames[3]
    m = f3["kl"]["m_id"]
    fwd = np.full(len(f2["kl"]), -1, np.int32)
    for j in range(len(m) - 1, -1, -1):
        if 0 <= m[j] < len(fwd):
            fwd[m[j]] = j
    lst = lambda kl: {k: kl[k].copy() for k in port.LIST_FIELDS}   # noqa: E731
    chain = [dict(kl=dict(pairs[0]["kf"]), Pose=pairs[0]["kf_Pose"], Pos=pairs[0]["kf_Pos"], K=pairs[0]["kf_K"]),
             dict(kl=dict(lst(f2["kl"]), m_id_f=fwd), Pose=f2["Pose"], Pos=f2["Pos"], K=np.float64(f2["K"])),
             dict(kl=dict(lst(f3["kl"]), m_id_f=np.full(len(f3["kl"]), -1, np.int32)), Pose=f3["Pose"], Pos=f3["Pos"], K=np.float64(f3["K"]))]
    list_cases = [(0, 1), (0, 3)]
    list_refs = [check_list_case(exe, chain, cam, it, f"chained list iters {it}") for _, it in list_cases]
    print(f"chained: kn {[(len(p['kf']['rho']), len(p['fr']['rho'])) for p in pairs]} counts {[r['count'] for r in refs]} list counts "
          f"{[r['count'] for r in list_refs]} stats {stats}")
    # the frame lists are the list's entries 1 and 2: stored once
    return pack(pairs, cam, cases, refs, [chain], list_cases, list_refs, stats, arrays=lambda case: case is not None and case[3] == 1)


def write(path, rec):
    # an array that is already in the file under another name (the chained list's entries are the pairs' lists) is stored once
    seen = {}
    for k in sorted(rec):
        v = np.asarray(rec[k])
        if v.nbytes < 1024:
            continue
        key = (v.dtype.str, v.shape, v.tobytes())
        if key in seen:
            del rec[k]
            rec[k + "__alias"] = np.array(seen[key])
        else:
            seen[key] = k
    np.savez_compressed(path, **rec)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size <= SIZE_LIMIT, (path, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF"), help="the reference tree (or $REBVO_REF)")
    ap.add_argument("--only", choices=("crafted", "chained"))
    a = ap.parse_args()
    if not a.ref:
        raise SystemExit("give --ref /path/to/reference (or set REBVO_REF)")
    os.makedirs(GOLD, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix="keyframe_depth_ref_") as tmp:
        exe = build_driver(a.ref, tmp)
        if a.only != "chained":
            write(os.path.join(GOLD, "crafted.npz"), crafted(exe))
        if a.only != "crafted":
            write(os.path.join(GOLD, "chained.npz"), chained(exe, a.ref, tmp))


if __name__ == "__main__":
    main()
