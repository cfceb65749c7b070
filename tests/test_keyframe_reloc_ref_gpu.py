"""edgehip_keyframe_relocalize against the REFERENCE's own kfvo::OptimizePosGT, recorded in tests/golden/keyframe_reloc/ by
tools/make_keyframe_reloc_golden.py: every case of both fixtures, no case left out.

Tolerances (the project's own for this minimiser): mnum and every m_id_f exact; X, Pose rtol 1e-9 + atol 1e-12; Pos the same, relative to the
larger of |Pos_t| and |BRelPos K|; score_ratio, Kp, K 1e-9 relative; RRV 1e-7 relative.  Where the reference's RRV is not finite (no link
at all: JtJ = 0) the device's is not finite either.  evals and accepted exact: they are the port's, which the tool ties to the reference
(OptimizePosGT returns neither).  The four cases whose key frame has 1 or 5 KeyLines have fewer than 30 links — six unknowns from fewer
rows — and are marked not numeric by the tool: their links, mnum and evals are compared, exactly, their fp64 outputs are not.

The cases of a fixture that share (field_radius, iter_max, rew_dis, rho_tol) go through ONE call as a ragged batch: one sequence per case,
its key frame as the current key frame, its query in ring slot 0, its own s_rho_q.  The chained cases run a second time with the three key
frames as ONE sequence's list (two entries and the current key frame): the same results at positions 0 .. 2."""
import os

import numpy as np
import pytest

import keyframe_covis_port as cport
import keyframe_reloc_port as port
from rebvo_amd import edgehip

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_reloc")
_FX = {}


def fixture(name):
    if name not in _FX:
        _FX[name] = port.load_fixture(os.path.join(GOLD, name + ".npz"))
    return _FX[name]


def pose(k):
    return edgehip.EdgeHip.kf_pose(k["Pose"], k["Pos"], K=float(k["K"]))


def context(f, nseq, capacity, radius):
    cam = f["cam"]
    mp = max([len(k["n_m"]) for k in f["kfs"]] + [len(c["q"]["n_m"]) for c in f["cases"]]) + 3
    p = edgehip.euroc_params(int(cam["w"]), int(cam["h"]), ppx=float(cam["ppx"]), ppy=float(cam["ppy"]), zfx=float(cam["zfx"]),
                             zfy=float(cam["zfy"]), max_points=mp, search_range=radius)
    eh = edgehip.EdgeHip(p, nseq=nseq, nslots=2, device=0)
    eh.keyframe_track_enable(True, 0.7, True, in_frame_driver=False)
    if capacity:
        eh.keyframe_list_enable(capacity)
    return eh


def within(got, want, rtol, atol=0.0, scale=None):
    got, want = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want, np.float64))
    fin = np.isfinite(want)
    if not np.array_equal(np.isfinite(got), fin):
        return False
    ref = np.abs(want) if scale is None else np.broadcast_to(scale, want.shape)
    return bool(np.all(np.abs(got[fin] - want[fin]) <= atol + rtol * ref[fin]))


def check(tag, g, links, c, kf):
    r, a = c["ref"], c["args"]
    assert np.array_equal(links, r["m_id_f"].astype(np.int32)), (tag, int((links != r["m_id_f"]).sum()))
    assert int(g["mnum"]) == int(r["mnum"]) and int(g["guard"]) == 0 and int(g["evals"]) == int(r["evals"]), tag
    print(tag, c["kind"], "numeric" if c["numeric"] else "integers only", "mnum", int(g["mnum"]), "accepted", int(g["accepted"]), int(r["accepted"]),
          "dX", np.abs(np.array(g["X"]) - r["X"]).max(), "dKp", abs(float(g["Kp"]) - float(r["Kp"])), "r", float(g["score_ratio"]), float(r["r"]))
    if not c["numeric"]:          # a key frame of 1 or 5 KeyLines: fewer than 30 links, six unknowns from fewer rows (the tool's docstring)
        return
    assert int(g["accepted"]) == int(r["accepted"]), (tag, int(g["accepted"]), int(r["accepted"]))
    assert within(g["X"], r["X"], 1e-9, 1e-12), (tag, list(g["X"]), r["X"])
    assert within(g["score_ratio"], r["r"], 1e-9), (tag, g["score_ratio"], r["r"])
    assert within(np.array(g["RRV"]).reshape(6, 6), r["RRV"], 1e-7), tag
    assert within(g["Kp"], r["Kp"], 1e-9) and within(g["K"], r["K"], 1e-9), (tag, g["Kp"], r["Kp"])
    assert within(np.array(g["Pose"]).reshape(3, 3), r["Pose"], 1e-9, 1e-12), tag
    scale = max(np.linalg.norm(kf["Pos"]), np.linalg.norm(r["X"][:3]) * float(r["K"]))
    assert within(g["Pos"], r["Pos"], 1e-9, 1e-12, scale=scale), (tag, list(g["Pos"]), r["Pos"])


def groups(f):
    out = {}
    for i, c in enumerate(f["cases"]):
        a = c["args"]
        out.setdefault((a["field_radius"], a["field_min_mod"], a["iter_max"], a["rew_dis"], a["rho_tol"]), []).append(i)
    return out


@pytest.mark.parametrize("name", ["crafted", "chained"])
def test_every_fixture_case_equals_the_reference(name):
    f = fixture(name)
    done = accepted = 0
    for (radius, min_mod, iter_max, rew_dis, rho_tol), idx in groups(f).items():
        eh = context(f, len(idx), 0, radius)
        try:
            for s, i in enumerate(idx):
                c = f["cases"][i]
                eh.upload_keyframe(s, cport.records(f["kfs"][c["t"]], edgehip.KEYLINE_DTYPE), pose(f["kfs"][c["t"]]))
                if len(c["q"]["n_m"]):
                    eh.upload_keylines(s, 0, cport.records(c["q"], edgehip.KEYLINE_DTYPE))
            got, _ = eh.keyframe_relocalize(0, [f["cases"][i]["args"]["s_rho_q"] for i in idx], radius, iter_max, rew_dis, rho_tol,
                                            field_min_mod=min_mod, poses=[pose(f["cases"][i]["q"]) for i in idx])
            for s, i in enumerate(idx):
                c = f["cases"][i]
                check((name, i), got[s, 0], eh.keyframe_relocalize_links(s, 0), c, f["kfs"][c["t"]])
                accepted += int(got["accepted"][s, 0])
                if c["kind"] != "moved":
                    assert got["Kp"][s, 0] == 1.0                       # optimizeScale's fallback: no link, or every q1[2] <= 0
                done += 1
        finally:
            eh.close()
    assert done == len(f["cases"]) and accepted > 0


def test_chained_cases_as_one_sequence_s_list():
    f = fixture("chained")
    cases = [c for c in f["cases"] if c["args"]["iter_max"] == 6]
    assert [c["t"] for c in cases] == [0, 1, 2]
    a = cases[0]["args"]
    eh = context(f, 2, 3, a["field_radius"])
    try:
        for m in range(3):
            eh.upload_keyframe(1, cport.records(f["kfs"][m], edgehip.KEYLINE_DTYPE), pose(f["kfs"][m]))
        for s in range(2):
            eh.upload_keylines(s, 0, cport.records(cases[0]["q"], edgehip.KEYLINE_DTYPE))
        got, info = eh.keyframe_relocalize(0, a["s_rho_q"], a["field_radius"], 6, a["rew_dis"], a["rho_tol"], poses=[pose(cases[0]["q"])] * 2)
        assert list(info["held"]) == [0, 2] and (got["mnum"][0] == -1).all() and got["mnum"][1, 3] == -1
        for t, c in enumerate(cases):
            check(("list", t), got[1, t], eh.keyframe_relocalize_links(1, t), c, f["kfs"][t])
    finally:
        eh.close()


def test_degenerate_inputs_return():
    """NaN rho in the query (stored as an input only: the reference is not run on it): two KeyLines are counted, the call returns.  (A NaN rho
    makes that KeyLine's Jacobian row NaN * 0 in the reference's arithmetic and the device's alike: X and the links are lost, nothing else.)"""
    f = fixture("crafted")
    d = f["nan_query"]
    eh = context(f, 1, 0, 5)
    try:
        eh.upload_keyframe(0, cport.records(f["kfs"][d["t"]], edgehip.KEYLINE_DTYPE), pose(f["kfs"][d["t"]]))
        eh.upload_keylines(0, 0, cport.records(d["q"], edgehip.KEYLINE_DTYPE))
        got, _ = eh.keyframe_relocalize(0, 0.39, 5, 6, 2.0, 1.5, poses=[pose(d["q"])])
        assert got["guard"][0, 0] >= 2 and got["evals"][0, 0] == 7 and got["mnum"][0, 0] >= 0
    finally:
        eh.close()
