#!/usr/bin/env python3
"""Generate tests/golden/edgemap_decode/{crafted,billboard}.npz from the REFERENCE's edgemap_com_decoder.

Build machine only (needs the reference tree and oracle/_ref from `make -C oracle`):
    python tools/make_edgemap_decode_golden.py [--ref /path/to/reference]

tools/edgemap_decode_ref_driver.cpp is compiled with the reference's src/CommLib/edgemap_com.cpp, src/UtilLib/linefitting.cpp,
src/UtilLib/libcrc.cpp and src/visualizer/depth_filler.cpp in place, into oracle/_ref/ (kept out of the repository; no reference source is
copied).  The fixtures are data only: per case the records, rho_scale and thresholds, Decode's segments, GetDPose() / GetDPos() of every
view, HideVisible's flags and s_num after every view, and the grid after fillDepthMap alone and after the whole chain.

The generator REFUSES to write a set in which
  - the serial host restatement (rebvo/edgemap_com.h through tools/edgemap_decode_host_check.cpp) differs from the reference in any bit
    (segments, DPose, DPos, flags, s_num, the grid after the fill),
  - the numpy port's chain behind that grid differs from the reference's,
  - one of the populations the crafted lists are there for is empty."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import edgemap_decode_crafted as crafted  # noqa: E402
from tests import edgemap_decode_port as port  # noqa: E402
from tools.make_edgemap_golden import PRELUDE  # noqa: E402

# billboard frame: (block_w, block_h, iter_num, bound_mode): the grid in LDS, in HBM (85 x 64 cells), and with a boundary
BILLBOARD = {3: (8, 8, 10, 0), 5: (3, 3, 4, 0), 6: (8, 4, 10, 2)}
BILLBOARD_THRESH = (1.0, 45.0)
POPULATIONS = ("segments", "shared_vertex", "closing_k1", "negative_k0", "partner_self", "s_rho_floor", "gate_sigma", "gate_sum", "gate_rel",
               "gate_angle", "degenerate", "folded", "hidden", "kept", "already_hidden", "behind", "fixed_cells")


def build_driver(ref, tmp):
    out = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(out, "libreforacle.so")):
        raise SystemExit("oracle/_ref/libreforacle.so is missing: run `make -C oracle` first")
    pre = os.path.join(tmp, "prelude.h")
    with open(pre, "w") as f:
        f.write(PRELUDE)
    exe = os.path.join(out, "edgemap_decode_ref_driver")
    src = [os.path.join(ref, "src", *p) for p in (("CommLib", "edgemap_com.cpp"), ("UtilLib", "linefitting.cpp"), ("UtilLib", "libcrc.cpp"),
                                                  ("visualizer", "depth_filler.cpp"))]
    cmd = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-fno-access-control", "-w", "-include", pre, "-I" + os.path.join(out, "inc"),
           "-I" + os.path.join(ref, "include"), "-I" + ref, os.path.join(ROOT, "tools", "edgemap_decode_ref_driver.cpp")] + src + \
          ["-L" + out, "-Wl,-rpath," + out, "-lreforacle", "-lm", "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run_ref(exe, records, rho_scale, v_thresh, a_thresh, **kw):
    size, block, views = kw.get("size", (crafted.W, crafted.H)), kw.get("block", (crafted.BW, crafted.BH)), kw.get("views", crafted.VIEWS)
    out = subprocess.run([exe], input=crafted.payload(records, rho_scale, v_thresh, a_thresh, **kw), check=True, capture_output=True).stdout
    return crafted.parse(out, len(views), (size[0] // block[0]) * (size[1] // block[1]), False)


def one_case(tag, c, exe_ref, exe_host, arrays, pop, **kw):
    rec = c["records"]
    ref = run_ref(exe_ref, rec, c["rho_scale"], c["v_thresh"], c["a_thresh"], **kw)
    host = crafted.host_run(exe_host, rec, c["rho_scale"], c["v_thresh"], c["a_thresh"], **kw)
    problems = []
    if host["segments"].tobytes() != ref["segments"].tobytes():
        problems.append("segments differ")
    for key in ("dpose", "dpos", "flags"):
        for v, (a, b) in enumerate(zip(host[key], ref[key])):
            if a.tobytes() != b.tobytes():
                problems.append(f"{key} of view {v} differ")
    if host["s_num"] != ref["s_num"]:
        problems.append(f"s_num: host {host['s_num']} reference {ref['s_num']}")
    for name, a, b in zip(("rho", "s_rho", "fixed"), host["fill"], ref["fill"]):
        if a.tobytes() != b.tobytes():
            problems.append(f"fill {name} differ in cells {np.nonzero(a.view(np.int64 if a.dtype == np.float64 else np.uint8) != b.view(np.int64 if b.dtype == np.float64 else np.uint8))[0][:8].tolist()}")
    size, block = kw.get("size", (crafted.W, crafted.H)), kw.get("block", (crafted.BW, crafted.BH))
    ch = port.chain(ref["fill"][0], ref["fill"][1], ref["fill"][2].astype(bool), size[0], size[1], block[0], block[1],
                    kw.get("iter_num", crafted.ITER_NUM), kw.get("bound_mode", crafted.BOUND_MODE))
    for name, a, b in zip(("rho", "s_rho", "fixed"), ch, ref["chain"]):
        if np.ascontiguousarray(a).reshape(-1).astype(b.dtype).tobytes() != b.tobytes():
            problems.append(f"chain {name} differ")
    if problems:
        raise SystemExit(f"{tag}: REFUSED: " + "; ".join(problems))
    arrays[f"{tag}__records"] = np.frombuffer(np.ascontiguousarray(rec).tobytes(), np.uint8).reshape(-1, 5)
    arrays[f"{tag}__params"] = np.array([c["rho_scale"], c["v_thresh"], c["a_thresh"]], np.float64)
    arrays[f"{tag}__segments"] = ref["segments"]
    arrays[f"{tag}__dpose"] = np.array(ref["dpose"]).reshape(-1, 3, 3)
    arrays[f"{tag}__dpos"] = np.array(ref["dpos"]).reshape(-1, 3)
    arrays[f"{tag}__flags"] = np.array(ref["flags"], np.uint8).reshape(len(ref["flags"]), -1)
    arrays[f"{tag}__s_num"] = np.array(ref["s_num"], np.int32)
    for k, part in (("fill", ref["fill"]), ("chain", ref["chain"])):
        for name, a in zip(("rho", "s_rho", "fixed"), part):
            arrays[f"{tag}__{k}_{name}"] = a
    rho = np.asarray(rec["rho"], np.int32)
    n, g = len(rho), host["gates"]
    starts = [i for i in range(n - 1) if rho[i] != 0 and not (rho[i] < 0 and i >= 1 and rho[i - 1] > 0)]
    pop["segments"] += len(ref["segments"])
    pop["shared_vertex"] += sum(1 for i in starts if rho[i] > 0 and rho[i + 1] > 0 and i + 1 in starts)
    pop["closing_k1"] += sum(1 for i in starts if rho[i] > 0 and rho[i + 1] < 0)
    pop["negative_k0"] += sum(1 for i in starts if rho[i] < 0)
    pop["partner_self"] += sum(1 for i in starts if rho[i] < 0 or rho[i + 1] == 0)
    pop["s_rho_floor"] += int((ref["segments"][:, [3, 7]] == np.float32(1e-3)).sum())
    for k, v in (("folded", 0), ("gate_sigma", 1), ("gate_sum", 2), ("gate_rel", 3), ("gate_angle", 4), ("degenerate", 5)):
        pop[k] += int((g == v).sum())
    prev = np.ones(len(ref["segments"]), np.uint8)
    for v, f in enumerate(ref["flags"]):
        pop["hidden"] += int(((prev == 1) & (f == 0)).sum())
        pop["kept"] += int(((prev == 1) & (f == 1)).sum())
        pop["already_hidden"] += int((prev == 0).sum())
        if v == 2:
            pop["behind"] += int(((prev == 1) & (f == 1)).sum())
        prev = f
    pop["fixed_cells"] += int(ref["chain"][2].sum())
    return len(ref["segments"]), int(ref["fill"][2].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REBVO_REF", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(crafted.GOLD, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe_ref = build_driver(a.ref, tmp)
        exe_host = crafted.build_host_tool(tmp)
        arrays, pop, counts = {}, dict.fromkeys(POPULATIONS, 0), {}
        for name in crafted.names():
            counts[name] = one_case(name, crafted.case(name), exe_ref, exe_host, arrays, pop)
        empty = [k for k, v in pop.items() if v == 0]
        if empty:
            raise SystemExit(f"crafted: REFUSED: empty populations {empty}")
        if arrays["cross_ab__fill_rho"].tobytes() == arrays["cross_ba__fill_rho"].tobytes():
            raise SystemExit("crafted: REFUSED: the two list orders of the crossing segments give the same grid")
        arrays["names"] = np.array(crafted.names())
        arrays["camera"] = np.array(crafted.CAM, np.float64)
        arrays["geometry"] = np.array([crafted.W, crafted.H, crafted.BW, crafted.BH, crafted.ITER_NUM, crafted.BOUND_MODE], np.int32)
        arrays["em_nav"] = crafted.EM_NAV
        arrays["views"] = np.array(crafted.VIEWS, np.float32)
        path = os.path.join(crafted.GOLD, "crafted.npz")
        np.savez_compressed(path, **arrays)
        print(f"{path}: {os.path.getsize(path)} bytes\n  (segments, fixed cells) {counts}\n  populations {pop}")

        g = np.load(os.path.join(ROOT, "tests", "golden", "edgemap", "billboard.npz"))
        frames = np.load(os.path.join(ROOT, "tests", "golden", "billboard_256x192.npz"))["frames"]
        _, h, w = frames.shape
        cam = tuple(float(v) for v in g["camera"])
        arrays, pop, counts = {}, dict.fromkeys(POPULATIONS, 0), {}
        for k, (bw, bh, iters, mode) in BILLBOARD.items():
            rec = np.frombuffer(np.ascontiguousarray(g[f"frame{k}__records"]).tobytes(), crafted.edgehip.COMPRESSED_KL_DTYPE)
            scale = float(np.float32(g[f"frame{k}__params"][5]))     # rho_scale=scale: the double narrowed to float
            c = dict(records=rec, rho_scale=scale, v_thresh=BILLBOARD_THRESH[0], a_thresh=BILLBOARD_THRESH[1])
            tag = f"frame{k}"
            counts[k] = one_case(tag, c, exe_ref, exe_host, arrays, pop, size=(w, h), block=(bw, bh), cam=cam, iter_num=iters, bound_mode=mode)
            arrays[f"{tag}__geometry"] = np.array([w, h, bw, bh, iters, mode], np.int32)
        if pop["fixed_cells"] <= 50 or pop["folded"] == 0 or pop["hidden"] == 0:
            raise SystemExit(f"billboard: REFUSED: populations {pop}")
        arrays["frames"] = np.array(list(BILLBOARD))
        arrays["camera"] = np.array(cam, np.float64)
        arrays["em_nav"] = crafted.EM_NAV
        arrays["views"] = np.array(crafted.VIEWS, np.float32)
        path = os.path.join(crafted.GOLD, "billboard.npz")
        np.savez_compressed(path, **arrays)
        print(f"{path}: {os.path.getsize(path)} bytes\n  (segments, fixed cells) {counts}\n  populations {pop}")


if __name__ == "__main__":
    main()
