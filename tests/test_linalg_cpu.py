"""CPU: rebvo/linalg.h, the one statement of the 6x6 / 3x3 algebra and the SO(3) maps for host and device, against what the tracker's
and the frame glue's former private copies gave (tests/golden/linalg/linalg_check.txt, made once at the commit before they were deleted:
DESIGN.md, "One copy of the algebra").  tools/linalg_check.cpp is a stand-alone program built here with the host compiler; every number
is compared bit for bit (hex doubles).  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "linalg", "linalg_check.txt")
# the rows that come from the header's side, not from stage C's former so3_ln: above 135 degrees TooN ends with unit(r2) * angle, the copy
# ended with angle * (r2 / |r2|), one rounding apart
LN_FAR_ROWS = ("ln_far_above_135deg.w", "ln_far_x_dominant.w", "ln_far_y_dominant.w", "ln_far_z_dominant.w", "ln_far_sign_flip.w")


def _rows(text):
    rows = {}
    for line in text.strip().splitlines():
        name, *vals = line.split()
        assert name not in rows, name
        rows[name] = vals
    return rows


def _build_and_run(tmp_path, tag, extra):
    exe = tmp_path / ("linalg_check_" + tag)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra +
                   ["-I" + os.path.join(ROOT, "rebvo_amd", "host", "include"), os.path.join(ROOT, "tools", "linalg_check.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stderr == "", p.stderr[-2000:]     # a sanitizer report that does not stop the program still fails the test
    return _rows(p.stdout)


@pytest.mark.parametrize("tag,extra", [("plain", []), ("asan_ubsan", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_linalg_header_bit_for_bit(tmp_path, tag, extra):
    want = _rows(open(GOLD).read())
    got = _build_and_run(tmp_path, tag, extra)
    assert set(LN_FAR_ROWS) <= set(want)
    assert len(want) == 151 and list(got) == list(want)
    for n in ("chol3", "chol6", "chol7"):       # every case of the list is in the fixture
        for case in ("cond0", "cond1", "cond2", "negative_pivot", "nan_entry"):
            assert all(f"{n}_{case}.{what}" in want for what in ("L", "backsub", "inverse")), (n, case)
        assert sum(k.startswith(n + "_zero_pivot_col") for k in want) == 9
    assert sum(k.startswith("svd6_") for k in want) == 3 * 15 and sum(k.startswith("svd7_") for k in want) == 6
    assert sum(k.startswith("exp_") for k in want) == 8 and sum(k.startswith("ln_") for k in want) == 10 and sum(k.startswith("inv3_") for k in want) == 10
    bad = [(k, i, got[k][i], want[k][i]) for k in want for i in range(max(len(want[k]), len(got[k])))
           if i >= len(got[k]) or i >= len(want[k]) or got[k][i] != want[k][i]]
    assert bad == [], bad[:8]
