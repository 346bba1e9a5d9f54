"""The BOXED row step of csrc/lbfgs_core.h - init_row_box, the three objective kinds, advance_row_box: the text the device kernels
run - on the CPU (tests/host/host_lbfgs_box.cpp, a stand-alone program with its own main) against code-robchar_amd/lbfgs.py, the
definition: every state field and the trial points after every call, bit for bit, on the cases of lbfgs_box_checks.identity_case
(rows on bounds, infinite sides, a row with bad bounds) written to a file; built plain and with the address and
undefined-behaviour sanitizers (host code only: nothing is loaded into Python under a sanitizer)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import lbfgs_box_checks as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "host_lbfgs_box.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]
CASES = [(n, m, kind) for n in (3, 8, 13) for m in (1, 3, 8) for kind in (0, 1, 2)]


def write_case(f, case, has_mask=1):
    p = case["params"]
    f.write(struct.pack("<8q4d", case["C"], case["n"], case["m"], case["kind"], len(case["calls"]), p["maxiter"], p["maxback"], has_mask,
                        case["lam"], p["c1"], p["gtol"], p["ftol"]))
    for arr in (case["x0"], case["mask"], case["lo"], case["hi"]) + tuple(case["init"]):
        f.write(np.ascontiguousarray(arr, dtype="<f8").tobytes())
    for call in case["calls"]:
        for arr in call:
            f.write(np.ascontiguousarray(arr, dtype="<f8").tobytes())


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("hostlbfgsbox") / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(CASES)))
        for n, m, kind in CASES:
            case = bc.identity_case(n, m, kind, C=9)
            assert len(set(case["status"])) >= 3 and case["status"][3] == 5 and case["status"][5] == 5, case["status"]
            assert case["counters"]["on_bound"] > 0 and case["counters"]["rejected"] > 0, case["counters"]
            write_case(f, case)
    return str(path), len(CASES)


@pytest.mark.parametrize("extra", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_core_equals_definition(case_file, tmp_path, extra):
    path, n = case_file
    exe = tmp_path / "host_lbfgs_box"
    subprocess.run(FLAGS + extra + ["-o", str(exe), SRC], check=True)
    out = subprocess.run([str(exe), path], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "OK" and len(lines) == n + 1, out.stdout[-2000:] + out.stderr[-2000:]


def test_the_program_sees_a_difference(tmp_path):
    """the comparison in the program is live: with a projection that forgets the upper bound it reports a difference"""
    text = open(SRC).read().replace('#include "../../code-robchar_amd/csrc/lbfgs_core.h"', '#include "lbfgs_core.h"')
    core = open(os.path.join(ROOT, "code-robchar_amd", "csrc", "lbfgs_core.h")).read()
    good = "return v < lo ? lo : (v > hi ? hi : v);"
    assert core.count(good) == 1
    (tmp_path / "lbfgs_core.h").write_text(core.replace(good, "return v < lo ? lo : v;"))
    (tmp_path / "host_lbfgs_box.cpp").write_text(text)
    exe = tmp_path / "host_lbfgs_box"
    subprocess.run(FLAGS + ["-o", str(exe), str(tmp_path / "host_lbfgs_box.cpp")], check=True)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<q", 1))
        write_case(f, bc.identity_case(8, 3, 1, C=9))
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "differs" in out.stdout, out.stdout + out.stderr
