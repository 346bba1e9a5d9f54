"""The per-element functions of csrc/select_core.h - key, digit, histogram walk, take rule, slot - in a serial select on the CPU
(tests/host/host_tail_select.cpp, a stand-alone program with its own main) against std::stable_sort, on the inputs of
tests/tail_select_checks.py written to a file; built plain and with the address and undefined-behaviour sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tail_select_checks as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "host_tail_select.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"]


def cases():
    out = []
    for K in tc.RANDOM_K:
        F = tc.random_rows(K)()
        out += [(F, a) for a in tc.random_alphas(K)]
    out.append((tc.random_rows(1000, C=1)(), 0.1))
    out.append((tc.random_rows(100, C=64)(), 0.1))
    out += [(tc.tie_rows(K)(), a) for K, a in tc.TIE_CASES]
    out += [(np.full((2, 1024), 0.75), m / 1024.0) for m in tc.CONSTANT_M]
    out.append((tc.last_digit_rows(), 0.1))
    out += [(tc.special_rows(), a) for a in tc.SPECIAL_ALPHAS]
    return out


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("hosttailselect") / "cases.bin"
    todo = cases()
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(todo)))
        for F, alpha in todo:
            F = np.ascontiguousarray(F, dtype="<f8")
            f.write(struct.pack("<qqd", F.shape[0], F.shape[1], alpha))
            f.write(F.tobytes())
    return str(path), len(todo)


@pytest.mark.parametrize("extra", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_serial_select_equals_stable_sort(case_file, tmp_path, extra):
    path, n = case_file
    exe = tmp_path / "host_tail_select"
    subprocess.run(FLAGS + extra + ["-o", str(exe), SRC], check=True)
    out = subprocess.run([str(exe), path], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "OK" and len(lines) == n + 1, out.stdout[-2000:] + out.stderr[-2000:]


def test_the_program_sees_a_difference(tmp_path):
    """the comparison in the program is live: with a key that does not make -0.0 equal to +0.0 it reports a difference"""
    text = open(SRC).read().replace('#include "../../code-robchar_amd/csrc/select_core.h"', '#include "select_core.h"')
    core = open(os.path.join(ROOT, "code-robchar_amd", "csrc", "select_core.h")).read()
    assert "    if (x == 0.0) u = 0ull;\n" in core
    (tmp_path / "select_core.h").write_text(core.replace("    if (x == 0.0) u = 0ull;\n", ""))
    (tmp_path / "host_tail_select.cpp").write_text(text)
    exe = tmp_path / "host_tail_select"
    subprocess.run(FLAGS + ["-o", str(exe), str(tmp_path / "host_tail_select.cpp")], check=True)
    path = tmp_path / "cases.bin"
    F = tc.special_rows()
    with open(path, "wb") as f:
        f.write(struct.pack("<qqqd", 1, F.shape[0], F.shape[1], 0.2) + np.ascontiguousarray(F, dtype="<f8").tobytes())
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "differs" in out.stdout, out.stdout + out.stderr
