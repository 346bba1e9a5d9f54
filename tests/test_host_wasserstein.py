"""csrc/wasserstein_core.h on the CPU (tests/host/host_wasserstein.cpp, a stand-alone program with its own main): the split plan
covers 0 .. K - 1 exactly once for every K around the chunk, and the per-element routine - term, the fixed summation tree, every
split a launch may choose, the division and the root - reproduces the exact dyadic-grid answers bit for bit and stays within the
bar of the fsum reference on real-valued rows; built plain and with the address and undefined-behaviour sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import wasserstein_checks as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "host_wasserstein.cpp")
CORE = os.path.join(ROOT, "code-robchar_amd", "csrc", "wasserstein_core.h")
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"]
PLAN_K = (1, 2, wc.CHUNK - 1, wc.CHUNK, wc.CHUNK + 1, 3 * wc.CHUNK + 5, 1024, 4096, 4097, 10000)


def cases():
    """(p, exact, a, b, want)"""
    out = []
    for K in (1, 2, 7, 255, 256, 257, 773, 1025, 4096):
        ra, rb = wc.grid_rows(1, K, 100 + K), wc.grid_rows(1, K, 200 + K)
        for p in (1, 2):
            out.append((p, 1, wc.grid_values(ra)[0], wc.grid_values(rb)[0], wc.grid_answer(ra, rb, p)[0, 0]))
    ra = wc.grid_rows(1, 300, 7)
    shift = ra + 12345
    for p in (1, 2):
        out.append((p, 1, wc.grid_values(ra)[0], wc.grid_values(ra)[0], 0.0))                                     # b = a
        out.append((p, 1, wc.grid_values(ra)[0], wc.grid_values(shift)[0], 12345 * 2.0 ** -wc.GRID))              # b = a + c
        out.append((p, 1, np.full(513, 0.25), np.full(513, 0.875), 0.625))                                        # constant rows
    for K in (1, 5, 300, 4097, 10000):
        a, b = np.sort(wc.beta_rows(1, K, K)[0]), np.sort(wc.beta_rows(1, K, K + 1, (2.0, 2.0))[0])
        for p in (1, 2):
            out.append((p, 0, a, b, wc.wd.pair_reference(a, b, p)))
    nan = np.sort(wc.beta_rows(1, 300, 9)[0])
    nan[-1] = np.nan
    out.append((1, 0, nan, np.sort(wc.beta_rows(1, 300, 10)[0]), float("nan")))
    return out


def write_cases(path, todo, plan_k=PLAN_K):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(plan_k)) + struct.pack("<%dq" % len(plan_k), *plan_k))
        f.write(struct.pack("<q", len(todo)))
        for p, exact, a, b, want in todo:
            f.write(struct.pack("<qqqd", p, len(a), exact, want))
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes() + np.ascontiguousarray(b, dtype="<f8").tobytes())


@pytest.mark.parametrize("extra", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_core_reproduces_the_known_answers(tmp_path, extra):
    todo = cases()
    path = tmp_path / "cases.bin"
    write_cases(path, todo)
    exe = tmp_path / "host_wasserstein"
    subprocess.run(FLAGS + extra + ["-o", str(exe), SRC], check=True)
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "OK" and len(lines) == len(PLAN_K) + len(todo) + 1, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("old, new, symptom", [
    ("        return e < K ? e : K;\n", "        return e < K ? e : K - 1;\n", "differs"),                        # the last value of k dropped
    ("    const double m = sum / (double)K;\n", "    const double m = sum;\n", "differs"),                         # no division
    ("    if (P == 1) return acc + fabs(d);\n", "    if (P == 1) return acc + d;\n", "differs"),                   # no absolute value
])
def test_the_program_sees_a_difference(tmp_path, old, new, symptom):
    """the comparison in the program is live: with a broken core header it reports a difference"""
    text = open(SRC).read().replace('#include "../../code-robchar_amd/csrc/wasserstein_core.h"', '#include "wasserstein_core.h"')
    core = open(CORE).read()
    assert old in core
    (tmp_path / "wasserstein_core.h").write_text(core.replace(old, new))
    (tmp_path / "host_wasserstein.cpp").write_text(text)
    exe = tmp_path / "host_wasserstein"
    subprocess.run(FLAGS + ["-o", str(exe), str(tmp_path / "host_wasserstein.cpp")], check=True)
    path = tmp_path / "cases.bin"
    write_cases(path, cases())
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and symptom in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
