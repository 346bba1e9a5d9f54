"""The per-lane functions of csrc/bootstrap_core.h - counter layout, index rule, accumulation order, butterfly, finish, summary -
run on the CPU as the kernels run them (tests/host/host_bootstrap.cpp, a stand-alone program with its own main) against the NumPy
definition (bootstrap.py) on the inputs of tests/bootstrap_checks.py written to a file; built plain and with the address and
undefined-behaviour sanitizers."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bootstrap_checks as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "host_bootstrap.cpp")
FLAGS = ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"]


def cases():
    """(F, B, seed, offset, thresholds, conf)"""
    out = [(bc.exact_rows(), 33, 0x5EED0001, 0, (0.25, 0.5, 0.95), 0.95),
           (np.full((2, 100), 0.75), 20, 3, 0, (0.75, 0.76), 0.95),
           (np.where(np.arange(602).reshape(2, 301) % 3 == 0, 0.99, 0.5), 40, 9, 11, (0.99, 0.5, 0.995), 0.95)]
    out += [(bc.ragged_fid(K), B, 21, 7, bc.Q, 0.95) for K in bc.RAGGED_K for B in (1, 5, 67)]
    out += [(bc.exact_rows(C=2, seed=6), 5, 0xABCDEF0123456789, off, (), 0.9) for off in (2 ** 40, 2 ** 32 - 3, 2 ** 64 - 2 * 5 * 64)]
    out.append((np.random.default_rng(8).beta(8.0, 2.0, (5, 128)), 400, 31, 0, bc.Q, 0.95))
    out.append((np.random.default_rng(9).random((1, 2500)), 3, 1, 5, (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8), 0.5))     # > 1024: two values per thread
    return out


def write_cases(path, todo):
    with open(path, "wb") as f:
        f.write(struct.pack("<q", len(todo)))
        for F, B, seed, offset, thr, conf in todo:
            F = np.ascontiguousarray(F, dtype="<f8")
            res = bc.boot.bootstrap_metrics(F, B, seed, offset, thr, conf)
            lo, hi = bc.boot.ranks(B, conf)
            f.write(struct.pack("<qqqQQq", F.shape[0], F.shape[1], B, seed, offset, len(thr)))
            f.write(np.asarray(thr, dtype="<f8").tobytes() + struct.pack("<qq", lo, hi) + F.tobytes())
            f.write(np.ascontiguousarray(res["replicates"], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(res["summary"], dtype="<f8").tobytes())


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("hostbootstrap") / "cases.bin"
    todo = cases()
    write_cases(path, todo)
    return str(path), len(todo)


@pytest.mark.parametrize("extra", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_wave_emulation_equals_the_definition(case_file, tmp_path, extra):
    path, n = case_file
    exe = tmp_path / "host_bootstrap"
    subprocess.run(FLAGS + extra + ["-o", str(exe), SRC], check=True)
    out = subprocess.run([str(exe), path], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "OK" and len(lines) == n + 1, out.stdout[-2000:] + out.stderr[-2000:]


def test_the_program_sees_a_difference(tmp_path):
    """the comparison in the program is live: with a counter that ignores the replicate number it reports a difference"""
    text = open(SRC).read().replace('#include "../../code-robchar_amd/csrc/bootstrap_core.h"', '#include "bootstrap_core.h"')
    core = open(os.path.join(ROOT, "code-robchar_amd", "csrc", "bootstrap_core.h")).read()
    assert "    return offset + (c * B + b) * Q;\n" in core
    (tmp_path / "bootstrap_core.h").write_text(core.replace("    return offset + (c * B + b) * Q;\n", "    return offset + (c * B + 0 * b) * Q;\n"))
    (tmp_path / "host_bootstrap.cpp").write_text(text)
    exe = tmp_path / "host_bootstrap"
    subprocess.run(FLAGS + ["-o", str(exe), str(tmp_path / "host_bootstrap.cpp")], check=True)
    path = tmp_path / "cases.bin"
    write_cases(path, cases()[:1])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "differs" in out.stdout, out.stdout + out.stderr
