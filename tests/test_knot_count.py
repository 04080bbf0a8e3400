"""The fused kernels' two-level knot count (fet-ode_amd/csrc/fetode_knot_count.h), checked on the
host: tests/knot_count.cpp includes the header, is built host-only with the address and
undefined-behaviour sanitizers, and run as a program of its own.  On sorted knot sets (uniform,
uneven, repeated knots, signed zeros, denormals, +inf padding) the two-level count equals the linear
count at every knot, its two neighbouring floats, +-0, +-inf, NaN, denormals and a sweep across
the set."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_level_count_equals_linear_count(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knot_count")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "fet-ode_amd", "csrc"),
                    os.path.join(REPO, "tests", "knot_count.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
