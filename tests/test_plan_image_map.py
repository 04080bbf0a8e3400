"""The lane map of the fused [2, 10, 2] kernels' plan image (fet-ode_amd/csrc/fetode_fused4_image.h),
checked on the host: tests/plan_image_map.cpp includes the header, is built host-only with the
address and undefined-behaviour sanitizers, and run as a program of its own.  Both variants (3 / 6
lanes per hidden unit) and both fields (KAN-FET K = 10, KAN): every layer-0 Ferro element (o, i, k),
every layer-1 element (o, d, k), every feature weight kw(o, i, ff), every layer-1 feature job of each
hidden unit and every knot is the source of exactly one slot of its owning group; every other slot
is a pad with the documented value; the LDS image holds every table value once."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lane_map_is_a_partition(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "plan_image_map")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "fet-ode_amd", "csrc"),
                    os.path.join(REPO, "tests", "plan_image_map.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "KAN-FET [2,10,2] K=10" in r.stdout and "KAN [2,10,2]" in r.stdout
