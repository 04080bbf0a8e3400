"""The wide field's training entry points (fetode_wide_dopri5_tape, fetode_wide_dopri5_backward,
fetode_wide_dopri5_backward_workspace): declared in include/fetode.h, exported by libfetode.so and
bound in _lib.SIGNATURES with the header's argument counts; the switch is off by default.  Host
code only: no GPU."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "fetode.h")
LIB = os.path.join(REPO, "fet-ode_amd", "libfetode.so")

# name -> arguments in the header
NEW = {"fetode_wide_dopri5_tape": 28, "fetode_wide_dopri5_backward_workspace": 6, "fetode_wide_dopri5_backward": 30}


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/fetode.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", list(NEW))
def test_declared_exported_and_bound(name):
    import fet_ode_amd
    args = _header_args(name)
    assert len(args) == NEW[name], args
    res, bound = fet_ode_amd._lib.SIGNATURES[name]
    assert len(bound) == len(args), (len(bound), len(args))
    assert os.path.exists(LIB), "libfetode.so is not built (__graft_entry__.build())"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    assert re.search(r"\bT " + name + r"\b", out), f"{name} is not exported"


def test_tape_is_the_untaped_signature_plus_three():
    import fet_ode_amd
    S = fet_ode_amd._lib.SIGNATURES
    base, tape = S["fetode_wide_dopri5"][1], S["fetode_wide_dopri5_tape"][1]
    assert tape[:len(base) - 1] == base[:-1] and tape[-1] == base[-1] and len(tape) == len(base) + 3
    assert _header_args("fetode_wide_dopri5_tape")[-4:-1] == ["float* tape", "int64_t tape_cap", "double* init_rec"]


def test_switch_exists_and_is_off_by_default():
    from fet_ode_amd import dopri5
    default = os.environ.get("FETODE_WIDE_DOPRI5_TAPE", "0") == "1"   # off unless the environment asks
    prev = dopri5.set_resident_wide_training(False)
    try:
        assert prev is default
        assert dopri5.set_resident_wide_training(True, tape_bytes=1 << 20) is False
        assert dopri5.set_resident_wide_training(False, tape_bytes=16 << 30) is True
    finally:
        dopri5.set_resident_wide_training(prev, tape_bytes=16 << 30)
