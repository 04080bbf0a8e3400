"""The C-ABI library builds for gfx950, loads, and exports exactly what include/fetode.h declares.
Host-only entry points (sizes, shape validation) are exercised without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "fetode.h")
LIB = os.path.join(REPO, "fet-ode_amd", "libfetode.so")


def declared_symbols():
    src = open(HDR).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fetode_[a-z_0-9]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "fet-ode_amd", "csrc")], check=True)
    return ctypes.CDLL(LIB)


def test_exports_every_declared_symbol(lib):
    syms = declared_symbols()
    assert len(syms) >= 10
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (fetode_\w+)", out))
    assert set(syms) <= exported, set(syms) - exported
    for s in syms:
        getattr(lib, s)


def test_python_binding_covers_header():
    import fet_ode_amd
    assert set(declared_symbols()) == set(fet_ode_amd._lib.SIGNATURES)


def test_gfx950_code_object_present():
    """The offload bundle names its target (amdgcn-amd-amdhsa--gfx950)."""
    assert b"gfx950" in open(LIB, "rb").read()


def _lv_field(F, with_ferro=True):
    """Descriptors with fake non-null device pointers: only host code runs."""
    L = F._lib
    fake = 0x1000
    kan = [L.KANLinearDesc(2, 10, 5, 3, 10, 0, *[fake] * 8, 1.0),
           L.KANLinearDesc(10, 2, 5, 3, 10, 0, *[fake] * 8, 1.0)]
    fer = [L.FerroDesc(2, 10, 10, *[fake] * 5, 10.0, 0.8, None, 0),
           L.FerroDesc(10, 2, 10, *[fake] * 5, 10.0, 0.8, None, 0)] if with_ferro else None
    return L.FieldHandle(kan, fer, [])


def test_host_queries_without_gpu():
    import fet_ode_amd as F
    lib = F._lib.load()
    h = _lv_field(F)
    assert lib.fetode_state_width(h.ref) == 12
    nb = lib.fetode_plan_bytes(h.ref)
    # per layer (fetode_common.h LayerPlan): 4*in*out*K + out + out*in*(1+nb) + 2*in*nb
    # + in*12 knots + in*11 spans, pad to 4; + out*in*12*4 spline table + 1 flag, pad to 4
    def lp(i, o):
        n = 4 * i * o * 10 + o + o * i * 11 + 2 * i * 10 + i * 12 + i * 11
        n = (n + 3) // 4 * 4 + o * i * 12 * 4 + 1
        return (n + 3) // 4 * 4
    assert nb == 4 * (lp(2, 10) + lp(10, 2))
    assert lib.fetode_fused_supported(h.ref) == 1
    assert lib.fetode_fused_supported(_lv_field(F, False).ref) == 1
    assert lib.fetode_state_width(_lv_field(F, False).ref) == 0


def test_v8_workgroup_shape_switch(lib):
    """fetode_fused_set_v8_tpb: 1 or 2 sets, anything else only queries; returns the previous value."""
    f = lib.fetode_fused_set_v8_tpb
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int]
    prev = f(-1)
    try:
        assert prev in (1, 2) and f(-1) == prev
        assert f(1) == prev and f(-1) == 1
        for bad in (0, 3, -7, 1 << 20):
            assert f(bad) == 1
        assert f(2) == 1 and f(-1) == 2
        assert f(0) == 2 and f(-1) == 2
    finally:
        f(prev)


def test_backward_tpw_switch():
    """fetode_backward_set_tpw: 0 / 1 / 2 set, anything else only queries, the previous value comes
    back; and the sweep's workspace size follows the forced shape (host code only: at B = 7 one
    trajectory per wave needs 8 partial rows, two per wave 4), the automatic choice being one of the
    two, while the stateless KAN entry, which has the one shape, ignores the knob."""
    import fet_ode_amd as F
    lib = F._lib.load()
    f = lib.fetode_backward_set_tpw
    prev, prev_v7 = f(-1), lib.fetode_backward_set_v7(0)
    try:
        assert prev in (0, 1, 2) and f(-1) == prev
        assert f(1) == prev and f(-1) == 1
        for bad in (-7, 3, 1 << 20):
            assert f(bad) == 1 and f(-1) == 1
        assert f(2) == 1 and f(0) == 2 and f(-1) == 0
        h, hk = _lv_field(F), _lv_field(F, False)
        ws = lib.fetode_integrate_fixed_backward_workspace
        size, size_kan = {}, {}
        for tpw in (0, 1, 2):
            f(tpw)
            size[tpw] = ws(h.ref, F._lib.RK4, 1, 7)
            size_kan[tpw] = ws(hk.ref, F._lib.RK4, 1, 7)
        assert 0 < size[2] < size[1] and size[0] in (size[1], size[2]), size
        assert size_kan[0] > 0 and size_kan[0] == size_kan[1] == size_kan[2], size_kan
    finally:
        f(prev)
        lib.fetode_backward_set_v7(prev_v7)


@pytest.mark.parametrize("env,expect", [(None, 2), ("1", 1), ("2", 2), ("0", 2), ("4", 2), ("x", 2), ("", 2)])
def test_v8_workgroup_shape_env(lib, env, expect):
    """FETODE_V8_TPB is read once at load: 1 or 2 is taken, anything else leaves the default of 2."""
    e = {k: v for k, v in os.environ.items() if k != "FETODE_V8_TPB"}
    if env is not None:
        e["FETODE_V8_TPB"] = env
    code = f"import ctypes; print(ctypes.CDLL({LIB!r}).fetode_fused_set_v8_tpb(-1))"
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    assert int(out) == expect


def test_shape_errors_are_reported():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    fake = 0x1000
    kan = [L.KANLinearDesc(2, 10, 5, 3, 10, 0, *[fake] * 8, 1.0),
           L.KANLinearDesc(9, 2, 5, 3, 10, 0, *[fake] * 8, 1.0)]   # 10 != 9
    h = L.FieldHandle(kan, None, [])
    assert lib.fetode_plan_bytes(h.ref) == -1
    assert b"in_features" in lib.fetode_last_error()
    rc = lib.fetode_integrate_fixed(h.ref, fake, 2, fake, 4, fake, 1, fake, fake, fake, 2, fake, None, 0,
                                    None, None)
    assert rc == L.FETODE_EINVAL
    with pytest.raises(ValueError):
        L.check(rc, "integrate")
