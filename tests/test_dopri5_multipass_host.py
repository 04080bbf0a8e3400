"""Host side of the multi-pass mode of the resident LV dopri5 launches (fetode_dopri5_set_multipass,
fetode_dopri5_set_grid_limit, fetode_integrate_dopri5_multipass_max_batch): the exports, the
switches' defaults and return values, the workspace sizes, and the Python routing's refusals — all
of it before any device call, so none of this needs a GPU."""
import ctypes

import pytest

FAKE = 0x1000


def _field(L, H=10, K=10, ferro=True, branch_sign=False):
    """A [2, H, 2] descriptor with fake device pointers (never dereferenced by the queries)."""
    kan = (L.KANLinearDesc * 2)()
    fer = (L.FerroDesc * 2)()
    for l, (i, o) in enumerate(((2, H), (H, 2))):
        kan[l] = L.KANLinearDesc(i, o, 5, 3, 10, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0)
        fer[l] = L.FerroDesc(i, o, K, FAKE, FAKE, FAKE, FAKE, FAKE, 10.0, 0.8, FAKE if branch_sign else None, 0)
    f = L.FieldDesc(2, kan, fer if ferro else None)
    f._keep = (kan, fer)
    return f


@pytest.fixture
def lib_off():
    """The library with the switch off and no limit; both restored afterwards."""
    import fet_ode_amd as F
    lib = F._lib.load()
    mp = lib.fetode_dopri5_set_multipass(0)
    lim = lib.fetode_dopri5_set_grid_limit(0)
    yield F._lib, lib
    lib.fetode_dopri5_set_multipass(mp)
    lib.fetode_dopri5_set_grid_limit(lim)


def test_symbols_exported_with_declared_argtypes():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    want = {"fetode_dopri5_set_multipass": (ctypes.c_int, [ctypes.c_int]),
            "fetode_dopri5_set_grid_limit": (ctypes.c_int64, [ctypes.c_int64]),
            "fetode_integrate_dopri5_multipass_max_batch": (ctypes.c_int64, [ctypes.POINTER(L.FieldDesc)])}
    for name, (res, args) in want.items():
        assert L.SIGNATURES[name] == (res, args)
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args


def test_switch_defaults_off_and_setters_return_previous():
    import os
    import subprocess
    import sys
    # the default comes from the environment of a fresh process: off, unless FETODE_DOPRI5_MULTIPASS=1
    code = ("import fet_ode_amd as F; l = F._lib.load(); "
            "print(l.fetode_dopri5_set_multipass(-1), l.fetode_dopri5_set_grid_limit(0))")
    for env, want in ((None, "0 0"), ("1", "1 0"), ("0", "0 0")):
        e = {k: v for k, v in os.environ.items() if k != "FETODE_DOPRI5_MULTIPASS"}
        if env is not None:
            e["FETODE_DOPRI5_MULTIPASS"] = env
        e["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p])
        out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True)
        assert out.stdout.split("\n")[-2].strip() == want, (env, out.stdout)


def test_setters_return_previous(lib_off):
    L, lib = lib_off
    assert lib.fetode_dopri5_set_multipass(1) == 0
    assert lib.fetode_dopri5_set_multipass(-1) == 1     # a negative argument only queries
    assert lib.fetode_dopri5_set_multipass(0) == 1
    assert lib.fetode_dopri5_set_multipass(-1) == 0
    assert lib.fetode_dopri5_set_grid_limit(5) == 0
    assert lib.fetode_dopri5_set_grid_limit(-3) == 5    # anything below 1 is "occupancy only"
    assert lib.fetode_dopri5_set_grid_limit(0) == 0
    from fet_ode_amd.dopri5 import set_resident_dopri5_multipass
    assert set_resident_dopri5_multipass(True) is False
    assert set_resident_dopri5_multipass(False) is True
    assert lib.fetode_dopri5_set_multipass(-1) == 0
    assert lib.fetode_integrate_dopri5_backward_set_shape(2) == 0
    assert lib.fetode_integrate_dopri5_backward_set_shape(7) == 2    # not a shape: a query
    assert lib.fetode_integrate_dopri5_backward_set_shape(0) == 2


def test_max_batch_by_shape(lib_off):
    L, lib = lib_off
    mb = lib.fetode_integrate_dopri5_multipass_max_batch
    cap = (1 << 31) // 14      # the sweep's 32-bit tape-row offsets: b * 14 + c < 2^31 for b < cap
    assert (cap - 1) * 14 + 13 < (1 << 31) <= cap * 14 + 13
    assert mb(ctypes.byref(_field(L))) == cap                          # LV KAN-FET [2, 10, 2]
    assert mb(ctypes.byref(_field(L, ferro=False))) == cap             # LV KAN [2, 10, 2]
    assert mb(ctypes.byref(_field(L, H=12))) == 0                      # a fieldn width
    assert mb(ctypes.byref(_field(L, branch_sign=True))) == 0          # explicit branch_sign
    assert mb(None) == 0
    lib.fetode_dopri5_set_multipass(1)                                 # independent of the switch
    assert mb(ctypes.byref(_field(L))) == cap


def test_capacity_exports_answer_without_a_device(lib_off):
    """The capacity exports size their answer by the device's resident workgroups; with no device the
    query fails and they answer 0 (or a negative value, ECG) instead of crashing.  With a device every
    one of them is positive."""
    import torch
    L, lib = lib_off
    fields = (_field(L), _field(L, ferro=False), _field(L, H=12), _field(L, H=12, ferro=False))
    fwd = [lib.fetode_integrate_dopri5_max_batch(ctypes.byref(f), s) for f in fields for s in (0, 1)]
    bwd = [lib.fetode_integrate_dopri5_backward_max_batch(ctypes.byref(f)) for f in fields]
    layer = L.HLogisticDesc(8, 10, FAKE, FAKE, FAKE, FAKE, 5.0, 0.5)
    ecg = lib.fetode_ecg_dopri5_backward_max_batch(ctypes.byref(layer))
    if torch.cuda.is_available():
        assert min(fwd) > 0 and min(bwd) > 0 and ecg > 0, (fwd, bwd, ecg)
    else:
        assert fwd == [0] * 8, fwd
        assert bwd == [0] * 4, bwd
        assert ecg <= 0, ecg


def test_workspace_includes_parking_only_when_on(lib_off):
    L, lib = lib_off
    ws = lib.fetode_integrate_dopri5_workspace
    off = [ws(B) for B in (1, 7, 4096, 8192)]
    lib.fetode_dopri5_set_grid_limit(3)          # the limit alone changes nothing
    assert [ws(B) for B in (1, 7, 4096, 8192)] == off
    lib.fetode_dopri5_set_multipass(1)
    for B, o in zip((1, 7, 4096, 8192), off):
        assert ws(B) - o == 5 * 64 * 4 * ((B + 1) // 2)      # (virtual grid, 5, 64) floats
    lib.fetode_dopri5_set_multipass(0)
    assert [ws(B) for B in (1, 7, 4096, 8192)] == off


def test_python_routing_declines_beyond_the_cap_while_off(lib_off):
    """_resident_cap: with the switch off the one-grid cap stands; on, the multi-pass cap replaces it
    for a field that has the mode and changes nothing for one that has not."""
    L, lib = lib_off
    from fet_ode_amd.dopri5 import _resident_cap

    class H:
        def __init__(self, f):
            self.ref = ctypes.byref(f)

    lv, wide = H(_field(L)), H(_field(L, H=12))
    assert _resident_cap(lib, lv, 4096) == 4096
    assert _resident_cap(lib, wide, 4096) == 4096
    lib.fetode_dopri5_set_multipass(1)
    assert _resident_cap(lib, lv, 4096) == (1 << 31) // 14
    assert _resident_cap(lib, wide, 4096) == 4096


def test_refusals_before_any_device_call(lib_off):
    L, lib = lib_off
    lib.fetode_dopri5_set_multipass(1)
    lib.fetode_dopri5_set_grid_limit(1)
    opts = (ctypes.c_double * 7)(0.0, 0.9, 10.0, 0.2, 0.0, float("inf"), 1e9)
    tab = (ctypes.c_float * 50)()
    f = _field(L)
    # null pointers are refused with the switch on as with it off
    rc = lib.fetode_integrate_dopri5(ctypes.byref(f), FAKE, None, 7, FAKE, 3, 1e-3, 1e-4, opts, tab, FAKE, FAKE, 3,
                                     FAKE, FAKE, FAKE, 16, None)
    assert rc == L.FETODE_EINVAL and b"null" in lib.fetode_last_error()
    rc = lib.fetode_integrate_dopri5_tape(ctypes.byref(f), FAKE, FAKE, 7, FAKE, 3, 1e-3, 1e-4, opts, tab, FAKE, FAKE,
                                          3, FAKE, FAKE, FAKE, 16, None, 64, FAKE, None)
    assert rc == L.FETODE_EINVAL and b"tape" in lib.fetode_last_error()
    rc = lib.fetode_integrate_dopri5_backward(ctypes.byref(f), FAKE, 7, FAKE, 3, 1e-3, 1e-4, opts, tab, FAKE, FAKE, 9,
                                              FAKE, 1, FAKE, FAKE, 3, FAKE, None, None, FAKE, FAKE, None)
    assert rc == L.FETODE_EINVAL and b"attempts" in lib.fetode_last_error()    # 9 != 2 + 6 * 1
    # an empty batch is a no-op in either mode
    assert lib.fetode_integrate_dopri5(ctypes.byref(f), FAKE, FAKE, 0, FAKE, 3, 1e-3, 1e-4, opts, tab, FAKE, FAKE, 3,
                                       FAKE, FAKE, FAKE, 16, None) == L.FETODE_OK
