"""Host-side queries and argument checks of the ECG dopri5 training entries (fetode_ecg_dopri5_tape,
fetode_ecg_dopri5_backward and its _workspace / _max_batch queries): every refusal here comes
before any device call, so none of this needs a GPU."""
import ctypes

FAKE = 0x1000


def _desc(L, in_dim=4, nb=5, null_param=False):
    return L.HLogisticDesc(in_dim, nb, None if null_param else FAKE, FAKE, FAKE, FAKE, 5.0, 0.5)


def _tape(lib, d, D=4, tape=FAKE, init_rec=FAKE, att=FAKE, y0=FAKE):
    opts = (ctypes.c_double * 7)(0.0, 0.9, 10.0, 0.2, 0.0, float("inf"), 1e9)
    tab = (ctypes.c_float * 50)()
    return lib.fetode_ecg_dopri5_tape(ctypes.byref(d), FAKE, FAKE, D, FAKE, y0, 3, FAKE, 2, 1e-3, 1e-4, opts, tab,
                                      FAKE, FAKE, FAKE, FAKE, FAKE, att, 16, tape, 64, init_rec, None)


def _bwd(lib, d, D=4, n_ev=8, n_att=1, first_step=0.0, tape=FAKE, status=FAKE):
    opts = (ctypes.c_double * 7)(first_step, 0.9, 10.0, 0.2, 0.0, float("inf"), 1e9)
    tab = (ctypes.c_float * 50)()
    return lib.fetode_ecg_dopri5_backward(ctypes.byref(d), FAKE, D, FAKE, 3, FAKE, 2, 1e-3, 1e-4, opts, tab, FAKE,
                                          tape, n_ev, FAKE, n_att, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                          FAKE, status, None)


def test_tape_entry_argument_checks():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    assert _tape(lib, _desc(L, null_param=True)) == L.FETODE_EINVAL
    for kw in ({"tape": None}, {"init_rec": None}, {"att": None}, {"y0": None}):
        assert _tape(lib, _desc(L), **kw) == L.FETODE_EINVAL, kw
    assert b"null" in lib.fetode_last_error()
    assert _tape(lib, _desc(L), D=5) == L.FETODE_EINVAL              # D != in_dim
    assert b"state dim" in lib.fetode_last_error()
    assert _tape(lib, _desc(L, in_dim=64, nb=13), D=64) == L.FETODE_EUNSUPPORTED   # F = 832 > 768
    assert b"768" in lib.fetode_last_error()


def test_backward_argument_checks():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    assert _bwd(lib, _desc(L, null_param=True)) == L.FETODE_EINVAL
    assert _bwd(lib, _desc(L), tape=None) == L.FETODE_EINVAL
    assert _bwd(lib, _desc(L), status=None) == L.FETODE_EINVAL
    assert _bwd(lib, _desc(L), D=3) == L.FETODE_EINVAL               # D != in_dim
    assert _bwd(lib, _desc(L, in_dim=64, nb=13), D=64) == L.FETODE_EUNSUPPORTED
    # n_ev must be base + 6 n_att, base = 2 (initial-step probe) or 1 (first_step given)
    assert _bwd(lib, _desc(L), n_ev=7, n_att=1) == L.FETODE_EINVAL
    assert b"attempts" in lib.fetode_last_error()
    assert _bwd(lib, _desc(L), n_ev=8, n_att=1, first_step=0.1) == L.FETODE_EINVAL
    assert _bwd(lib, _desc(L), n_ev=8, n_att=-1) == L.FETODE_EINVAL


def test_backward_queries():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    d = _desc(L)
    ws = lib.fetode_ecg_dopri5_backward_workspace
    assert ws(ctypes.byref(_desc(L, null_param=True)), 3, 8) == -1
    assert ws(ctypes.byref(d), 0, 8) == -1 and ws(ctypes.byref(d), 3, 0) == -1
    assert ws(ctypes.byref(_desc(L, in_dim=64, nb=13)), 3, 8) == -1
    a, b = ws(ctypes.byref(d), 3, 8), ws(ctypes.byref(d), 3, 80)
    assert a > 0 and b - a >= 72 * 3 * 4 * 4     # the gradient tape grows with n_ev: (n_ev, B, D) floats
    mb = lib.fetode_ecg_dopri5_backward_max_batch
    assert mb(ctypes.byref(_desc(L, null_param=True))) == -1
    assert mb(ctypes.byref(_desc(L, in_dim=64, nb=13))) == 0     # no resident sweep for this shape
    assert mb(ctypes.byref(_desc(L, in_dim=65, nb=2))) == 0
