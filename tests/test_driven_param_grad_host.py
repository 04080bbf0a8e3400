"""Host-side logic of the driven-field parameter-gradient pass (fetode_driven_param_grad):
the exported symbols and their bindings, what the entry decides before any launch, the workspace query,
the row-split setter, the Python knob with its environment variable, and which entry the two trainers'
backward calls with the knob on and off.  No GPU."""
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from test_driven_dopri5_host import _desc

NEW = ("fetode_driven_param_grad_workspace", "fetode_driven_param_grad", "fetode_driven_param_grad_set_splits")


def test_symbols_and_signatures():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    for n in NEW:
        assert n in L.SIGNATURES, n
        getattr(lib, n)
    res, args = L.SIGNATURES["fetode_driven_param_grad"]
    assert res is ctypes.c_int and len(args) == 17 and args[12] is ctypes.POINTER(L.FerroGrad)
    assert L.SIGNATURES["fetode_driven_param_grad_workspace"][0] is ctypes.c_int64
    assert lib.fetode_abi_version() == 3


def _call(lib, d, gain=0x1000, B=3, n_ev=8, sb=1, se=3, nfev=None, ns=0, prev0=None, hx=0x1000, phi=0x1000,
          adj=0x1000, grads="all", g_gain=0x1000, g_bias=0x1000, ws=0x1000):
    import fet_ode_amd as F
    L = F._lib
    gs = L.FerroGrad(*[0x1000] * 5) if grads == "all" else grads
    return lib.fetode_driven_param_grad(ctypes.byref(d), gain, B, n_ev, sb, se, nfev, ns, prev0, hx, phi, adj,
                                        ctypes.byref(gs) if gs is not None else None, g_gain, g_bias, ws, None)


def test_abi_decides_before_any_launch():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    ok = _desc(L, 8, 1, 3)
    # outside the family: EUNSUPPORTED, whatever else is wrong
    for H, D, K in ((65, 1, 10), (64, 5, 10), (64, 1, 17)):
        assert _call(lib, _desc(L, H, D, K)) == L.FETODE_EUNSUPPORTED, (H, D, K)
        assert _call(lib, _desc(L, H, D, K), hx=None, B=0) == L.FETODE_EUNSUPPORTED
    assert _call(lib, _desc(L, 8, 1, 3, bsign=0x2000)) == L.FETODE_EUNSUPPORTED
    assert b"family" in lib.fetode_last_error()
    # the required pointers: the three tapes, gain, and the workspace when any output is requested
    for k in ("hx", "phi", "adj", "gain", "ws"):
        assert _call(lib, ok, **{k: None}) == L.FETODE_EINVAL, k
    assert b"null pointer" in lib.fetode_last_error()
    assert _call(lib, ok, ws=None, grads=None, g_gain=None) == L.FETODE_EINVAL          # g_bias alone needs it too
    assert _call(lib, ok, ws=None, grads=L.FerroGrad(None, None, None, None, 0x1000), g_gain=None,
                 g_bias=None) == L.FETODE_EINVAL
    # nothing requested: nothing to do, no workspace needed, nothing launched
    assert _call(lib, ok, ws=None, grads=None, g_gain=None, g_bias=None) == L.FETODE_OK
    assert _call(lib, ok, ws=None, grads=L.FerroGrad(), g_gain=None, g_bias=None) == L.FETODE_OK
    # an empty batch or tape is done, the null pointers are not even looked at
    assert _call(lib, ok, B=0) == L.FETODE_OK and _call(lib, ok, n_ev=0) == L.FETODE_OK
    assert _call(lib, ok, B=0, hx=None, ws=None) == L.FETODE_OK and _call(lib, ok, n_ev=-1, adj=None) == L.FETODE_OK
    # strides are row counts
    assert _call(lib, ok, sb=0) == L.FETODE_EINVAL and _call(lib, ok, se=-1) == L.FETODE_EINVAL
    assert _call(lib, ok, nfev=0x1000, ns=0) == L.FETODE_EINVAL


def _slice_bytes(H, D, K):
    return 4 * 3 * ((H + D) * K * H + H)


def test_workspace_query_and_splits():
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    ws, setter = lib.fetode_driven_param_grad_workspace, lib.fetode_driven_param_grad_set_splits
    for H, D, K in ((65, 1, 10), (64, 5, 10), (64, 1, 17)):
        assert ws(ctypes.byref(_desc(L, H, D, K)), 3, 8) == -1
    assert ws(ctypes.byref(_desc(L, 8, 1, 3, bsign=0x2000)), 3, 8) == -1
    prev = setter(-1)
    try:
        assert prev == 0                                  # from the shape by default
        assert setter(3) == 0 and setter(-1) == 3 and setter(-7) == 3
        for bad in (65, 1 << 20, -2):
            assert setter(bad) == 3 and setter(-1) == 3
        assert setter(0) == 3 and setter(-1) == 0
        sizes = [(1, 1), (1, 3), (3, 8), (5, 20), (67, 4), (67, 40), (256, 380), (256, 386), (4096, 400)]
        for H, D, K in ((1, 1, 1), (8, 1, 3), (64, 1, 10), (64, 4, 16)):
            d = _desc(L, H, D, K)
            auto = [ws(ctypes.byref(d), B, n) for B, n in sizes]
            assert all(a > 0 for a in auto)
            assert all(a <= b for a, b in zip(auto, auto[1:])), auto    # never decreases in B * n_ev
            assert ws(ctypes.byref(d), 0, 5) > 0 and ws(ctypes.byref(d), 1 << 40, 1 << 20) == auto[-1]
            for s in range(1, 65):                       # every split the setter accepts
                assert setter(s) in (0, s - 1)
                for (B, n), a in zip(sizes, auto):
                    got = ws(ctypes.byref(d), B, n)
                    assert got == a                                      # the size does not follow the knob
                    assert got >= min(s, max(1, B * n // 4)) * _slice_bytes(H, D, K), (s, B, n)
            setter(0)
        assert ws(ctypes.byref(_desc(L, 64, 4, 16)), 4096, 400) == 64 * _slice_bytes(64, 4, 16)
    finally:
        setter(prev)


@pytest.mark.parametrize("env,expect", [(None, False), ("0", False), ("1", True), ("", False)])
def test_knob_env_and_return_value(env, expect):
    """Off by default; FETODE_DRIVEN_PARAM_GRADS=1 turns it on at import; the setter returns the previous
    value."""
    e = {k: v for k, v in os.environ.items() if k != "FETODE_DRIVEN_PARAM_GRADS"}
    if env is not None:
        e["FETODE_DRIVEN_PARAM_GRADS"] = env
    code = ("import sys; sys.path.insert(0, %r); from fet_ode_amd import ecg; "
            "S = ecg.set_fused_driven_param_grads; a = S(True); b = S(False); c = S(a); d = S(False); "
            "print(a, b, c, d, sep='|')" % REPO)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout
    assert out.strip().split("|") == [str(expect), "True", "False", str(expect)]


class _FakeLib:
    """Stands where libfetode does: every entry returns FETODE_OK and is logged with its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 4096 if name.endswith("_workspace") else 0
        return entry

    def names(self):
        return [n for n, _ in self.calls]


@pytest.fixture
def fake(monkeypatch):
    import fet_ode_amd as F
    from fet_ode_amd import autograd_ops
    lib = _FakeLib()
    monkeypatch.setattr(F._lib, "load", lambda: lib)
    monkeypatch.setattr(F._lib, "stream_handle", lambda dev: None)
    monkeypatch.setattr(autograd_ops, "_stream", lambda x: None)
    return lib


def _field_ctx(ecg, H=8, D=1, K=3):
    torch.manual_seed(0)
    f = ecg.InputDrivenKANODEFunc(D, H, K)
    keep = []
    return f, f.basis.desc(keep), keep, [p.detach() for p in ecg._driven_tensors(f)]


def test_rk4_backward_takes_the_new_entry_only_with_the_knob_on(fake):
    from fet_ode_amd import ecg
    H, D, B, n_steps = 8, 1, 3, 2
    f, d, keep, params = _field_ctx(ecg)
    ne = 4 * n_steps
    thx, tphi = torch.randn(ne, B, H + D), torch.randn(ne, B, H)
    ctx = SimpleNamespace(f=f, n_steps=n_steps, d=d, keep=keep, plan=torch.zeros(4),
                          saved_tensors=(torch.ones(n_steps), torch.zeros(B, H + D), thx, tphi, *params),
                          needs_input_grad=(False, False, False, True) + (True,) * 7)
    prev = ecg.set_fused_driven_param_grads(False)
    try:
        out = ecg._DrivenFn.backward(ctx, torch.randn(n_steps + 1, B, H))
        assert fake.names() == ["fetode_driven_fixed_backward", "fetode_ferro_backward"]
        assert len(out) == 11 and all(g is not None for g in out[3:])
        fake.calls.clear()
        ecg.set_fused_driven_param_grads(True)
        out = ecg._DrivenFn.backward(ctx, torch.randn(n_steps + 1, B, H))
        assert fake.names() == ["fetode_driven_fixed_backward", "fetode_driven_param_grad_workspace",
                                "fetode_driven_param_grad"]
        a = fake.calls[-1][1]
        # B, n_ev, stride_b, stride_e of the (n_ev, B, .) tape; no nfev; prev0 and the tapes themselves
        assert a[2:6] == (B, ne, 1, B) and a[6] is None and a[7] == 0
        assert a[8] == ctx.saved_tensors[1].data_ptr() and a[9:11] == (thx.data_ptr(), tphi.data_ptr())
        assert [tuple(g.shape) for g in out[4:]] == [tuple(p.shape) for p in params]
        # needs_input_grad -> NULL pointers
        fake.calls.clear()
        ctx.needs_input_grad = (False, False, False, True, False, False, False, False, True, False, True)
        out = ecg._DrivenFn.backward(ctx, torch.randn(n_steps + 1, B, H))
        a = fake.calls[-1][1]
        gs = a[12]._obj
        assert (gs.k, gs.Ec, gs.Ps, gs.bias) == (None,) * 4 and gs.coef and a[13] is None and a[14]
        assert [g is None for g in out[4:]] == [True, True, True, True, False, True, False]
        # no evaluations: zeros, and no parameter pass of either kind
        fake.calls.clear()
        ctx.saved_tensors = (torch.ones(0), torch.zeros(B, H + D), thx[:0], tphi[:0], *params)
        ctx.n_steps, ctx.needs_input_grad = 0, (False, False, False, True) + (True,) * 7
        out = ecg._DrivenFn.backward(ctx, torch.randn(1, B, H))
        assert fake.names() == ["fetode_driven_fixed_backward"]
        assert all(not g.any() and g.shape == p.shape for g, p in zip(out[4:], params))
    finally:
        ecg.set_fused_driven_param_grads(prev)


def test_dopri5_backward_takes_the_new_entry_only_with_the_knob_on(fake):
    from fet_ode_amd import ecg
    from fet_ode_amd.dopri5 import _opts_array
    H, D, B, T, max_att = 8, 1, 2, 5, 4
    max_ev = 2 + 6 * max_att
    f, d, keep, params = _field_ctx(ecg)
    stats = torch.tensor([[14, 2, 0], [8, 1, 0]], dtype=torch.int32)
    tape = SimpleNamespace(hx=torch.zeros(B, max_ev, H + D), phi=torch.zeros(B, max_ev, H), slope=torch.zeros(B, max_ev, D),
                           init=torch.zeros(B, 5, dtype=torch.float64), att=torch.zeros(B, max_att, 4, dtype=torch.float64),
                           stats=stats, opts=_opts_array({}), max_ev=max_ev, max_att=max_att)
    rec = ecg.DrivenDopri5Solve(stats, tape.att, None)
    ctx = SimpleNamespace(f=f, d=d, keep=keep, plan=torch.zeros(4), tape=tape, rec=rec, tg=torch.linspace(0, 1, T),
                          prev0=None, tols=(1e-2, 1e-3), step_grad=True, saved_tensors=tuple(params),
                          needs_input_grad=(False,) * 3 + (True,) + (False,) * 4 + (True,) * 7)
    prev = ecg.set_fused_driven_param_grads(False)
    try:
        out = ecg._DrivenDopri5Fn.backward(ctx, torch.randn(T, B, H))
        assert fake.names() == ["fetode_driven_dopri5_backward", "fetode_ferro_backward"]
        assert fake.calls[-1][1][2] == B * 14            # today: B * max(nfev) rows, padding included
        fake.calls.clear()
        ecg.set_fused_driven_param_grads(True)
        out = ecg._DrivenDopri5Fn.backward(ctx, torch.randn(T, B, H))
        assert fake.names() == ["fetode_driven_dopri5_backward", "fetode_driven_param_grad_workspace",
                                "fetode_driven_param_grad"]
        a = fake.calls[-1][1]
        # the (B, max_ev, .) tape up to the longest solve, stats as nfev with stride 3, the reset state
        assert a[2:6] == (B, 14, max_ev, 1) and a[6] == stats.data_ptr() and a[7] == 3 and a[8] is None
        assert a[9:12] == (tape.hx.data_ptr(), tape.phi.data_ptr(), ecg._DrivenDopri5Fn.last_adj.data_ptr())
        assert len(out) == 15 and [tuple(g.shape) for g in out[8:]] == [tuple(p.shape) for p in params]
    finally:
        ecg.set_fused_driven_param_grads(prev)
        ecg._DrivenDopri5Fn.last_adj = None
