"""Training the ECG KAN-FET NODE through the device-resident dopri5 solve (fetode_ecg_dopri5_tape +
fetode_ecg_dopri5_backward, switch dopri5.set_resident_ecg_training): loss and every gradient against
the CPU oracle's fp32 autograd through oracle.torch_ref.odeint (oracle/ecg_ref.py), with the
host-driven autograd path (_Dopri5Grad) measured against the same oracle in the same test.

Input condition: every case wraps the oracle field, records every evaluation's input and asserts
the oracle's gate margin min |x_e[b, i] - prev_e[i]| >= 1e-5 (100x the fp32 rounding of O(1)
states), so no hysteresis gate sits where two fp32 implementations could take different branches.
The seeds were picked on the CPU for that; the margins found are noted at each case.

Gradient bar per tensor: close() of tests/test_gpu_ecg.py with rel = max(1e-3, 2x the error the
host-driven path makes against the same oracle on the same inputs)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 1e-5
RTOL, ATOL = 1e-3, 1e-4


def rel_err(got, exp):
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    return (got - exp).abs().max().item() / (exp.abs().max().item() + 1e-12)


def close(got, exp, rel, name):
    got, exp = got.detach().double().cpu(), exp.detach().double().cpu()
    scale = exp.abs().max().item() + 1e-12
    err = (got - exp).abs().max().item()
    assert err <= rel * scale, f"{name}: max|diff|={err:.3e} scale={scale:.3e} rel bar={rel:.3e}"


class Recorder:
    """The oracle field, recording the gate margin of every evaluation's input."""

    def __init__(self, field):
        self.field, self.margin, self.calls = field, float("inf"), 0

    def __call__(self, t, h):
        prev = self.field.basis.prev_x.detach()
        self.margin = min(self.margin, (h.detach().unsqueeze(-1) - prev).abs().min().item())
        self.calls += 1
        return self.field(t, h)


def field_sd(seed, latent, nb):
    from fet_ode_amd import ecg
    torch.manual_seed(seed)
    f = ecg.No_MLP_KANODEFunc(latent_dim=latent, num_basis=nb)
    return {k: v.clone() for k, v in f.state_dict().items()}


def field_h0(seed, B, latent, scale=2.0):
    return torch.randn(B, latent, generator=torch.Generator().manual_seed(seed + 1000)) * scale


def trainable(sd):
    return {k: v.clone().requires_grad_(v.dtype.is_floating_point and "prev_x" not in k and "branch_state" not in k)
            for k, v in sd.items()}


T_FIELD = [0.0, 0.3, 0.7, 1.0]


def oracle_field(sd, h0, t, rtol, atol, opts, grad=True):
    """loss = mean(sol ** 2) over all output times through the oracle: loss, grads, trace, margin."""
    from oracle import ecg_ref as E
    from oracle import torch_ref as O
    ps = trainable(sd) if grad else sd
    rec = Recorder(E.ECGFieldRef.from_state_dict(ps))
    h = h0.clone().requires_grad_(grad)
    trace = O.Dopri5Trace()
    with torch.set_grad_enabled(grad):
        sol = O.odeint(rec, h, torch.tensor(t, dtype=torch.float64), method="dopri5", rtol=rtol, atol=atol,
                       options=opts, trace=trace)
        loss = (sol ** 2).mean()
    grads = {}
    if grad:
        loss.backward()
        grads = {k: v.grad for k, v in ps.items() if v.requires_grad}
        grads["h0"] = h.grad
    return loss.detach(), grads, trace, rec.margin, sol.detach()


def gpu_field(sd, h0, t, rtol, atol, opts, dev, resident, latent, nb, tape=None):
    """The same loss on the GPU with the switch on / off: loss, grads, last solve, module, solution."""
    import fet_ode_amd as F
    from fet_ode_amd import dopri5 as D5
    from fet_ode_amd import ecg
    m = ecg.No_MLP_KANODEFunc(latent_dim=latent, num_basis=nb)
    m.load_state_dict(sd)
    m = m.to(dev)
    if tape is not None:
        m._fetode_d5tape = tape
    h = h0.to(dev).requires_grad_(True)
    prev = D5.set_resident_ecg_training(resident)
    try:
        sol = F.odeint(m, h, torch.tensor(t, dtype=torch.float64), method="dopri5", rtol=rtol, atol=atol,
                       options=opts)
        last = D5.dopri5_solve.last
        loss = (sol ** 2).mean()
        loss.backward()
    finally:
        D5.set_resident_ecg_training(prev)
    grads = {n: p.grad for n, p in m.named_parameters()}
    grads["h0"] = h.grad
    return loss.detach().cpu(), grads, last, m, sol.detach()


def check_grads(res, host, ref, label):
    """Every tensor of `res` under the bar max(1e-3, 2x host error) against `ref`; both errors printed."""
    for n, exp in ref.items():
        if exp is None:
            assert res[n] is None or float(res[n].abs().max()) == 0.0, n
            continue
        assert res[n] is not None, n
        e_host = rel_err(host[n], exp) if host is not None else 0.0
        e_res = rel_err(res[n], exp)
        print(f"{label} {n}: resident {e_res:.3e} host {e_host:.3e}")
        close(res[n], exp, max(1e-3, 2.0 * e_host), f"{label} grad {n}")


# (B, latent, nb, seed, opts, rtol, atol, needs a rejected attempt).  The seed is the first from 1
# whose oracle gate margin is >= 1e-5 on the CPU (the last row's stage-6 and stage-7 inputs differ
# only by the step's error, so many seeds give a margin near 0); margin found / oracle attempts:
FIELD_CASES = {
    "default_latent1": (1, 1, 10, 7, None, RTOL, ATOL, False),                # 7.5e-05 / 2
    "one_workgroup": (3, 5, 7, 3, None, RTOL, ATOL, False),                   # 1.1e-05 / 4
    "second_workgroup": (4, 5, 7, 2, None, RTOL, ATOL, False),                # 1.5e-05 / 5
    "latent64": (37, 64, 10, 3, None, RTOL, ATOL, False),                     # 1.2e-05 / 5
    "first_step": (5, 6, 4, 1, {"first_step": 0.05}, RTOL, ATOL, False),      # 1.2e-05 / 5
    "rejected": (6, 8, 6, 6, {"first_step": 0.9}, 1e-5, 1e-6, True),          # 2.4e-05 / 28, 14 rejected
}


@pytest.mark.parametrize("name", list(FIELD_CASES))
def test_field_gradients_vs_oracle(dev, name):
    """The field alone, loss = mean(sol ** 2) over t = [0, 0.3, 0.7, 1] (the interpolant's adjoint at
    two interior times): loss within 1e-5, the oracle's attempt sequence, every gradient (h0's too)
    under the bar, with the host-driven path's error printed next to the resident one's."""
    from fet_ode_amd import dopri5 as D5
    B, latent, nb, seed, opts, rtol, atol, need_rej = FIELD_CASES[name]
    sd, h0 = field_sd(seed, latent, nb), field_h0(seed, B, latent)
    lref, gref, trace, margin, sref = oracle_field(sd, h0, T_FIELD, rtol, atol, opts)
    print(f"{name}: oracle gate margin {margin:.3e}, attempts {len(trace.attempts)}")
    assert margin >= MARGIN, margin
    acc = [a[3] for a in trace.attempts]
    if need_rej:
        assert any(acc) and not all(acc), acc
    lh, gh, last_h, _, _ = gpu_field(sd, h0, T_FIELD, rtol, atol, opts, dev, False, latent, nb)
    assert isinstance(last_h, D5._Dopri5Grad)
    lr, gr, last_r, _, sol = gpu_field(sd, h0, T_FIELD, rtol, atol, opts, dev, True, latent, nb)
    assert isinstance(last_r, D5.ResidentSolve)
    assert last_r.n_attempts == len(trace.attempts) == len(last_h.attempts)
    assert [a[3] for a in last_r.attempts] == acc
    assert last_r.nfev == (1 if opts and "first_step" in opts else 2) + 6 * len(acc)
    assert abs(lr.item() - lref.item()) <= 1e-5 * abs(lref.item())
    check_grads(gr, gh, gref, name)


# KanFet_NODE(T = 96, 2 classes, latent 64, nb 10), B = 16: the first seed from 1 (model and series)
# whose oracle gate margin is >= 1e-5 on the CPU (1.07e-05, 8 attempts)
NODE_SEED = 306
_NODE = {}


def node_case(dev):
    """Case 1's model, inputs, oracle and host-driven results, computed once."""
    if _NODE:
        return _NODE
    from fet_ode_amd import dopri5 as D5
    from fet_ode_amd import ecg
    from oracle import ecg_ref as E
    torch.manual_seed(NODE_SEED)
    m = ecg.KanFet_NODE(T=96, num_classes=2, latent_dim=64, num_basis=10, rtol=RTOL, atol=ATOL)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = E.ecg_x(16, seed=NODE_SEED)
    y = torch.arange(16) % 2
    ps = trainable(sd)
    ref = E.ECGNodeRef(ps, rtol=RTOL, atol=ATOL)
    ref.field = Recorder(ref.field)
    lref = torch.nn.functional.cross_entropy(ref(x), y)
    lref.backward()
    _NODE.update(sd=sd, x=x, y=y, lref=lref.detach(), gref={k: v.grad for k, v in ps.items() if v.requires_grad},
                 trace=ref.trace, margin=ref.field.margin)
    _NODE["host"] = node_run(dev, False)
    assert isinstance(_NODE["host"][2], D5._Dopri5Grad)
    return _NODE


def node_run(dev, resident, tape=None):
    from fet_ode_amd import dopri5 as D5
    from fet_ode_amd import ecg
    c = _NODE
    m = ecg.KanFet_NODE(T=96, num_classes=2, latent_dim=64, num_basis=10, rtol=RTOL, atol=ATOL)
    m.load_state_dict(c["sd"])
    m = m.to(dev).eval()
    if tape is not None:
        m.odefunc._fetode_d5tape = tape
    prev = D5.set_resident_ecg_training(resident)
    try:
        loss = torch.nn.functional.cross_entropy(m(c["x"].to(dev)), c["y"].to(dev))
        last = m.last_solve
        loss.backward()
    finally:
        D5.set_resident_ecg_training(prev)
    return loss.detach().cpu(), {n: p.grad for n, p in m.named_parameters()}, last, m


def test_node_training_vs_oracle(dev):
    """KanFet_NODE, B = 16, cross-entropy: loss within 1e-5, the oracle's attempt count, a
    ResidentSolve, every parameter gradient (encoder.* through grad_y0) under the bar."""
    from fet_ode_amd import dopri5 as D5
    c = node_case(dev)
    print(f"node: oracle gate margin {c['margin']:.3e}, attempts {len(c['trace'].attempts)}")
    assert c["margin"] >= MARGIN, c["margin"]
    loss, grads, last, m = node_run(dev, True)
    assert isinstance(last, D5.ResidentSolve)
    assert last.n_attempts == len(c["trace"].attempts) == len(c["host"][2].attempts)
    assert abs(loss.item() - c["lref"].item()) <= 1e-5 * abs(c["lref"].item())
    ref = {n: c["gref"].get(n) for n, _ in m.named_parameters()}
    assert ref["encoder.weight"] is not None and ref["odefunc.feat.basis.k"] is not None
    check_grads(grads, c["host"][1], ref, "node")


def test_node_training_is_deterministic(dev):
    """Two runs of case 1 give bitwise-equal gradients (fixed-order sums, no atomics)."""
    node_case(dev)
    _, g1, _, _ = node_run(dev, True)
    _, g2, _, _ = node_run(dev, True)
    for n in g1:
        if g1[n] is None:
            assert g2[n] is None, n
        else:
            assert torch.equal(g1[n], g2[n]), n


def test_tape_overflow_reruns_bitwise(dev):
    """A tape capacity below nfev (and an attempt log below the attempts): the solve is re-run from
    the saved prev_x; solution, gradients, prev_x and branch_state are bitwise the uncapped run's."""
    B, latent, nb, seed, opts, rtol, atol, _ = FIELD_CASES["latent64"]
    sd, h0 = field_sd(seed, latent, nb), field_h0(seed, B, latent)
    _, g1, last1, m1, s1 = gpu_field(sd, h0, T_FIELD, rtol, atol, opts, dev, True, latent, nb, tape=(4096, 512))
    _, g2, last2, m2, s2 = gpu_field(sd, h0, T_FIELD, rtol, atol, opts, dev, True, latent, nb, tape=(3, 1))
    assert last1.nfev == last2.nfev > 3 and last1.n_attempts == last2.n_attempts > 1
    assert torch.equal(s1, s2)
    for n in g1:
        assert (g1[n] is None and g2[n] is None) or torch.equal(g1[n], g2[n]), n
    assert torch.equal(m1.feat.basis.prev_x, m2.feat.basis.prev_x)
    assert torch.equal(m1.feat.basis.branch_state, m2.feat.basis.branch_state)


@pytest.mark.parametrize("B,seed", [(37, 3), (769, 118)])
def test_taped_forward_is_bitwise_the_inference_solve(dev, B, seed):
    """fetode_ecg_dopri5_tape against fetode_ecg_dopri5 on the same inputs (R = 4 and R = 8 grids):
    solution, attempt log, nfev, prev_x and branch_state bit for bit."""
    import fet_ode_amd as F
    from fet_ode_amd import dopri5 as D5
    from fet_ode_amd import ecg
    latent, nb = 64, 10
    sd, h0 = field_sd(seed, latent, nb), field_h0(seed, B, latent)
    _, _, last_t, mt, st = gpu_field(sd, h0, T_FIELD, RTOL, ATOL, None, dev, True, latent, nb)
    mi = ecg.No_MLP_KANODEFunc(latent_dim=latent, num_basis=nb)
    mi.load_state_dict(sd)
    mi = mi.to(dev)
    with torch.no_grad():
        si = F.odeint(mi, h0.to(dev), torch.tensor(T_FIELD, dtype=torch.float64), method="dopri5", rtol=RTOL,
                      atol=ATOL)
    last_i = D5.dopri5_solve.last
    assert isinstance(last_t, D5.ResidentSolve) and isinstance(last_i, D5.ResidentSolve)
    assert torch.equal(st, si)
    assert last_t.nfev == last_i.nfev and last_t.attempts == last_i.attempts
    assert torch.equal(mt.feat.basis.prev_x, mi.feat.basis.prev_x)
    assert torch.equal(mt.feat.basis.branch_state, mi.feat.basis.branch_state)


def test_r8_variant_vs_host_path(dev):
    """B = 769, latent 64: the first batch on the R = 8 forward grid.  Gradients against the
    host-driven path (switch off) as the reference, bar 1e-3; equal attempt counts."""
    from fet_ode_amd import dopri5 as D5
    B, latent, nb, seed = 769, 64, 10, 118   # the first seed from 1 with an oracle gate margin >= 1e-5 (1.39e-05)
    sd, h0 = field_sd(seed, latent, nb), field_h0(seed, B, latent)
    _, _, trace, margin, _ = oracle_field(sd, h0, T_FIELD, RTOL, ATOL, None, grad=False)
    print(f"B=769: oracle gate margin {margin:.3e}, attempts {len(trace.attempts)}")
    assert margin >= MARGIN, margin
    lh, gh, last_h, _, sh = gpu_field(sd, h0, T_FIELD, RTOL, ATOL, None, dev, False, latent, nb)
    lr, gr, last_r, _, sr = gpu_field(sd, h0, T_FIELD, RTOL, ATOL, None, dev, True, latent, nb)
    assert isinstance(last_h, D5._Dopri5Grad) and isinstance(last_r, D5.ResidentSolve)
    assert last_r.n_attempts == len(last_h.attempts) == len(trace.attempts)
    close(sr, sh, 1e-5, "solution")
    check_grads(gr, None, gh, "B=769")


def test_module_state_after_training_forward(dev):
    """prev_x equals the host-driven training forward's within 1e-5, branch_state differs in <= 1 %
    of the elements (the bounds of test_resident_dopri5_matches_host_driven)."""
    B, latent, nb, seed, opts, rtol, atol, _ = FIELD_CASES["latent64"]
    sd, h0 = field_sd(seed, latent, nb), field_h0(seed, B, latent)
    _, _, _, mh, _ = gpu_field(sd, h0, T_FIELD, rtol, atol, opts, dev, False, latent, nb)
    _, _, _, mr, _ = gpu_field(sd, h0, T_FIELD, rtol, atol, opts, dev, True, latent, nb)
    close(mr.feat.basis.prev_x, mh.feat.basis.prev_x, 1e-5, "prev_x")
    assert mr.feat.basis.branch_state.shape == mh.feat.basis.branch_state.shape == (B, latent, nb)
    assert (mr.feat.basis.branch_state != mh.feat.basis.branch_state).float().mean().item() <= 1e-2


def test_routing(dev):
    """Switch on: no_grad keeps the inference ResidentSolve; a non-Sigmoid act or a batch above the
    resident grids takes _Dopri5Grad.  Switch off: _Dopri5Grad."""
    import fet_ode_amd as F
    from fet_ode_amd import _lib
    from fet_ode_amd import dopri5 as D5
    from fet_ode_amd import ecg
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)

    def solve(m, B, grad=True, **kw):
        h = torch.randn(B, m.latent_dim, generator=torch.Generator().manual_seed(5)).to(dev)
        with torch.set_grad_enabled(grad):
            sol = F.odeint(m, h, t, method="dopri5", rtol=RTOL, atol=ATOL, **kw)
        return sol, D5.dopri5_solve.last

    torch.manual_seed(0)
    m = ecg.No_MLP_KANODEFunc(latent_dim=4, num_basis=5).to(dev)
    prev = D5.set_resident_ecg_training(True)
    try:
        sol, last = solve(m, 6)
        assert isinstance(last, D5.ResidentSolve) and sol.requires_grad
        sol, last = solve(m, 6, grad=False)
        assert isinstance(last, D5.ResidentSolve) and not sol.requires_grad
        keep = []
        mb = _lib.load().fetode_ecg_dopri5_backward_max_batch(_lib.ctypes.byref(m.feat.basis.desc(keep)))
        assert mb >= 769
        sol, last = solve(m, min(mb, 3072) + 1)
        assert isinstance(last, D5._Dopri5Grad) and sol.requires_grad
        torch.manual_seed(0)
        m2 = ecg.No_MLP_KANODEFunc(latent_dim=4, num_basis=5)
        m2.feat.act = torch.nn.Tanh()
        sol, last = solve(m2.to(dev), 6)
        assert isinstance(last, D5._Dopri5Grad)
        D5.set_resident_ecg_training(False)
        sol, last = solve(m, 6)
        assert isinstance(last, D5._Dopri5Grad)
    finally:
        D5.set_resident_ecg_training(prev)
