"""tests/node_rnn_ref.py (the CPU restatement of the ECG NODE-RNN the GPU tests measure against)
reproduces the fixture generated from the reference's own classes bit for bit
(tests/golden/make_golden_node_rnn.py -> tests/golden/node_rnn.npz)."""
import pytest
import torch
import torch.nn.functional as F

import node_rnn_ref as R
from conftest import golden_sd, load_golden


@pytest.fixture(scope="module")
def g():
    return load_golden("node_rnn")


def eq(a, b, what):
    b = torch.as_tensor(b)
    assert a.shape == b.shape and torch.equal(a.detach(), b), (what, (a.detach() - b).abs().max().item())


def test_trajectories_logits_states_and_gradients(g):
    sd = golden_sd(g)
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    r = R.NodeRnn(sd).requires_grad_()
    with torch.no_grad():
        for b in range(x.shape[0]):
            eq(r.encode(x[b]), g[f"traj{b}"], f"trajectory {b}")
    logits, trajs = r(x)
    eq(logits, g["logits"], "logits")
    for b, tr in enumerate(trajs):
        eq(tr, g[f"traj{b}"], f"trajectory {b} inside the model")
    for k, v in r.end_states().items():
        eq(v, g["end/" + k], k)
    F.cross_entropy(logits, y).backward()
    names = [k[len("grad/"):] for k in g if k.startswith("grad/")]
    assert len(names) == 21, names   # 3 Ferro x 5 + gain, bias + lift, head weight / bias
    for n in names:
        p = r.named_params()[n]
        eq(p.grad if p.grad is not None else torch.zeros_like(p), g["grad/" + n], "grad " + n)
    # hidden_basis never reaches the logits
    assert not torch.from_numpy(g["grad/rnn_cell.hidden_basis.coef"]).any()
    assert torch.from_numpy(g["grad/enc.odefunc.basis.coef"]).any()


def test_bare_field_sequence(g):
    sd = golden_sd(g)
    x = torch.from_numpy(g["x"])
    f = R.DrivenField(sd, "enc.odefunc.")
    f.set(torch.linspace(0.0, 1.0, steps=x.shape[1]), x[1])
    hs, ts = torch.from_numpy(g["field/h"]), torch.from_numpy(g["field/t"])
    with torch.no_grad():
        for c in range(3):
            eq(f(ts[c], hs[c]), g[f"field/y{c}"], f"field call {c}")
            eq(f.basis.prev, g[f"field/prev{c}"], f"field prev {c}")


def test_stage_times_are_the_solver_call_times(g):
    """stage_times (what the driving-table test evaluates the interpolation at) lists exactly the
    times at which the oracle's rk4 calls the field."""
    sd = golden_sd(g)
    x = torch.from_numpy(g["x"])
    r = R.NodeRnn(sd)
    seen = []
    inner = r.field.__call__

    class Spy:
        def __call__(self, t, h):
            seen.append(t.clone())
            return inner(t, h)

    t_grid = torch.linspace(0.0, 1.0, steps=x.shape[1])
    r.field.set(t_grid, x[0])
    r.field.basis.st.reset()
    with torch.no_grad():
        R.O.odeint(Spy(), F.linear(x[0, 0:1], r.lift_w, r.lift_b), t_grid, method="rk4")
    eq(torch.stack(seen), R.stage_times(t_grid), "stage times")
