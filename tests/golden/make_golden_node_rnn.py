"""Generate tests/golden/node_rnn.npz from the REFERENCE's ECG NODE-RNN classes.

Run in the survey/build container (needs the reference snapshot; never on the GPU box):

    python tests/golden/make_golden_node_rnn.py

compare_noise_ecg.py cannot be imported whole (it imports torchdiffeq and runs its experiments at
import), so this script reads the file as text, takes the five class definitions out of it with
`ast` (FullyNonlinearKANCell :325-341, LinearInterp1D :848-872, InputDrivenKANODEFunc :875-907,
OneODEEncoder :910-946, NODE_RNN :949-986) and executes exactly those definitions with torch / nn
in scope, FerroelectricBasis bound to the reference's own ferro_class module and `odeint` to the
oracle's restated torchdiffeq (oracle/torch_ref.py), as for the other trajectory fixtures.  Every
array is cross-checked bit for bit against tests/node_rnn_ref.py before it is written.

Contents (H = 8, D = 1, K = 3, T = 9, three samples): the state_dict, the inputs, per-sample
trajectories, logits, the three end states, the parameter gradients of a cross-entropy loss, and a
three-call sequence of the bare field with its states.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("FETODE_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import node_rnn_ref as R  # noqa: E402
from oracle import torch_ref as O  # noqa: E402

torch.set_num_threads(1)
CLASSES = ("FullyNonlinearKANCell", "LinearInterp1D", "InputDrivenKANODEFunc", "OneODEEncoder", "NODE_RNN")
H, D, K, T, B, C = 8, 1, 3, 9, 3, 2


def reference_classes():
    sys.path.insert(0, REF)
    import ferro_class  # noqa: E402  (the reference module)
    tree = ast.parse(open(os.path.join(REF, "compare_noise_ecg.py")).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in CLASSES]
    assert [n.name for n in body] == list(CLASSES), [n.name for n in body]
    ns = {"torch": torch, "nn": nn, "F": F, "odeint": O.odeint, "FerroelectricBasis": ferro_class.FerroelectricBasis}
    exec(compile(ast.Module(body=body, type_ignores=[]), "compare_noise_ecg.py", "exec"), ns)
    return ns


def same(a, b, what):
    a, b = a.detach(), b.detach()
    assert a.shape == b.shape and torch.equal(a, b), (what, (a - b).abs().max().item())


def main():
    ref = reference_classes()
    torch.manual_seed(41)
    m = ref["NODE_RNN"](input_size=D, hidden_size=H, num_classes=C, num_basis=K, solver="rk4")
    with torch.no_grad():   # gain / bias start at ones / zeros: move them so their gradients are exercised
        m.enc.odefunc.gain.add_(0.2 * torch.randn(H))
        m.enc.odefunc.bias.add_(0.1 * torch.randn(H))
    out = {"sd/" + k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(42)
    x = torch.randn(B, T, D, generator=g)
    y = torch.tensor([0, 1, 1])
    out["x"], out["y"] = x.numpy(), y.numpy()

    # per-sample trajectories (the encoder alone), then the model: logits, end states, gradients
    r = R.NodeRnn(sd).requires_grad_()
    with torch.no_grad():
        for b in range(B):
            tr = m.enc(x[b:b + 1], return_traj=True)
            same(tr, r.encode(x[b]), f"trajectory {b}")
            out[f"traj{b}"] = tr.numpy()
    logits = m(x)
    lo, _ = r(x)
    same(logits, lo, "logits")
    out["logits"] = logits.detach().numpy()
    states = {"enc.odefunc.basis.prev_x": m.enc.odefunc.basis.prev_x,
              "rnn_cell.input_basis.prev_x": m.rnn_cell.input_basis.prev_x,
              "rnn_cell.hidden_basis.prev_x": m.rnn_cell.hidden_basis.prev_x}
    for k_, v in states.items():
        same(v, r.end_states()[k_], k_)
        out["end/" + k_] = v.detach().numpy().copy()
    F.cross_entropy(logits, y).backward()
    F.cross_entropy(lo, y).backward()
    rp = r.named_params()
    for n, p in m.named_parameters():
        gr = p.grad if p.grad is not None else torch.zeros_like(p)
        gq = rp[n].grad if rp[n].grad is not None else torch.zeros_like(rp[n])
        same(gr, gq, "grad " + n)
        out["grad/" + n] = gr.numpy()

    # the bare field: three calls at t = 0, 0.3, 0.3 + 1/24 from the reset state, with its states
    f = m.enc.odefunc
    t_grid = torch.linspace(0.0, 1.0, steps=T)
    f.set_interpolator(ref["LinearInterp1D"](t_grid, x[1]))
    f.basis.reset_state()
    rf = R.DrivenField(sd, "enc.odefunc.")
    rf.set(t_grid, x[1])
    hs = torch.randn(3, 1, H, generator=g)
    ts = torch.tensor([0.0, 0.3, 0.3 + 1.0 / 24.0])
    out["field/h"], out["field/t"] = hs.numpy(), ts.numpy()
    with torch.no_grad():
        for c in range(3):
            yc = f(ts[c], hs[c])
            same(yc, rf(ts[c], hs[c]), f"field call {c}")
            same(f.basis.prev_x, rf.basis.st.prev_x, f"field prev_x {c}")
            out[f"field/y{c}"] = yc.numpy()
            out[f"field/prev{c}"] = f.basis.prev_x[:, :, 0, 0].numpy().copy()
    np.savez_compressed(os.path.join(HERE, "node_rnn.npz"), **out)
    print("node_rnn", len(out), "arrays", sum(v.nbytes for v in out.values()), "bytes")


if __name__ == "__main__":
    main()
