"""Tape-anchored replay of a fixed-grid solve — test infrastructure only (as oracle/torch_ref.py).

The training path of the fused solves is two computations: a forward that records the layer inputs
of every field evaluation (the tape), and a reverse sweep that, GIVEN those inputs, is linear in the
cotangent.  End to end the pair is ill-conditioned for KAN-FET fields (the hysteresis gate amplifies
the rounding of x - prev_x), so a gradient compared with autograd through an independent trajectory
can be held to 1e-3 at best.  Cut at the tape it is not: a replay of the oracle solve whose layer
inputs are REPLACED by the tape's values has the sweep's exact inputs, in any precision, and its
gradients are the plain high-precision reference of the sweep alone.

Built only from oracle/torch_ref.py pieces.  The substitution is ``x = x + (x_tape - x).detach()``:
the value is the tape's, the gradient flows as in the solve; the hysteresis state follows from the
substituted inputs as in ``ferro_forward`` (prev_x <- the layer's input, ferro_class.py:409), and the
first-call rules (ferro_class.py:373-378) come from building the oracle's state the way the module
holds it.  The hooks are per (evaluation, layer) and know nothing of the step grid, so an adaptive
solve can be replayed through them as well.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional, Sequence, Union

import torch

from . import parity as P
from . import torch_ref as O

NOT_TRAINED = ("grid", "prev_x", "branch_sign")   # buffers of the state dict
REL = 1e-5     # the floor of the bar (the project's parity bar, tests/test_gpu_parity.py REL)
FACTOR = 4     # the envelope rule's factor (tests/test_gpu_ecg.py, tests/test_gpu_dispatch.py)
CAP = 1e-4     # no asserted bar above this fraction of a tensor's scale

State0 = Union[str, Sequence[Optional[torch.Tensor]]]
Hook = Callable[[int, int, torch.Tensor], torch.Tensor]


# ---------------------------------------------------------------------------------------------
# the field with a hook on every layer input
# ---------------------------------------------------------------------------------------------

def build_field(sd: Dict[str, torch.Tensor], widths: Sequence[int], dtype, gate_slope=10.0, alpha=0.8,
                requires_grad=True):
    """(params, field): the float entries of ``sd`` as leaves of ``dtype`` (the parameters requiring
    grad) and the oracle field over them: KANFETRef where the state dict has Ferro layers, else KANRef."""
    n_layers = len(widths) - 1
    params = {}
    for k, v in sd.items():
        if not v.dtype.is_floating_point:
            continue
        p = v.detach().clone().to(dtype)
        if requires_grad and k.rsplit(".", 1)[-1] not in NOT_TRAINED:
            p.requires_grad_(True)
        params[k] = p
    if "layers.0.ferro.k" in sd:
        field = O.KANFETRef.from_state_dict(params, n_layers, gate_slope, alpha)
        kan = field.kan
    else:
        kan = [O.KANLinearParams.from_state_dict(params, f"layers.{l}.") for l in range(n_layers)]
        field = O.KANRef(kan)
    for l, kp in enumerate(kan):
        assert (kp.in_features, kp.out_features) == (widths[l], widths[l + 1]), (l, widths)
    return params, field


def set_state(field, state0: State0, dtype):
    """The hysteresis state before the solve, as the module would hold it: "fresh" = a new module's
    (prev_x zeros of batch 1: dx = x at B = 1, re-initialised to x, dx = 0, at B > 1); else per Ferro
    layer the compact (B, in) prev_x, or None for a stored state that does not fit the batch
    (re-initialised on the first call).  branch_sign stays all ones (the only value the reference
    ever holds)."""
    if isinstance(field, O.KANRef) or isinstance(state0, str):
        assert not isinstance(state0, str) or state0 == "fresh", state0
        return
    assert len(state0) == len(field.states)
    for st, fp, p in zip(field.states, field.ferro, state0):
        i, o, K = fp.k.shape
        if p is None:
            st.prev_x = torch.zeros(0, i, o, K, dtype=dtype)
        else:
            st.prev_x = p.detach().to(dtype)[:, :, None, None].expand(-1, -1, o, K).clone()


class HookedField:
    """``func(t, y)`` of the oracle field with ``hook(evaluation, layer, x) -> x`` applied to every
    layer's input; evaluations are counted in call order, whatever the solver."""

    def __init__(self, field, hook: Hook):
        self.field, self.hook, self.ev = field, hook, 0

    def __call__(self, t, x):
        f = self.field
        if isinstance(f, O.KANRef):
            for l, kp in enumerate(f.layers):
                x = O.kanlinear_forward(self.hook(self.ev, l, x), kp)
        else:
            for l, (kp, fp, st) in enumerate(zip(f.kan, f.ferro, f.states)):
                x = self.hook(self.ev, l, x)
                x = O.kanlinear_forward(x, kp) + O.ferro_forward(x, fp, st)
        self.ev += 1
        return x


# ---------------------------------------------------------------------------------------------
# a named approximation of the kernels, applied to the replay
# ---------------------------------------------------------------------------------------------

class _SigmoidRoundedDerivative(torch.autograd.Function):
    """s = 1 / (1 + exp(-z)) whose derivative is formed from the ROUNDED s as s - s * s (one fma), the
    way every sweep kernel forms the logistic basis' derivative (ffma(-sg, sg, sg)).  Where s is
    saturated towards 1 that difference cancels: its absolute error is an ulp of s (6e-8), whatever
    the derivative's size, while autograd through 2 / (1 + exp(-z)) keeps the derivative's relative
    precision.  Identical in exact arithmetic (fp64: 4e-14 apart)."""

    @staticmethod
    def forward(ctx, z):
        s = 1.0 / (1.0 + torch.exp(-z))
        ctx.save_for_backward(s)
        return s

    @staticmethod
    def backward(ctx, g):
        s, = ctx.saved_tensors
        return g * torch.addcmul(s, -s, s)


def _logistic_basis_rounded_derivative(x, a, b):
    return 2.0 * _SigmoidRoundedDerivative.apply(a * (x.unsqueeze(-1) - b))


@contextlib.contextmanager
def logistic_derivative(kind: str):
    """"exact": the oracle as it is; "rounded": its logistic basis with the kernels' derivative."""
    assert kind in ("exact", "rounded"), kind
    prev = O.logistic_basis
    if kind == "rounded":
        O.logistic_basis = _logistic_basis_rounded_derivative
    try:
        yield
    finally:
        O.logistic_basis = prev


# ---------------------------------------------------------------------------------------------
# tapes
# ---------------------------------------------------------------------------------------------

def parse_tape_rows(tape: torch.Tensor, D: int, H: int) -> List[torch.Tensor]:
    """The [2, 10, 2] kernels' tape (n_ev, B, D + H): per evaluation and trajectory the row (x, h)."""
    assert tape.dim() == 3 and tape.shape[2] == D + H, tape.shape
    t = tape.detach().cpu()
    return [t[:, :, :D].contiguous(), t[:, :, D:].contiguous()]


def parse_tape_planes(tape: torch.Tensor, n_ev: int, B: int, D: int, H: int) -> List[torch.Tensor]:
    """The fieldn kernels' tape: the plane of layer-0 inputs (n_ev, B, D), then the plane of layer-1
    inputs (n_ev, B, H), in one buffer of n_ev * B * (D + H) floats."""
    flat = tape.detach().cpu().reshape(-1)
    assert flat.numel() == n_ev * B * (D + H), (flat.numel(), n_ev, B, D, H)
    nx = n_ev * B * D
    return [flat[:nx].reshape(n_ev, B, D).contiguous(), flat[nx:].reshape(n_ev, B, H).contiguous()]


def record_tape(sd, widths, y0, t, method, options=None, state0: State0 = "fresh", dtype=torch.float32,
                gate_slope=10.0, alpha=0.8):
    """The plain oracle solve in ``dtype``, recording its own tape.  Returns (solution, tape,
    final_state): tape[l] is (n_ev, B, widths[l]); final_state the compact prev_x per Ferro layer."""
    _, field = build_field(sd, widths, dtype, gate_slope, alpha, requires_grad=False)
    set_state(field, state0, dtype)
    rows: List[List[torch.Tensor]] = [[] for _ in widths[:-1]]

    def rec(ev, l, x):
        rows[l].append(x.detach().clone())
        return x

    with torch.no_grad():
        sol = O.odeint(HookedField(field, rec), y0.to(dtype), t, method=method, options=options)
    final = [] if isinstance(field, O.KANRef) else [s.prev_x[:, :, 0, 0].clone() for s in field.states]
    return sol, [torch.stack(r) for r in rows], final


def replay_vjp(sd, widths, y0, t, method, options, state0: State0, tape: Sequence[torch.Tensor],
               cotangent: torch.Tensor, dtype, gate_slope=10.0, alpha=0.8, hook: Optional[Hook] = None,
               logistic="exact"):
    """Gradients of sum(cotangent * solution) w.r.t. y0 ("y0") and every parameter (state-dict
    names), in float64 tensors, of the oracle solve in ``dtype`` with every layer input taken from
    ``tape`` (per layer (n_ev, B, width), any dtype; converted to ``dtype``).  ``hook`` replaces the
    substitution (a follow-up may substitute other recorded quantities); ``logistic="rounded"`` applies
    the kernels' logistic-derivative approximation (logistic_derivative)."""
    params, field = build_field(sd, widths, dtype, gate_slope, alpha)
    set_state(field, state0, dtype)
    tp = [x.to(dtype) for x in tape]
    n_ev = tp[0].shape[0]

    def sub(ev, l, x):
        return x + (tp[l][ev] - x).detach()

    f = HookedField(field, hook or sub)
    yc = y0.detach().clone().to(dtype).requires_grad_(True)
    leaves = {k: p for k, p in params.items() if p.requires_grad}
    with logistic_derivative(logistic):
        sol = O.odeint(f, yc, t, method=method, options=options)
        assert f.ev == n_ev, (f.ev, n_ev)
        assert sol.shape == cotangent.shape, (sol.shape, cotangent.shape)
        grads = torch.autograd.grad((sol * cotangent.to(dtype)).sum(), [yc] + list(leaves.values()),
                                    allow_unused=True)
    out = {"y0": grads[0].double() if grads[0] is not None else torch.zeros_like(yc, dtype=torch.float64)}
    for (k, p), g in zip(leaves.items(), grads[1:]):
        out[k] = g.double() if g is not None else torch.zeros_like(p, dtype=torch.float64)
    return out


# ---------------------------------------------------------------------------------------------
# the bar: |got - fp64 replay| <= 4 Y + 1e-5 scale, never above 1e-4 scale
# ---------------------------------------------------------------------------------------------

class Envelope:
    """The fp64-anchored replay ``g64`` of one (problem, tape, cotangent), and per tensor its scale
    (max |g64|) and Y: the worst distance from g64 of the fp32-anchored replay, of ``n_rerounded``
    6e-8 re-roundings of its parameters (oracle.parity.perturbed_state_dicts) and of the fp32 replay
    under the kernels' one named approximation (logistic_derivative("rounded"); DESIGN.md §4 has the
    evidence that it accounts for what the sweeps add to plain fp32 rounding), all on the same tape.

    ``rowwise``: tensors that are compared per leading row as well (each trajectory's y0 gradient
    against its own scale: over a long horizon the rows span nine decades), under the key
    ``name + "/row"`` with a scale and a Y per row.  A row is WELL CHOSEN where its own bar
    4 Y + 1e-5 scale fits under the cap; the others are ill-conditioned in fp32 itself (the fp32 replay
    alone misses them) and stay under the tensor's max-norm bar only."""

    def __init__(self, sd, widths, y0, t, method, options, state0, tape, cotangent, n_rerounded=3, seed=4242,
                 rowwise=()):
        args = (widths, y0, t, method, options, state0, tape, cotangent)
        self.g64 = replay_vjp(sd, *args, torch.float64)
        self.rowwise = tuple(rowwise)
        self.scale = self._maxes(self.g64)
        self.Y = {k: torch.zeros_like(s) for k, s in self.scale.items()}
        self.add_reference(replay_vjp(sd, *args, torch.float32))
        for sdp in P.perturbed_state_dicts(sd, n_rerounded, seed=seed):
            self.add_reference(replay_vjp(sdp, *args, torch.float32))
        self.Y_plain = dict(self.Y)   # rounding alone: what decides whether a case is well chosen
        self.add_reference(replay_vjp(sd, *args, torch.float32, logistic="rounded"))

    def _maxes(self, gs):
        out = {k: g.abs().max() for k, g in gs.items()}
        for k in self.rowwise:
            out[k + "/row"] = gs[k].abs().reshape(gs[k].shape[0], -1).amax(1)
        return out

    def dist(self, got):
        """per tensor: max |got - g64| (and per row for the row-wise tensors)"""
        return self._maxes({k: got[k].double().cpu() - g for k, g in self.g64.items()})

    def add_reference(self, run):
        """Widen Y by another equally valid fp32 evaluation of the same replay."""
        for k, d in self.dist(run).items():
            self.Y[k] = torch.maximum(self.Y[k], d)

    def well_chosen(self, k):
        """where the bar of the reference's own rounding error fits under the cap (a mask for a
        row-wise key)"""
        return FACTOR * self.Y_plain[k] + REL * self.scale[k] <= CAP * self.scale[k]

    def bar(self, k):
        """min(4 Y + 1e-5 scale, 1e-4 scale).  Row-wise keys: one relative Y for every row, the worst
        Y / scale over the well-chosen rows (as the state bar of test_gpu_dispatch pools the references
        over the steps: the maximum of five samples per row under-samples the spread of 129 rows)."""
        y = self.Y[k]
        if k.endswith("/row"):
            well = self.well_chosen(k)
            y = (y / self.scale[k].clamp_min(1e-300))[well].max() * self.scale[k] if bool(well.any()) else y
        return torch.minimum(FACTOR * y + REL * self.scale[k], CAP * self.scale[k])

    def report(self, got=None):
        """{"Y": (worst Y / scale, tensor) over the well-chosen entries, "err": (worst err / scale, tensor)
        over the same, "margin": (worst err / bar, tensor), "over": entries beyond the bar, "cap": tensors for which rounding alone exceeds the cap
        (a badly chosen case), "rows": per row-wise key (well-chosen rows, rows, worst err / scale on the
        other rows)}"""
        r = {"Y": (0.0, None), "err": (0.0, None), "margin": (0.0, None), "over": [], "cap": [], "rows": {}}
        d = self.dist(got) if got is not None else None
        for k in self.scale:
            sc = self.scale[k].clamp_min(1e-300)
            well = self.well_chosen(k)
            if k.endswith("/row"):
                rest = float((d[k] / sc)[~well].max()) if d is not None and bool((~well).any()) else 0.0
                r["rows"][k] = (int(well.sum()), well.numel(), rest)
                if not bool(well.any()):
                    continue
            elif not bool(well):
                r["cap"].append((k, float(self.Y_plain[k] / sc)))
                well = torch.ones_like(well)   # still held to the capped bar
            y = float((self.Y[k] / sc)[well].max())
            if y > r["Y"][0]:
                r["Y"] = (y, k)
            if d is not None:
                e = float((d[k] / sc)[well].max())
                if e > r["err"][0]:
                    r["err"] = (e, k)
                mg = float((d[k] / self.bar(k).clamp_min(1e-300))[well].max())
                if mg > r["margin"][0]:
                    r["margin"] = (mg, k)
                if bool((d[k] > self.bar(k))[well].any()):
                    r["over"].append((k, e, float((self.bar(k) / sc)[well].min())))
        return r
