"""The layer-0 Ferro operands of the fused [2, 10, 2] kernels (fetode_fused.hip, v4_edges): every
pair round and the single element of a lane take the {e, w, x} row of ONE input, and the batched form
reads all of a lane's rows ahead of the rounds and binds each round to its own.  A round bound to
another round's row evaluates an element of input 0 with input 1's x, gate factor and exp(gs x) (or
the single element with a pair's row).  With all 100 x 2 elements summed, other tests see that as one
wrong term among many; here each of the 20 (input i, element k) slots of layer 0 is isolated: layer 0's
Ferro output coefficient is zeroed for every other slot, so only the elements (i, :, k) reach the
hidden units' Ferro sums.  The rows of y0 have strongly different components, so the other input's
row is an O(1) error in the slot's term; the CPU test below asserts from the oracle that each slot's
term is far above the 1e-5 bars, so a lost or swapped term cannot pass unnoticed.

Both gate forms: the plan factors exp(gs (x + Ec)) while |gs log2e Ec| <= 60 over a layer; one layer-0
Ec of 4.5 (gs = 10: 64.9) sends both layers to the unfactored form.
"""
import functools

import pytest
import torch

SEED = 0
D, H, K = 2, 10, 10
Y0 = [[0.5, 3.0], [3.0, 0.5], [-0.7, 1.9]]   # B = 3: one full two-trajectory wave and a half-filled one
SLOTS = [(i, k) for i in range(D) for k in range(K)]
GATES = ["factored", "unfactored"]
EC_BIG = 4.5   # 10 * log2(e) * 4.5 = 64.9 > 60: the plan's guard fails


@functools.lru_cache(maxsize=None)
def _base(gate):
    import fet_ode_amd as F
    torch.manual_seed(SEED)
    m = F.KANFET([D, H, D], grid_size=5)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    if gate == "unfactored":
        sd["layers.0.ferro.Ec"][1, H - 1, K - 1] = EC_BIG
    return sd


def _isolated(gate, slot):
    """the state dict with layer 0's Ferro coefficient kept for slot (i, k) only (all outputs)"""
    i, k = slot
    sd = {n: v.clone() for n, v in _base(gate).items()}
    coef = torch.zeros_like(sd["layers.0.ferro.coef"])
    coef[i, :, k] = sd["layers.0.ferro.coef"][i, :, k]
    sd["layers.0.ferro.coef"] = coef
    return sd


def _oracle(sd):
    from oracle import torch_ref as O
    return O.KANFETRef.from_state_dict(sd, 2)


def _t():
    return torch.linspace(0, 3.5, 35, dtype=torch.float64)[:3]   # 2 rk4 steps: 8 evaluations


@functools.lru_cache(maxsize=None)
def _refs(gate):
    """per slot: (field(y0), the 2-step rk4 solution), from the oracle; computed once per gate form"""
    from oracle import torch_ref as O
    y = torch.tensor(Y0)
    out = {}
    with torch.no_grad():
        for slot in SLOTS:
            sd = _isolated(gate, slot)
            f = _oracle(sd)(y)
            s, _ = O.rk4_with_states(_oracle(sd), y, _t())
            out[slot] = (f, s)
    return out


@pytest.mark.parametrize("gate", GATES)
def test_oracle_isolated_slot_terms_are_far_above_the_bar(gate):
    """Each isolated slot's Ferro term reaches some hidden unit with >= 1e-2 (1000 x the 1e-5 bar),
    changes by >= 1e-2 when the two components of a row are exchanged (the wrong input's row), and
    moves the field's output by >= 1e-3 (100 x the bar) against the same model without the slot."""
    from oracle import torch_ref as O
    y = torch.tensor(Y0)
    worst = [1e30, 1e30, 1e30]
    for slot in SLOTS:
        sd = _isolated(gate, slot)
        ref = _oracle(sd)
        with torch.no_grad():
            term = O.ferro_forward(y, ref.ferro[0], _oracle(sd).states[0])
            term_sw = O.ferro_forward(y.flip(-1), ref.ferro[0], _oracle(sd).states[0])
            f = _oracle(sd)(y)
            sd0 = dict(sd)
            sd0["layers.0.ferro.coef"] = torch.zeros_like(sd["layers.0.ferro.coef"])
            f0 = _oracle(sd0)(y)
        a, b, c = term.abs().max().item(), (term - term_sw).abs().max().item(), (f - f0).abs().max().item()
        print(f"{gate} slot {slot}: hidden term {a:.3e}, against the exchanged row {b:.3e}, output {c:.3e}")
        worst = [min(worst[0], a), min(worst[1], b), min(worst[2], c)]
        assert a >= 1e-2 and b >= 1e-2 and c >= 1e-3, (slot, a, b, c)
    print(f"{gate}: smallest over the slots {worst}")


def _model(sd, dev):
    import fet_ode_amd as F
    m = F.KANFET([D, H, D], grid_size=5)
    m.load_state_dict(sd)
    return m.to(dev)


def _slice_rel_err(a, b):
    a = a.double().reshape(a.shape[0], -1)
    b = b.double().reshape(b.shape[0], -1)
    return ((a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)).max().item()


# default: whatever the dispatch picks at this batch; the two fused4 lane maps forced at every batch
KERNELS = {"default": None,
           "two-per-wave": dict(small=0, tpw1=(0, 0), v8=(0, 0)),
           "one-per-wave": dict(small=0, tpw1=(0, 1 << 40), v8=(0, 0))}


@pytest.mark.gpu
@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_isolated_layer0_ferro_slots_vs_oracle(dev, kernel, gate):
    """All 20 slots, one field evaluation and a 2-step rk4 solve each (the gate state w differs
    between the inputs from the second evaluation on); every slot is checked, failures listed."""
    import fet_ode_amd as F
    from conftest import fused_ranges
    y = torch.tensor(Y0)
    bad = []
    worst_f = worst_s = 0.0
    with fused_ranges() as fr:
        if KERNELS[kernel] is not None:
            fr.set(**KERNELS[kernel])
        for slot in SLOTS:
            f_ref, s_ref = _refs(gate)[slot]
            sd = _isolated(gate, slot)
            with torch.no_grad():
                f_gpu = _model(sd, dev)(y.to(dev)).cpu()
                s_gpu = F.odeint(F.autonomous(_model(sd, dev)), y.to(dev), _t(), method="rk4").cpu()
            nan_ok = torch.equal(torch.isnan(f_gpu), torch.isnan(f_ref)) and \
                torch.equal(torch.isnan(s_gpu), torch.isnan(s_ref))
            d = (torch.nan_to_num(f_gpu).double() - torch.nan_to_num(f_ref).double()).abs()
            f_ok = bool((d <= 1e-5 * torch.nan_to_num(f_ref).double().abs() + 1e-5).all())
            err = _slice_rel_err(s_gpu, s_ref)
            worst_f, worst_s = max(worst_f, d.max().item()), max(worst_s, err)
            if not (nan_ok and f_ok and err <= 1e-5):
                bad.append((slot, nan_ok, d.max().item(), err))
    print(f"{kernel} {gate}: field max abs diff {worst_f:.3e}, rk4 2 steps max slice rel err {worst_s:.3e}")
    assert torch.isfinite(torch.stack([s for _, s in _refs(gate).values()])).all()
    assert not bad, bad
