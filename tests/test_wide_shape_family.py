"""The shape family of the wide-layer kernels (fetode_wide.hip), host side only: what
fetode_wide_layer_supported admits and refuses, the size of the packed plan, and which admitted
shapes have the MFMA KANLinear VJP.  The shape lists below ARE the parametrisation of
tests/test_gpu_wide_shapes.py and of the resident-solver cases in tests/test_gpu_wide_dopri5.py
(imported from here), so the GPU cases and the predicate cannot drift apart: a shape that stops
being admitted fails here, without a GPU, before it silently runs the generic kernels there.

wide_supported(): in >= 16, in % 8 == 0, out >= 16, out % 16 == 0, grid_size 5 / cubic / 10
logistic bases for the KANLinear, K = 10 or 12 for the Ferro layer, equal (in, out) when both.
"""
import pytest

import fet_ode_amd as F

L = F._lib
FAKE = 0x1000   # non-null "device pointers": only host code runs

# ---------------------------------------------------------------------------------------------
# the GPU parametrisation (each entry: shape, then the branch it is there for)
# ---------------------------------------------------------------------------------------------

# layer forward (KANLinear alone, Ferro alone at K = 10 and 12, both in one launch).  S = input
# slices at B <= 300 (wide_slices), chunks = 8-input chunks each slice's workgroup walks.
FORWARD_SHAPES = [
    (16, 16),     # both minima; S = 2, one chunk per slice (no prefetch iteration); grid.y = 1
    (24, 48),     # S = 1 always, 3 chunks (odd: the loop ends on parameter buffer 1); grid.y = 3
    (32, 64),     # S = 4: the slab path (> 2 slices), single-chunk slices
    (40, 80),     # S = 1, 5 chunks; 5 output blocks
    (72, 16),     # S = 1, 9 chunks; one output block: a small tile walked by one workgroup
    (136, 144),   # both beyond 128; S = 1, 17 chunks; grid.y = 9
]
FORWARD_BATCHES = [1, 37, 100, 300]   # one row | partial first tile | partial second tile | 5 tiles

# one-pass Ferro VJP.  K = 10: 3 outputs per 16-lane group, K = 12: 2; two groups per wave.
FERRO_BWD_SHAPES = [
    (16, 16),     # K = 10: 6 groups, 1-output tail, 3 group blocks; K = 12: 8 groups, 4 blocks
    (24, 48),     # K = 10: 16 groups, exact, 8 blocks
    (40, 80),     # K = 10: 27 groups, 2-output tail, 14 blocks whose last holds one group
    (72, 16),     # many inputs over the 1-output tail
    (136, 144),   # both beyond 128; K = 10: 48 groups, exact
]
FERRO_BWD_BATCHES = [37, 100, 300]

# MFMA KANLinear VJP (out = 64 -> wide_kan_gx_kernel<16>, 128 -> <32>); nch = in / 4 input quads
KAN_BWD_SHAPES = [
    (16, 64),     # nch = 4: one workgroup per row group; 20 feature-column tiles
    (24, 128),    # nch = 6: a workgroup spans two row groups' tasks (4 waves over 6 quads)
    (40, 64),     # nch = 10
    (72, 128),    # nch = 18
    (136, 64),    # in beyond 128: nch = 34
]
KAN_BWD_BATCHES = [1, 37, 100]

# whole fields under autograd: layer 0 through _WideLayerFn, layer 1 (out = in of layer 0, not 64 /
# 128) through the generic KANLinear VJP and the one-pass Ferro VJP
FIELD_SHAPES = [([32, 64, 32], 10), ([16, 128, 16], 12)]

# resident dopri5 (D -> H -> D, K).  Both layers must be admitted, so D and H are multiples of 16;
# then in / 2 is a multiple of 8 and every layer is input-sliced (S >= 2) until its tile count
# passes 512: "whole at a small batch" does not exist inside the admitted family.
DOPRI_SHAPES = [
    (16, 32, 10),   # S0 = 2, S1 = 4: single-chunk slices in both layers, the > 2-slab sums
    (48, 16, 12),   # D > H; S0 = 2 with 3 chunks per slice, S1 = 2; one hidden output block
    (16, 144, 10),  # H beyond 128: 9 hidden output blocks, S1 = 2 with 9 chunks per slice
]
DOPRI_BATCHES = [1, 100]
# pairs whose layer 1 (H -> D) is refused (D % 16 != 0): the solver must take the host loop there
DOPRI_REFUSED = [(24, 48, 12), (40, 16, 10)]

PRODUCTION_SHAPES = [(64, 128), (128, 64), (128, 128)]


def _layers_of_fields():
    out = []
    for widths, K in FIELD_SHAPES:
        out += [(a, b, K) for a, b in zip(widths[:-1], widths[1:])]
    for D, H, K in DOPRI_SHAPES:
        out += [(D, H, K), (H, D, K)]
    return out


ADMITTED = sorted(set(
    [(i, o, K) for i, o in FORWARD_SHAPES + FERRO_BWD_SHAPES + KAN_BWD_SHAPES + PRODUCTION_SHAPES for K in (10, 12)]
    + _layers_of_fields()))


def kan_desc(i, o, grid_size=5, spline_order=3, num_logistic=10):
    return L.KANLinearDesc(i, o, grid_size, spline_order, num_logistic, 0, *[FAKE] * 8, 1.0)


def ferro_desc(i, o, K):
    return L.FerroDesc(i, o, K, *[FAKE] * 5, 10.0, 0.8, None, 0)


def _ref(d):
    return None if d is None else L.ctypes.byref(d)


def supported(kd, fd):
    return F._lib.load().fetode_wide_layer_supported(_ref(kd), _ref(fd))


# ---------------------------------------------------------------------------------------------
# the launch arithmetic, restated (fetode_wide.hip wide_slices / ferro_bwd_plan): what each shape
# above exercises is computed, not asserted by hand
# ---------------------------------------------------------------------------------------------

def wide_slices(wgs, n_in):
    """Input slices of a layer launch with `wgs` (row tile, output block) workgroups."""
    S = 1
    while S < 16 and wgs * S <= 512 and (n_in // (2 * S)) % 8 == 0 and n_in % (2 * S) == 0:
        S *= 2
    return S


def forward_walk(i, o, B):
    """(slices, chunks per slice) of the forward launch."""
    S = wide_slices(-(-B // 64) * (o // 16), i)
    return S, i // S // 8


def ferro_groups(o, K, ogw=2):
    """(output groups, outputs in the last group, group blocks) of the one-pass Ferro VJP."""
    opg = 16 // (K // 2)
    n_og = -(-o // opg)
    return n_og, o - (n_og - 1) * opg, -(-n_og // ogw)


def test_forward_cases_cover_the_chunk_walk():
    walks = {(i, o, B): forward_walk(i, o, B) for i, o in FORWARD_SHAPES for B in FORWARD_BATCHES}
    assert {S for S, _ in walks.values()} == {1, 2, 4}
    chunks = {c for _, c in walks.values()}
    assert 1 in chunks and {3, 5, 9, 17} <= chunks          # a single chunk; odd counts
    assert walks[(16, 16, 300)] == (2, 1) and walks[(32, 64, 1)] == (4, 1) and walks[(72, 16, 300)] == (1, 9)
    # production widths, for contrast: 8 / 16 single-chunk slices at B = 300, even counts at 8192
    assert forward_walk(64, 128, 300) == (8, 1) and forward_walk(128, 64, 300) == (16, 1)
    assert forward_walk(64, 128, 8192) == (1, 8) and forward_walk(128, 64, 8192) == (2, 8)


def test_ferro_vjp_cases_cover_the_group_tails():
    assert ferro_groups(16, 10) == (6, 1, 3)
    assert ferro_groups(48, 10) == (16, 3, 8)
    assert ferro_groups(80, 10) == (27, 2, 14)
    assert ferro_groups(144, 10) == (48, 3, 24)
    tails = {ferro_groups(o, 10)[1] for _, o in FERRO_BWD_SHAPES}
    assert tails == {1, 2, 3}
    assert {ferro_groups(o, 10)[0] % 2 for _, o in FERRO_BWD_SHAPES} == {0, 1}   # a half-filled last block
    assert all(ferro_groups(o, 12)[1] == 2 for _, o in FERRO_BWD_SHAPES)        # K = 12 always divides


def test_dopri_cases_slicing():
    for (D, H, K), want in zip(DOPRI_SHAPES, [(2, 4), (2, 2), (2, 2)]):
        for B in DOPRI_BATCHES:
            rows = -(-B // 64)
            assert (wide_slices(rows * (H // 16), D), wide_slices(rows * (D // 16), H)) == want, (D, H, B)


# ---------------------------------------------------------------------------------------------
# the predicate
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i,o,K", ADMITTED)
def test_admitted(i, o, K):
    assert supported(kan_desc(i, o), None) == 1
    assert supported(None, ferro_desc(i, o, K)) == 1
    assert supported(kan_desc(i, o), ferro_desc(i, o, K)) == 1
    lib = F._lib.load()
    assert lib.fetode_wide_layer_plan_bytes(_ref(kan_desc(i, o)), _ref(ferro_desc(i, o, K))) > 0


REFUSED = [
    ("in = 8", kan_desc(8, 16), ferro_desc(8, 16, 10)),
    ("in = 20", kan_desc(20, 16), ferro_desc(20, 16, 10)),
    ("out = 8", kan_desc(16, 8), ferro_desc(16, 8, 10)),
    ("out = 40", kan_desc(16, 40), ferro_desc(16, 40, 10)),
    ("out = 24", kan_desc(48, 24), ferro_desc(48, 24, 12)),
    ("the generic-kernel shape of test_gpu_wide.py", kan_desc(48, 40), ferro_desc(48, 40, 7)),
]


@pytest.mark.parametrize("why,kd,fd", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_shapes(why, kd, fd):
    lib = F._lib.load()
    for k, f in ((kd, None), (None, fd), (kd, fd)):
        assert supported(k, f) == 0, why
        assert lib.fetode_wide_layer_plan_bytes(_ref(k), _ref(f)) == -1
    assert lib.fetode_kanlinear_backward_wide_workspace(_ref(kd), None, 37) == -1


def test_refused_parameters():
    assert supported(None, ferro_desc(64, 128, 7)) == 0                       # K = 7
    assert supported(kan_desc(64, 128), ferro_desc(64, 128, 7)) == 0
    assert supported(None, ferro_desc(64, 128, 11)) == 0
    assert supported(kan_desc(64, 128, grid_size=6), None) == 0               # grid_size != 5
    assert supported(kan_desc(64, 128, grid_size=6), ferro_desc(64, 128, 10)) == 0
    assert supported(kan_desc(64, 128, spline_order=2), None) == 0
    assert supported(kan_desc(64, 128, num_logistic=8), None) == 0
    assert supported(kan_desc(64, 128), ferro_desc(64, 64, 10)) == 0          # Ferro out != KAN out
    assert supported(kan_desc(64, 128), ferro_desc(32, 128, 10)) == 0         # Ferro in != KAN in
    assert supported(None, None) == 0
    bs = ferro_desc(64, 128, 10)
    bs.branch_sign = FAKE                                                     # an explicit branch_sign
    assert supported(None, bs) == 0


@pytest.mark.parametrize("D,H,K", DOPRI_REFUSED)
def test_resident_solver_pairs_outside_the_family(D, H, K):
    """Layer 0 (D -> H) is admitted, layer 1 (H -> D) is not: no resident solve at these widths."""
    assert supported(kan_desc(D, H), ferro_desc(D, H, K)) == 1
    assert supported(kan_desc(H, D), ferro_desc(H, D, K)) == 0


def test_kan_vjp_workspace():
    """The MFMA KANLinear VJP exists for 64 / 128 outputs only: a positive workspace there, -1 for
    every other admitted shape (kan_backward then takes the generic kernels)."""
    lib = F._lib.load()
    ws = lib.fetode_kanlinear_backward_wide_workspace
    for i, o in KAN_BWD_SHAPES + PRODUCTION_SHAPES:
        for B in KAN_BWD_BATCHES:
            assert ws(_ref(kan_desc(i, o)), None, B) > 0, (i, o, B)
        assert ws(_ref(kan_desc(i, o)), _ref(ferro_desc(i, o, 10)), 37) > 0
        assert ws(_ref(kan_desc(i, o)), None, 0) == 0
    others = [(i, o) for i, o, _ in ADMITTED if o not in (64, 128)]
    assert {(16, 16), (24, 48), (40, 80), (72, 16), (136, 144)} <= set(others)
    for i, o in others:
        assert supported(kan_desc(i, o), None) == 1
        assert ws(_ref(kan_desc(i, o)), None, 37) == -1, (i, o)
    # B = 37 at 16 -> 64, by kan_bwd_plan: features 37 * 320, logistic partials 3 row groups * 16 * 20,
    # weight partials 320 * 64, d/d(2 sigma) 64 * 160, a d/dx scratch 37 * 16 (floats), + 256 bytes
    assert ws(_ref(kan_desc(16, 64)), None, 37) == 4 * (37 * 320 + 3 * 320 + 320 * 64 + 64 * 160 + 37 * 16) + 256


def layout_floats(i, o, K, kan, ferro):
    """WideLayout.end (fetode_wide.hip wide_layout), field by field."""
    n = 0
    if ferro:
        ne = o * i * K
        n += 4 * ne          # fe4: {P, 2 log2e k, 2 log2e k Ec, coef Ps} per element
        n += ne              # gec: gs log2e Ec
        n += o * i           # dflag
    n += o                   # fconst
    n = (n + 3) & ~3
    if kan:
        n += i * 20 * o      # wp: packed weights, 20 features per input
        n += i * 10 * 2      # lg
        n += i * 12          # knots
        n += i * 11          # rh
        n = (n + 3) & ~3
        n += i * 12 * 8 * 4  # bt
        n += i * 64          # par
    return (n + 3) & ~3


@pytest.mark.parametrize("i,o,K", [(24, 48, 10), (136, 144, 12)])
def test_plan_bytes_follow_the_layout(i, o, K):
    lib = F._lib.load()
    pb = lib.fetode_wide_layer_plan_bytes
    assert pb(_ref(kan_desc(i, o)), _ref(ferro_desc(i, o, K))) == 4 * layout_floats(i, o, K, True, True)
    assert pb(_ref(kan_desc(i, o)), None) == 4 * layout_floats(i, o, 0, True, False)
    assert pb(None, _ref(ferro_desc(i, o, K))) == 4 * layout_floats(i, o, K, False, True)
