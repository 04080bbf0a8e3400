"""The host glue the three resident dopri5 families share (dopri5.py: _taped_solve, deferred_status,
the two dispatch tables, the wide recogniser), driven on the CPU: a fake launch writes a chosen
(nfev, n_att, status) into stats, stub fields stand for the wide family's failure classes.  The
constants, formulas, texts and orders asserted here are written out from the three hand-written
copies this glue replaced: LV grows an overflowed tape to nfev + 64 / n_att + 16 and remembers
nfev + max(64, nfev // 8) / n_att + max(16, n_att // 8); ECG and wide use 12 / 2."""
import ctypes
import types
import weakref

import pytest
import torch

from fet_ode_amd import _lib
from fet_ode_amd import dopri5 as D5

FAMILIES = {   # rule, (evaluations, attempts) added, the attribute, the timeout text
    "lv": (D5._LV_TAPE, (64, 16), "_fetode_d5tape",
           "fetode_integrate_dopri5_tape: a grid reduction timed out (workgroups not co-resident); "
           "the solution is invalid"),
    "ecg": (D5._ECG_TAPE, (12, 2), "_fetode_d5tape",
            "fetode_ecg_dopri5_tape: a grid barrier timed out (workgroups not co-resident); the solution is invalid"),
    "wide": (D5._WIDE_TAPE, (12, 2), "_fetode_wide_d5tape",
             "fetode_wide_dopri5_tape: a grid barrier timed out (workgroups not co-resident); the solution is invalid"),
}
fam = pytest.mark.parametrize("family", list(FAMILIES))


def SHAPE(cap):   # a family's tape-shape rule
    return (cap * 3, 5)


class Fake:
    """A solve that reports outcomes[i] = (nfev, n_att, status) from its i-th launch."""

    def __init__(self, *outcomes, rc=0):
        self.outcomes, self.rc = list(outcomes), rc
        self.stats = torch.zeros(3, dtype=torch.int32)
        self.events, self.calls, self.first_tape = [], [], None

    def launch(self, cap, max_att, tape, att):
        assert tape.shape == SHAPE(cap) and tape.dtype == torch.float32
        assert att.shape == (max_att, 4) and att.dtype == torch.float64
        if self.first_tape is None:
            self.first_tape = weakref.ref(tape)
        self.events.append("launch")
        self.calls.append((cap, max_att))
        self.stats.copy_(torch.tensor(self.outcomes[len(self.calls) - 1], dtype=torch.int32))
        return self.rc

    def restore(self):
        self.events.append("restore")

    def on_fail(self):
        self.events.append("on_fail")

    def run(self, family, room, owner=None, **kw):
        self.owner = owner if owner is not None else types.SimpleNamespace()
        return D5._taped_solve(FAMILIES[family][0], self.owner, room, SHAPE, self.stats, self.launch, self.restore, **kw)


@fam
@pytest.mark.parametrize("nfev,n_att", [(50, 7), (800, 160)])   # below and above the n // 8 slack
def test_fitting_solve_launches_once_and_remembers_the_size(family, nfev, n_att):
    _, (ge, ga), attr, _ = FAMILIES[family]
    s = Fake((nfev, n_att, 0))
    D5.dopri5_solve.last = None
    tape, att, got_ev, got_att, cap = s.run(family, (1000, 200))
    assert s.events == ["launch"] and s.calls == [(1000, 200)]
    assert (got_ev, got_att, cap) == (nfev, n_att, 1000) and tape.shape == SHAPE(1000) and att.shape[0] == 200
    assert getattr(s.owner, attr) == (nfev + max(ge, nfev // 8), n_att + max(ga, n_att // 8))
    last = D5.dopri5_solve.last
    assert isinstance(last, D5.ResidentSolve) and last.nfev == nfev and last.n_attempts == n_att


@fam
@pytest.mark.parametrize("nfev,n_att", [(130, 20), (90, 60)], ids=["nfev", "n_att"])
def test_overflow_restores_once_frees_the_tape_and_reruns_with_room(family, nfev, n_att, monkeypatch):
    _, (ge, ga), attr, _ = FAMILIES[family]
    s = Fake((nfev, n_att, 0), (nfev, n_att, 0))
    alive_at_alloc = []
    empty = torch.empty

    def spy(*a, **kw):
        if s.first_tape is not None:   # every allocation after the first launch
            alive_at_alloc.append(s.first_tape() is not None)
        return empty(*a, **kw)

    monkeypatch.setattr(torch, "empty", spy)
    tape, att, got_ev, got_att, cap = s.run(family, (100, 50))
    monkeypatch.undo()
    assert s.events == ["launch", "restore", "launch"]
    assert s.calls == [(100, 50), (nfev + ge, n_att + ga)] and cap == nfev + ge
    assert alive_at_alloc and not any(alive_at_alloc), "the first tape outlived the re-run's allocation"
    assert tape.shape == SHAPE(nfev + ge) and att.shape[0] == n_att + ga
    assert getattr(s.owner, attr) == (nfev + max(ge, nfev // 8), n_att + max(ga, n_att // 8))


@fam
@pytest.mark.parametrize("status,text", [(1, "non-finite values in state `y`"), (2, "underflow in dt"),
                                         (3, "max_num_steps exceeded")])
def test_torchdiffeq_assertions_keep_the_last_memory(family, status, text):
    s = Fake((40, 6, status))
    D5.dopri5_solve.last = None
    with pytest.raises(AssertionError) as e:
        s.run(family, (100, 50), on_fail=s.on_fail)
    assert str(e.value) == text
    assert s.events == ["launch", "on_fail"]   # no restore; the family's hook ran before the raise
    assert not hasattr(s.owner, FAMILIES[family][2]) and D5.dopri5_solve.last is None


@fam
def test_timeout_restores_then_raises_the_family_text(family):
    s = Fake((40, 6, 4))
    with pytest.raises(RuntimeError) as e:
        s.run(family, (100, 50), on_fail=s.on_fail)
    assert str(e.value) == FAMILIES[family][3] and not isinstance(e.value, AssertionError)
    assert s.events == ["launch", "restore", "on_fail"]


@fam
def test_unsupported_declines_or_is_an_error(family):
    s = Fake((0, 0, 0), rc=_lib.FETODE_EUNSUPPORTED)
    with pytest.raises(NotImplementedError if family == "lv" else D5._Declined) as e:   # LV: _lib.check's
        s.run(family, (100, 50))
    if family == "lv":
        assert str(e.value).startswith("fetode_integrate_dopri5_tape: ")
    assert s.events == ["launch"] and not hasattr(s.owner, FAMILIES[family][2])


def test_wide_budget_declines_after_one_launch_with_the_grown_size():
    per_ev = 15
    budget = 120 * per_ev * 4   # room for 120 evaluations; the re-run needs 130 + 12
    asked = []

    def fits(cap, max_att):
        asked.append((cap, max_att))
        return cap * per_ev * 4 <= budget

    s = Fake((130, 20, 0))
    with pytest.raises(D5._Declined):
        s.run("wide", (100, 50), fits=fits)
    assert s.events == ["launch", "restore"] and asked == [(142, 22)]
    assert s.owner._fetode_wide_d5tape == (142, 22)
    s = Fake((105, 20, 0), (105, 20, 0))   # within it: the re-run goes ahead
    s.run("wide", (100, 50), fits=fits)
    assert s.calls == [(100, 50), (117, 22)]


def test_wide_tape_fits_is_the_budget_rule(monkeypatch):
    class Lib:
        sweep = 1000

        def fetode_wide_dopri5_backward_workspace(self, *a):
            self.args = a[4:]
            return self.sweep

    lib, e = Lib(), (None, ctypes.c_int(), ctypes.c_int())
    monkeypatch.setattr(D5, "_WIDE_RESIDENT_TRAIN", [True, 10 * 7 * 4 + 1000])
    assert D5._wide_tape_fits(lib, e, e, 3, 7, 10, 5) and lib.args == (3, 5)
    assert not D5._wide_tape_fits(lib, e, e, 3, 7, 11, 5)
    lib.sweep = -1   # no sweep workspace at all
    assert not D5._wide_tape_fits(lib, e, e, 3, 7, 1, 5)


def test_tape_room_is_the_previous_solve_or_the_first_guess():
    o = types.SimpleNamespace()
    assert D5._tape_room(o, "_fetode_d5tape") == (256, 64)
    o._fetode_d5tape = (0, -3)
    assert D5._tape_room(o, "_fetode_d5tape") == (1, 1)
    o._fetode_d5tape = (77, 9)
    assert D5._tape_room(o, "_fetode_d5tape") == (77, 9)


def _stats(status):
    return torch.tensor([0, 0, status], dtype=torch.int32)


def test_deferred_status_queues_and_raises_the_first_failure_on_exit():
    with pytest.raises(AssertionError, match="max_num_steps exceeded"):
        with D5.deferred_status():
            D5._status_check(_stats(0), "t")
            D5._status_check(_stats(3), "t")   # raises nothing inside the context
            D5._status_check(_stats(1), "t")
            assert len(D5._DEFERRED) == 3
    assert D5._DEFERRED == []
    with pytest.raises(AssertionError, match="underflow in dt"):   # outside: at once
        D5._status_check(_stats(2), "t")


def test_deferred_status_drops_its_queue_when_an_exception_passes():
    with pytest.raises(KeyError):
        with D5.deferred_status():
            D5._status_check(_stats(2), "t")
            raise KeyError("other")
    assert D5._DEFERRED == []
    D5.check_deferred()   # nothing left to raise


INFER = ["_try_ecg_resident", "_try_field_resident", "_try_wide_resident"]
TRAIN = ["_try_ecg_resident_train", "_try_wide_resident_train", "_try_field_resident_train"]


@pytest.fixture
def tried(monkeypatch):
    """Every try-function of the two tables replaced by one that records its name and returns None;
    the host solvers by stubs; every switch on (and put back)."""
    names = []

    def recorder(name):
        def rec(*request):
            assert len(request) == 7
            names.append(name)
        return rec

    for name in INFER + TRAIN:   # the tables hold names: rebinding a try-function reaches dopri5_solve
        monkeypatch.setattr(D5, name, recorder(name))

    class Host:
        def __init__(self, *a, **kw):
            names.append(type(self).__name__)

        def integrate(self, tp):
            return "host"

    monkeypatch.setattr(D5, "_Dopri5", type("_Dopri5", (Host,), {}))
    monkeypatch.setattr(D5, "_Dopri5Grad", type("_Dopri5Grad", (Host,), {}))
    setters = (D5.set_resident_dopri5, D5.set_wide_resident_dopri5, D5.set_resident_ecg_training,
               D5.set_resident_wide_training, D5.set_resident_dopri5_training)
    prev = [s(True) for s in setters]
    yield names
    for s, p in zip(setters, prev):
        s(p)
    D5.dopri5_solve.last = None


def _solve(names, grad):
    del names[:]
    y0 = torch.zeros(2, 2, requires_grad=grad)
    with torch.set_grad_enabled(grad):
        assert D5.dopri5_solve(lambda t, y: y, y0, None, torch.tensor([0.0, 1.0]), False, 1e-3, 1e-4, {}) == "host"
    return list(names)


def test_dispatch_order(tried):
    assert _solve(tried, False) == INFER + ["_Dopri5"]
    assert _solve(tried, True) == INFER + TRAIN + ["_Dopri5Grad"]


@pytest.mark.parametrize("setter,gone", [
    ("set_wide_resident_dopri5", ["_try_wide_resident"]), ("set_resident_ecg_training", ["_try_ecg_resident_train"]),
    ("set_resident_wide_training", ["_try_wide_resident_train"]),
    ("set_resident_dopri5_training", ["_try_field_resident_train"]), ("set_resident_dopri5", INFER + TRAIN)])
def test_each_switch_removes_its_own_entry(tried, setter, gone):
    assert getattr(D5, setter)(False) is True
    assert _solve(tried, True) == [n for n in INFER + TRAIN if n not in gone] + ["_Dopri5Grad"]


# ---- the wide recogniser: which failures return before a sharded request's vote, which vote no

def _wide_func(D=4, H=6, out=None, k1_in=None, nb=(5, 5), n_layers=2, bsign=None, noise=False, has_ferro=True,
               grad=False):
    def layer(i, o, nbasis):
        return types.SimpleNamespace(kan=types.SimpleNamespace(in_features=i, out_features=o),
                                     ferro=types.SimpleNamespace(_bsign=bsign, use_noise=noise, num_basis=nbasis))
    layers = [layer(D, H, nb[0]), layer(H if k1_in is None else k1_in, D if out is None else out, nb[1])]
    layers += [layer(D, D, nb[0])] * (n_layers - 2)
    p = torch.zeros(1, requires_grad=grad)
    field = types.SimpleNamespace(has_ferro=has_ferro, layers=layers, parameters=lambda: iter([p]))
    return types.SimpleNamespace(_fetode_field=field)


@pytest.fixture
def vote(monkeypatch):
    """resident_agreement and wide_plan recorded: votes[i] = the ok a rank passed in; the agreement
    is None (the group takes the host loop), so no launch follows."""
    from fet_ode_amd import autograd_ops
    from fet_ode_amd import dist
    rec = types.SimpleNamespace(votes=[], plans=0, plan=None)

    def agreement(group, device, batch, ok):
        assert type(ok) is bool
        rec.votes.append(ok)
        return None

    def wide_plan(kan, fer, device, parts=None):
        rec.plans += 1
        return rec.plan

    monkeypatch.setattr(dist, "resident_agreement", agreement)
    monkeypatch.setattr(dist, "_RESIDENT_SHARDED", [True])
    monkeypatch.setattr(autograd_ops, "wide_plan", wide_plan)
    return rec


def _try_wide(func, y0, group="world", reversed_=False, **opts):
    options = dict(opts, norm_group=group) if group is not None else opts
    return D5._try_wide_resident(func, y0, torch.tensor([0.0, 1.0]), reversed_, 1e-3, 1e-4, options)


Y0 = torch.zeros(3, 4)
NO_VOTES = {
    "chain in": dict(func=_wide_func(D=5)), "chain hidden": dict(func=_wide_func(k1_in=7)),
    "chain out": dict(func=_wide_func(out=3)), "num_basis": dict(func=_wide_func(nb=(5, 6))),
    "empty shard": dict(func=_wide_func(), y0=torch.zeros(0, 4)),
    "y0 requires grad": dict(func=_wide_func(), y0=torch.zeros(3, 4, requires_grad=True)),
    "parameter requires grad": dict(func=_wide_func(grad=True)),
    "no plan": dict(func=_wide_func()),
    "no plan, a batch inside the single-device gap": dict(func=_wide_func(), y0=torch.zeros(1000, 4)),
}
EARLY = {
    "no tagged field": dict(func=lambda t, y: y), "state not (B, D)": dict(func=_wide_func(), y0=torch.zeros(3, 2, 2)),
    "reversed": dict(func=_wide_func(), reversed_=True), "a non-scalar option": dict(func=_wide_func(), step_t=[0.5]),
    "no has_ferro": dict(func=_wide_func(has_ferro=False)), "three layers": dict(func=_wide_func(n_layers=3)),
    "branch-sign buffer": dict(func=_wide_func(bsign=torch.ones(3, 4))), "noise": dict(func=_wide_func(noise=True)),
}


@pytest.mark.parametrize("case", list(NO_VOTES))
def test_wide_failures_that_vote_no_in_a_sharded_request(vote, case):
    kw = dict(NO_VOTES[case])
    assert _try_wide(kw.pop("func"), kw.pop("y0", Y0), **kw) is None
    assert vote.votes == [False]
    assert vote.plans == (2 if case.startswith("no plan") else 0)   # the plans only once the shapes agree


@pytest.mark.parametrize("case", list(EARLY))
def test_wide_failures_that_return_before_the_vote(vote, case):
    kw = dict(EARLY[case])
    assert _try_wide(kw.pop("func"), kw.pop("y0", Y0), **kw) is None
    assert vote.votes == [] and vote.plans == 0


def test_wide_eligible_rank_votes_yes_and_the_switch_votes_no(vote, monkeypatch):
    from fet_ode_amd import dist
    vote.plan = ("plan", "kan desc", "ferro desc")
    assert _try_wide(_wide_func(), Y0) is None
    monkeypatch.setattr(dist, "_RESIDENT_SHARDED", [False])
    assert _try_wide(_wide_func(), Y0) is None
    assert vote.votes == [True, False]


def test_wide_single_device_failures_return_without_a_vote(vote):
    for case, kw in NO_VOTES.items():
        kw = dict(kw)
        assert _try_wide(kw.pop("func"), kw.pop("y0", Y0), group=None, **kw) is None, case
    assert vote.votes == []
    before = vote.plans
    assert _try_wide(_wide_func(), torch.zeros(1000, 4), group=None) is None   # inside _WIDE_RESIDENT_GAP
    assert vote.plans == before


def test_wide_training_recognition_shares_the_stages(vote, monkeypatch):
    """_try_wide_resident_train: the same stage-1 classes return None, norm_group is no scalar option,
    a frozen parameter and a missing plan return None — none of them votes."""
    from fet_ode_amd import autograd_ops
    w = torch.zeros(1, requires_grad=True)
    monkeypatch.setattr(autograd_ops, "kan_params", lambda k: [w, None])
    monkeypatch.setattr(autograd_ops, "FERRO_PARAM_NAMES", ("num_basis_p",))
    tp = torch.tensor([0.0, 1.0])

    def func(frozen=False, **kw):
        f = _wide_func(**kw)
        for l in f._fetode_field.layers:
            l.ferro.num_basis_p = torch.zeros(1, requires_grad=not frozen)
        return f

    for f, opts in ((func(has_ferro=False), {}), (func(n_layers=3), {}), (func(), {"norm_group": "world"}),
                    (func(D=5), {}), (func(frozen=True), {})):
        assert D5._try_wide_resident_train(f, Y0, tp, False, 1e-3, 1e-4, opts) is None
    assert vote.plans == 0
    assert D5._try_wide_resident_train(func(), Y0, tp, False, 1e-3, 1e-4, {}) is None
    assert vote.plans == 2 and vote.votes == []
