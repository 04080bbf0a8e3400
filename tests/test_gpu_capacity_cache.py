"""The shared resident-capacity cache (fetode_common.hip: device_cus / occupancy_per_cu /
resident_wgs) is keyed by (device, kernel, threads, dynamic LDS bytes).  Keyed too coarsely, a query
would come back with another kernel's or another LDS size's answer once that one is cached: so every
capacity export is asked twice in one process, the questions interleaved, and then alone in a fresh
process, and must give the same positive number each time.  The queries launch no kernel; the
descriptors carry fake pointers.

Run as a script with one query's name, the module prints that query's answer (the child processes)."""
import ctypes
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000
# two ECG layers whose in_dim * num_basis, and so the sweep's dynamic LDS, differ
ECG_LAYERS = {"ecg 8x10": (8, 10), "ecg 64x12": (64, 12)}


def _field(L, H, ferro):
    """A [2, H, 2] descriptor (K = 10) with fake device pointers: never dereferenced by the queries."""
    kan = (L.KANLinearDesc * 2)()
    fer = (L.FerroDesc * 2)()
    for l, (i, o) in enumerate(((2, H), (H, 2))):
        kan[l] = L.KANLinearDesc(i, o, 5, 3, 10, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0)
        fer[l] = L.FerroDesc(i, o, 10, FAKE, FAKE, FAKE, FAKE, FAKE, 10.0, 0.8, None, 0)
    f = L.FieldDesc(2, kan, fer if ferro else None)
    f._keep = (kan, fer)
    return f


def queries():
    """name -> a function that asks the library; in a fixed order."""
    import fet_ode_amd as F
    L = F._lib
    lib = L.load()
    fields = {"kanfet [2,10,2]": _field(L, 10, True), "kan [2,10,2]": _field(L, 10, False),
              "kanfet [2,12,2]": _field(L, 12, True), "kan [2,12,2]": _field(L, 12, False)}
    q = {}
    for name, f in fields.items():
        for sharded in (0, 1):
            q[f"fwd {name} sharded={sharded}"] = (
                lambda f=f, s=sharded: lib.fetode_integrate_dopri5_max_batch(ctypes.byref(f), s))
        q[f"bwd {name}"] = lambda f=f: lib.fetode_integrate_dopri5_backward_max_batch(ctypes.byref(f))
    for name, (in_dim, nb) in ECG_LAYERS.items():
        layer = L.HLogisticDesc(in_dim, nb, FAKE, FAKE, FAKE, FAKE, 5.0, 0.5)
        q[name] = lambda layer=layer: lib.fetode_ecg_dopri5_backward_max_batch(ctypes.byref(layer))
    return q


@pytest.mark.gpu
def test_capacity_answers_repeat_and_match_a_fresh_process(dev):
    q = queries()
    names = list(q)
    first = {n: q[n]() for n in names}
    second = {n: q[n]() for n in reversed(names)}     # every kernel's answer is cached by now
    third = {n: q[n]() for n in names[1::2] + names[0::2]}
    print(first)
    assert all(v > 0 for v in first.values()), first
    assert second == first and third == first, (first, second, third)
    # the exchange workgroup of a sharded launch takes one workgroup's trajectories
    for n in names:
        if "sharded=1" in n:
            assert first[n] < first[n.replace("sharded=1", "sharded=0")], (n, first)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO] + [p for p in sys.path if p]))
    for n in ("ecg 8x10", "ecg 64x12", "bwd kanfet [2,12,2]"):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), n], env=env, capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, (n, out.stdout, out.stderr)
        assert int(out.stdout.split()[-1]) == first[n], (n, out.stdout, first[n])


if __name__ == "__main__":
    print(queries()[sys.argv[1]]())
