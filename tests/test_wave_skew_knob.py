"""The two scheduling knobs of the KAN-FET rk4 inference kernel (fetode_fused_set_wave_skew,
fetode_fused_set_wave_prio): setter contracts and the environment variables, host code only."""
import ctypes
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "fet-ode_amd", "libfetode.so")
SKEW_MAX, SKEW_DEFAULT, PRIO_DEFAULT = 127, 0, 67


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(REPO, "fet-ode_amd", "csrc")], check=True)
    lib = ctypes.CDLL(LIB)
    for name in ("fetode_fused_set_wave_skew", "fetode_fused_set_wave_prio"):
        f = getattr(lib, name)
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int]
    return lib


def test_wave_skew_setter(lib):
    """0..127 sets, larger values clamp to s_sleep's range, a negative argument only queries; the previous
    value comes back."""
    f = lib.fetode_fused_set_wave_skew
    prev = f(-1)
    try:
        assert 0 <= prev <= SKEW_MAX and f(-1) == prev
        assert f(19) == prev and f(-1) == 19
        assert f(-7) == 19 and f(-(1 << 20)) == 19 and f(-1) == 19
        assert f(SKEW_MAX) == 19 and f(-1) == SKEW_MAX
        assert f(SKEW_MAX + 1) == SKEW_MAX and f(-1) == SKEW_MAX
        assert f(1) == SKEW_MAX and f(1 << 20) == 1 and f(-1) == SKEW_MAX
        assert f(0) == SKEW_MAX and f(-1) == 0
    finally:
        f(prev)


def test_wave_prio_setter(lib):
    """0..100 sets, anything else only queries; the previous value comes back."""
    f = lib.fetode_fused_set_wave_prio
    prev = f(-1)
    try:
        assert 0 <= prev <= 100 and f(-1) == prev
        assert f(50) == prev and f(-1) == 50
        for bad in (-7, 101, 1 << 20):
            assert f(bad) == 50
        assert f(100) == 50 and f(0) == 100 and f(-1) == 0
    finally:
        f(prev)


def _fresh(var, env, fn):
    e = {k: v for k, v in os.environ.items() if k not in ("FETODE_WAVE_SKEW", "FETODE_WAVE_PRIO")}
    if env is not None:
        e[var] = env
    code = f"import ctypes; print(ctypes.CDLL({LIB!r}).{fn}(-1))"
    return int(subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout)


@pytest.mark.parametrize("env,expect", [(None, SKEW_DEFAULT), ("0", 0), ("1", 1), ("19", 19), ("127", 127),
                                        ("128", SKEW_MAX), ("100000", SKEW_MAX), ("-3", 0), ("x", SKEW_DEFAULT),
                                        ("19x", SKEW_DEFAULT), ("", SKEW_DEFAULT)])
def test_wave_skew_env(lib, env, expect):
    """FETODE_WAVE_SKEW is read once at load: a whole number is clamped to 0..127, anything else leaves
    the default."""
    assert _fresh("FETODE_WAVE_SKEW", env, "fetode_fused_set_wave_skew") == expect


@pytest.mark.parametrize("env,expect", [(None, PRIO_DEFAULT), ("0", 0), ("50", 50), ("100", 100),
                                        ("101", PRIO_DEFAULT), ("-1", PRIO_DEFAULT), ("x", PRIO_DEFAULT),
                                        ("", PRIO_DEFAULT)])
def test_wave_prio_env(lib, env, expect):
    """FETODE_WAVE_PRIO is read once at load: a whole number 0..100 is taken, anything else leaves the
    default."""
    assert _fresh("FETODE_WAVE_PRIO", env, "fetode_fused_set_wave_prio") == expect
