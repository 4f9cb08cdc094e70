"""The ice-to-air direct ray without a GPU: the n = 1 route of airice_iceair_host on the calling
thread and the drop-in's GetDirectRayPar_Air / fDa_Air.  Header and exports, the argument checks,
the head rows, the physics of 1,000 rows against mpmath, the drop-in bit for bit against the host
route through the caller program, and that program under ASan + UBSan.
Rows, the draw and the physics check: tests/iceair_cases.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import iceair_cases as cases
from tests.conftest import ROOT

SENTINEL = -777.25
N_ROWS = 2000
N_PHYSICS = 1000


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


@pytest.fixture(scope="module")
def host(solver):
    """(rows (n, 3), values (n, 10), status (n)) of the head rows and the draw, computed once."""
    q = cases.batch(N_ROWS, np.random.default_rng(20261021))
    out, st = cases.host_rows(solver, q)
    for a in (q, out, st):
        a.setflags(write=False)
    return q, out, st


@pytest.fixture(scope="module")
def physics(host):
    q, out, st = host
    return cases.physics_errors(q[:N_PHYSICS], out[:N_PHYSICS], st[:N_PHYSICS])


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import AirIceSolver, _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    for name in ("airice_iceair_launch", "airice_iceair_host"):
        assert f"int {name}(const double *model3" in header, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "#define AIRICE_ICEAIR_FIELDS 10" in header
    assert header.count('"iceair_kernel"') == 2  # the timer's and the counter's lists
    assert _lib.launch_count("iceair_kernel") >= 0
    assert _lib.kernel_time("iceair_kernel", reset=False)[1] >= 0
    with open(os.path.join(ROOT, "include", "IceRayTracing.hh")) as f:
        hh = f.read()
    assert "double fDa_Air(double x, void *params);" in hh
    assert "double *GetDirectRayPar_Air(double z0, double x1, double z1);" in hh
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.split()}
    # the reference's mangled names
    assert "_ZN13IceRayTracing7fDa_AirEdPv" in exported
    assert "_ZN13IceRayTracing19GetDirectRayPar_AirEddd" in exported
    assert callable(AirIceSolver.ice_to_air_device) and callable(AirIceSolver.ice_to_air_host)
    assert _lib.ICEAIR_FIELDS == cases.FIELDS


def test_argument_checks_need_no_device():
    """Every AIRICE_EINVAL case of both entries names its argument, before any device call and
    with the outputs untouched; n == 0 is a no-op; no launch counter moves."""
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every launch call below returns first
    before = _lib.launch_count("iceair_kernel")

    def launch(**kw):
        a = dict(model=None, z0=p, x1=p, h=p, n=8, out=p, ld=8, status=None, stream=None)
        a.update(kw)
        return L.airice_iceair_launch(*a.values()), L.airice_last_error().decode()

    assert launch(n=0, z0=None, x1=None, h=None, out=None)[0] == 0
    for name in ("z0", "x1", "h", "out"):
        rc, msg = launch(**{name: None})
        assert rc == -1 and "iceair" in msg and f"({name})" in msg, (name, msg)
    rc, msg = launch(ld=7)
    assert rc == -1 and "ld (7) < n (8)" in msg, msg

    z0, x1, h = (np.array([v, v]) for v in (-100.0, 10.0, 500.0))
    out = np.full((cases.FIELDS, 2), SENTINEL)
    st = np.full(2, 0xAB, dtype=np.uint8)

    def host(**kw):
        a = dict(model=None, z0=z0, x1=x1, h=h, n=2, out=out, ld=2, status=st)
        a.update(kw)
        args = [_lib.ptr(v) if isinstance(v, np.ndarray) else v for v in a.values()]
        return L.airice_iceair_host(*args), L.airice_last_error().decode()

    assert host(n=0, z0=None, x1=None, h=None, out=None)[0] == 0
    for name in ("z0", "x1", "h", "out"):
        rc, msg = host(**{name: None})
        assert rc == -1 and f"({name})" in msg, (name, msg)
    rc, msg = host(ld=1)
    assert rc == -1 and "ld (1) < n (2)" in msg, msg
    assert (out == SENTINEL).all() and (st == 0xAB).all()
    assert _lib.launch_count("iceair_kernel") == before


def test_head_rows_and_the_draw_are_accepted(host):
    """Every finite row is accepted (the issue's draw: all 4,000 of a Python restatement were),
    every search ends within 100 iterations, the rejected receive angle is -1000 only where the
    status bit is clear, and a non-finite input in any slot is status 128 with NaN in columns 0-4
    and 8-9 and no search."""
    q, out, st = host
    n_head, n_bad = len(cases.FINITE_HEAD), len(cases.nonfinite_rows())
    bad = slice(n_head, n_head + n_bad)
    assert (st[bad] == cases.NONFINITE).all()
    assert np.isnan(out[bad][:, [0, 1, 2, 3, 4, 8, 9]]).all()
    assert (out[bad][:, [cases.EVALS, cases.ITERS]] == 0).all()
    fin = np.ones(len(q), dtype=bool)
    fin[bad] = False
    assert (st[fin] == cases.ACCEPTED).all(), np.flatnonzero(fin & (st != cases.ACCEPTED))[:5]
    assert np.array_equal(out[:, cases.STATUS], st.astype(np.float64))
    assert (np.abs(out[fin, cases.CHECKZERO]) <= 0.5).all()
    assert (out[fin, cases.RANG] != -1000).all()
    assert (out[fin, cases.ITERS] <= 100).all() and (out[fin, cases.ITERS] >= 1).all()
    # the two ends, then per iteration the linear point, the bisection point and the moved root
    assert (out[fin, cases.EVALS] <= 2 + 3 * out[fin, cases.ITERS]).all()
    assert (out[fin, cases.LVALUE] > 0).all() and (out[fin, cases.LVALUE] < 1).all()
    print(f"[iceair host] {fin.sum()} rows: mean {out[fin, cases.ITERS].mean():.2f} iterations, "
          f"{(out[fin, cases.ITERS] == 100).sum()} at the limit, "
          f"mean {out[fin, cases.EVALS].mean():.2f} evaluations")
    # the grazing head row leaves within a degree of the surface, the steep one near the vertical
    assert 89 < out[1, cases.RANG] < 90 and out[0, cases.RANG] < 2
    # the physical time is the longer one: the air leg's length against its horizontal reach
    assert (out[fin, cases.PHYS_TIME] > out[fin, cases.TIME]).all()


def test_physics_against_mpmath(physics):
    """No oracle: the ice leg integrated with mpmath at 30 digits, the air leg in closed form.
    Reach within |checkzero| + 1e-9 x1, column 8 within 1.78e-6/c + 1e-12 t, column 9 within
    1e-6 + 1e-12 s, Snell (sin of column 0 is L) to 1e-12 -- on every accepted row of the first
    1,000."""
    assert len(physics) == N_PHYSICS - len(cases.nonfinite_rows())
    r = np.array(physics)
    print(f"[iceair host physics] {len(r)} rows, worst error / bound: reach "
          f"{(r[:, 1] / r[:, 2]).max():.3g}, time {(r[:, 3] / r[:, 4]).max():.3g}, path "
          f"{(r[:, 5] / r[:, 6]).max():.3g}; worst |sin(col 0) - L| {r[:, 7].max():.3g}")
    bad = [b for b in cases.physics_failures(physics) if b[1] != "col2-col8"]
    assert not bad, bad[:5]


def test_reference_time_is_the_physical_time_less_the_air_legs_gap(physics):
    """Column 2 - column 8 = h (L - 1) / (c sqrt(1 - L^2)), to 1e-12 of the time: the reference's
    time adds the air leg's horizontal distance over c, not its length.  (With the tangent taken
    at the reference's rounded air angle this held on 974 of these 991 rows and was off by up to
    2.3e-9 of the time at the grazing ones, while column 8 kept its bound: DESIGN.md §13.)"""
    bad = [b for b in cases.physics_failures(physics) if b[1] == "col2-col8"]
    r = np.array(physics)
    print(f"[iceair host physics] col 2 - col 8: worst {r[:, 8].max():.3g} of the time")
    assert not bad, bad[:5]


def test_dropin_is_the_host_route_bit_for_bit(host):
    """GetDirectRayPar_Air through the caller program on 2,000 rows: its five values are columns
    0-4 of the host route, and fDa_Air at the L it reports is column 4."""
    q, out, _ = host
    got = cases.run_driver("air", q)
    assert got["A"].shape == (N_ROWS, 5) and got["F"].shape == (N_ROWS, 1)
    assert np.array_equal(got["A"], cases.bits(out[:, :5]))
    assert np.array_equal(got["F"][:, 0], cases.bits(out[:, cases.CHECKZERO]))


def test_caller_program_plain_and_under_sanitizers(solver, host):
    """tests/cpp/iceair_driver on its own rows: the head rows' lines are this process's host
    route, the lines after SetA / SetB / SetC the other model's; the ASan + UBSan build (its own
    program, nothing preloaded) prints the same lines and reports nothing -- it delete[]s every
    array the drop-in returned."""
    _, out, _ = host
    plain = subprocess.run([cases.DRIVER], capture_output=True, text=True, check=True)
    assert plain.stderr == "", plain.stderr
    lines = [ln.split() for ln in plain.stdout.splitlines()]
    air = {int(ln[1]): [int(w, 16) for w in ln[2:]] for ln in lines if ln[0] == "A"}
    n_head = len(cases.head_rows())
    for i in range(n_head):
        assert air[i] == cases.bits(out[i, :5]).tolist(), i
    other, _ = cases.host_rows(solver, np.array([cases.FINITE_HEAD[0]]), model=cases.OTHER_MODEL)
    assert air[1000] == cases.bits(other[0, :5]).tolist()
    assert air[1000] != air[0]
    assert sum(ln[0] == "T" for ln in lines) >= 7
    run = subprocess.run([cases.DRIVER_ASAN], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == plain.stdout
