"""The first-arrival tracer without a GPU: the one-pair route of airice_icefirst_host on the
calling thread and the drop-in's DirectRayTracer.  Header and exports, the argument checks, the
reference's rule restated in numpy over the in-ice solver's host rows -- all eight columns bit for
bit -- with the cases the rule turns on, and the drop-in through the caller program.
Points and the rule: tests/iceair_cases.py; the in-ice rows: tests/iceray_cases.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import iceair_cases as cases
from tests import iceray_cases as rays
from tests.conftest import ROOT

KERNELS = ("icefirst_geom_kernel", "iceray_kernel", "icefirst_select_kernel")
SENTINEL = -777.25
N_DRAWN = 2000


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


@pytest.fixture(scope="module")
def pairs(solver):
    """(tx, rx, triples, the solver's host rows, the rule's (n, 8), the host route's (n, 8) and
    status) of the head points and 2,000 drawn pairs with random origins and azimuths."""
    rng = np.random.default_rng(20261022)
    htx, hrx = cases.first_head_points()
    dtx, drx = cases.first_points(rays.drawn(N_DRAWN, rng), rng)
    tx = np.ascontiguousarray(np.concatenate([htx, dtx], axis=1))
    rx = np.ascontiguousarray(np.concatenate([hrx, drx], axis=1))
    triples = cases.first_triples(tx, rx)
    ray_rows, _ = rays.host_rows(solver, triples)
    want = cases.first_rule(ray_rows, triples[:, 1])
    got, st = cases.first_host_rows(solver, tx, rx)
    for a in (tx, rx, triples, ray_rows, want, got, st):
        a.setflags(write=False)
    return tx, rx, triples, ray_rows, want, got, st


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import AirIceSolver, _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    for name in ("airice_icefirst_launch", "airice_icefirst_host"):
        assert f"int {name}(const double *model3" in header, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert "size_t airice_icefirst_work_bytes(size_t n_pairs);" in header
    assert "#define AIRICE_ICEFIRST_FIELDS 8" in header
    for k in (KERNELS[0], KERNELS[2]):
        assert header.count(f'"{k}"') == 2  # the timer's and the counter's lists
        assert _lib.launch_count(k) >= 0 and _lib.kernel_time(k, reset=False)[1] >= 0
    assert _lib.lib().airice_icefirst_work_bytes(10) == 10 * 35 * 8
    with open(os.path.join(ROOT, "include", "IceRayTracing.hh")) as f:
        assert ("double *DirectRayTracer(double xT, double yT, double zT, double xR, double yR, "
                "double zR);") in f.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    assert "_ZN13IceRayTracing15DirectRayTracerEdddddd" in {ln.split()[-1]
                                                            for ln in nm.splitlines() if ln.split()}
    assert callable(AirIceSolver.ice_first_arrivals_device)
    assert callable(AirIceSolver.ice_first_arrivals_host)


def test_argument_checks_need_no_device():
    """Each AIRICE_EINVAL case names its argument and leaves every launch counter and the outputs
    as they were; zero pairs is a no-op."""
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every launch call below returns first
    before = [_lib.launch_count(k) for k in KERNELS]
    need = L.airice_icefirst_work_bytes(8)

    def launch(**kw):
        a = dict(model=None, tx_x=p, tx_y=p, tx_z=p, n_tx=8, rx_x=p, rx_y=p, rx_z=p, n_rx=8,
                 pairing=_lib.PAIRS_ELEMENTWISE, work=p, work_bytes=need, out=p, ld=8, status=None,
                 stream=None)
        a.update(kw)
        return L.airice_icefirst_launch(*a.values()), L.airice_last_error().decode()

    nothing = dict(tx_x=None, tx_y=None, tx_z=None, rx_x=None, rx_y=None, rx_z=None, work=None,
                   out=None, work_bytes=0)
    assert launch(n_tx=0, n_rx=0, **nothing)[0] == 0
    assert launch(n_tx=0, n_rx=5, pairing=_lib.PAIRS_CROSS, **nothing)[0] == 0
    for name in ("tx_x", "tx_y", "tx_z", "rx_x", "rx_y", "rx_z", "work", "out"):
        rc, msg = launch(**{name: None})
        assert rc == -1 and "icefirst" in msg and f"({name})" in msg, (name, msg)
    rc, msg = launch(work_bytes=need - 1)
    assert rc == -1 and f"work_bytes ({need - 1})" in msg, msg
    rc, msg = launch(pairing=_lib.PAIRS_CROSS, work_bytes=8 * need - 1, ld=64)
    assert rc == -1 and f"work_bytes ({8 * need - 1})" in msg, msg
    rc, msg = launch(n_rx=7)
    assert rc == -1 and "n_tx (8) != n_rx (7)" in msg, msg
    for bad in (-1, 2, 99):
        rc, msg = launch(pairing=bad)
        assert rc == -1 and f"pairing {bad}" in msg, msg
    rc, msg = launch(ld=7)
    assert rc == -1 and "ld (7) < n (8)" in msg, msg
    rc, msg = launch(pairing=_lib.PAIRS_CROSS, work_bytes=8 * need, ld=63)
    assert rc == -1 and "ld (63) < n (64)" in msg, msg

    tx = np.array([[0.0, 1.0], [0.0, 1.0], [-180.0, -170.0]])
    rx = np.array([[60.0, 61.0], [80.0, 81.0], [-100.0, -90.0]])
    out = np.full((cases.FIRST_FIELDS, 4), SENTINEL)
    st = np.full(4, 0xAB, dtype=np.uint8)

    def host(**kw):
        a = dict(model=None, tx_x=tx[0], tx_y=tx[1], tx_z=tx[2], n_tx=2, rx_x=rx[0], rx_y=rx[1],
                 rx_z=rx[2], n_rx=2, pairing=_lib.PAIRS_ELEMENTWISE, out=out, ld=4, status=st)
        a.update(kw)
        args = [_lib.ptr(v) if isinstance(v, np.ndarray) else v for v in a.values()]
        return L.airice_icefirst_host(*args), L.airice_last_error().decode()

    for kw in (dict(tx_x=None), dict(tx_y=None), dict(tx_z=None), dict(rx_x=None),
               dict(rx_y=None), dict(rx_z=None), dict(out=None), dict(n_rx=1), dict(pairing=7),
               dict(ld=1), dict(pairing=_lib.PAIRS_CROSS, ld=3)):
        rc, msg = host(**kw)
        assert rc == -1 and msg, (kw, msg)
        assert (out == SENTINEL).all() and (st == 0xAB).all(), kw
    # the choice alone, over a caller's rows: both entries refuse the same things
    for kw, word in ((dict(rays=None), "(rays)"), (dict(x1=None), "(x1)"), (dict(out=None), "(out)"),
                     (dict(ld_rays=7), "ld_rays (7) < n (8)"), (dict(ld=7), "ld (7) < n (8)")):
        a = dict(rays=p, ld_rays=8, x1=p, n=8, out=p, ld=8, status=None, stream=None)
        a.update(kw)
        assert L.airice_icefirst_select_launch(*a.values()) == -1
        assert word in L.airice_last_error().decode(), kw
        del a["stream"]
        assert L.airice_icefirst_select_host(*a.values()) == -1
        assert word in L.airice_last_error().decode(), kw
    assert L.airice_icefirst_select_launch(None, 0, None, 0, None, 0, None, None) == 0
    assert [_lib.launch_count(k) for k in KERNELS] == before


def test_first_arrival_rule_against_numpy(pairs):
    """The host route against the rule as written, applied to ice_rays_host rows of the same
    (z0, x1, z1): all eight columns bit for bit; column 6 is np.sqrt(dx*dx + dy*dy)."""
    tx, rx, triples, ray_rows, want, got, st = pairs
    dx, dy = tx[0] - rx[0], tx[1] - rx[1]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(cases.bits(got[:, cases.F_X1]),
                              cases.bits(np.sqrt(dx * dx + dy * dy)))
    assert np.array_equal(st, ray_rows[:, rays.STATUS].astype(np.int64))
    diff = np.flatnonzero((cases.bits(got) != cases.bits(want)).any(axis=1))
    assert len(diff) == 0, (diff[:5], got[diff[0]], want[diff[0]])


def test_the_cases_the_rule_turns_on(pairs):
    """No candidate gives -1000; the reflected ray is never chosen, also when it is the only ray;
    a direct ray slower than the refracted one loses; equal depths; a non-finite coordinate in any
    slot gives NaN, type 0 and status 128."""
    tx, rx, triples, ray_rows, want, got, st = pairs
    ok = (st & rays.NONFINITE) == 0
    types = got[:, cases.F_TYPE]
    assert set(np.unique(types)) == {0.0, 1.0, 3.0, 4.0}
    none = ok & ((st & (rays.D | rays.RA0 | rays.RA1)) == 0)
    assert none.sum() >= 2 and (got[none, :5] == -1000).all() and (types[none] == 0).all()
    r_only = ok & (st == rays.R)
    assert r_only.sum() >= 1, "no pair whose only ray is the reflected one"
    assert (got[r_only, :5] == -1000).all()
    # with both a direct and a refracted ray the direct one is the earlier in every solved pair
    # (Fermat): the slower direct ray is in test_the_rule_on_rows_no_geometry_gives
    both = ok & ((st & rays.D) != 0) & ((st & rays.RA0) != 0)
    assert both.sum() >= 1 and (types[both] == 1).all()
    assert (ray_rows[both, rays.TIME] < ray_rows[both, rays.TIME + 2]).all()
    two = ok & ((st & rays.RA0) != 0) & ((st & rays.RA1) != 0)
    assert two.sum() >= 1 and np.isin(types[two], (3.0, 4.0)).all()
    assert (types[two] == 4).any() or (ray_rows[two, rays.TIME + 2]
                                       <= ray_rows[two, rays.TIME + 3]).all()
    equal = ok & (triples[:, 0] == triples[:, 2])
    assert equal.sum() >= 1
    # the winner's values are its solver columns, and its time*c is the smallest of the candidates
    for i in np.flatnonzero(ok & (types > 0))[:500]:
        ray = int(types[i]) - 1
        assert got[i, cases.F_TIME] == ray_rows[i, rays.TIME + ray]
        assert got[i, cases.F_PATH] == ray_rows[i, rays.PATH + ray]
        assert got[i, cases.F_TIMEC] == ray_rows[i, rays.TIME + ray] * cases.C_LIGHT
    assert (~ok).sum() == len(rays.nonfinite_queries()) + 12  # and the six coordinates' two each
    assert np.isnan(got[~ok, :5]).all() and (types[~ok] == 0).all()
    assert (st[~ok] == rays.NONFINITE).all() and (got[~ok, cases.F_STATUS] == 128).all()


def test_the_rule_on_rows_no_geometry_gives(solver, pairs):
    """airice_icefirst_select_host over written rows: a direct ray slower than Ra0 loses to it,
    Ra1 can win, equal times keep the first candidate, a time*c that is not < 1e9 (1e9 itself, or
    NaN) never displaces candidate 0 and leaves it standing when it is candidate 0, the reflected
    ray alone -- however early -- gives -1000.  Over the solved rows it is the host route."""
    _, _, triples, ray_rows, want, got, st = pairs
    out, s8 = solver.ice_first_select_host(ray_rows.T, triples[:, 1])
    assert np.array_equal(cases.bits(out.T), cases.bits(got)) and np.array_equal(s8, st)

    def row(times, rangs, status):
        g = np.zeros(rays.FIELDS)
        g[rays.LANG:rays.LANG + 4] = (10.0, 20.0, 30.0, 40.0)
        g[rays.TIME:rays.TIME + 4] = times
        g[rays.RANG:rays.RANG + 4] = rangs
        g[rays.PATH:rays.PATH + 4] = (100.0, 200.0, 300.0, 400.0)
        g[rays.STATUS] = status
        return g

    no = -1000.0
    big = 1e9 / cases.C_LIGHT * 1.000001  # time*c is above 1e9
    rows = np.array([
        row((3e-6, 1e-6, 2e-6, 4e-6), (50, 60, 70, 80), 15),          # D slower than Ra0 -> Ra0
        row((3e-6, 1e-6, 2e-6, 1.5e-6), (50, 60, 70, 80), 15),        # Ra1 the earliest -> Ra1
        row((2e-6, 1e-6, 2e-6, 2e-6), (50, 60, 70, 80), 15),          # equal: the first stands
        row((0.0, 1e-6, 0.0, 0.0), (no, 60, no, no), 2),              # R only -> -1000
        row((big, 1e-6, big * 2, 0.0), (50, 60, 70, no), 7),          # none < 1e9: candidate 0
        row((np.nan, 1e-6, 2e-6, 0.0), (50, 60, 70, no), 7),          # NaN first, then a real one
        row((2e-6, 1e-6, np.nan, 0.0), (50, 60, 70, no), 7),          # NaN never displaces
        row((0.0, 0.0, 5e-6, 4e-6), (no, no, 70, 80), 12),            # no D: Ra1 before Ra0
    ])
    x1 = np.arange(len(rows), dtype=np.float64)
    out, s8 = solver.ice_first_select_host(rows.T, x1)
    assert np.array_equal(cases.bits(out.T), cases.bits(cases.first_rule(rows, x1)))
    assert out[cases.F_TYPE].tolist() == [3, 4, 1, 0, 1, 3, 1, 4]
    assert (out[:5, 3] == -1000).all()
    assert out[cases.F_TIME, 5] == 2e-6 and out[cases.F_TIME, 4] == big
    assert np.array_equal(s8, rows[:, rays.STATUS].astype(np.uint8))
    assert np.array_equal(out[cases.F_X1], x1)


def test_dropin_is_the_host_route_bit_for_bit(pairs):
    """DirectRayTracer through the caller program on every pair: its five values are columns 0-4
    of the host route."""
    tx, rx, _, _, _, got, _ = pairs
    rows = np.concatenate([tx, rx]).T
    words = cases.run_driver("first", rows)["T"]
    assert words.shape == (len(rows), 5)
    assert np.array_equal(words, cases.bits(got[:, :5]))


def test_other_model_and_the_callers_rows(solver):
    """Another ice model goes through the host entry (the rule over that model's rows), and the
    caller program's own pairs are this process's host route, before and after SetA/SetB/SetC."""
    rng = np.random.default_rng(7)
    tx, rx = cases.first_points(rays.drawn(64, rng), rng)
    triples = cases.first_triples(tx, rx)
    ray_rows, _ = rays.host_rows(solver, triples, model=cases.OTHER_MODEL)
    got, _ = cases.first_host_rows(solver, tx, rx, model=cases.OTHER_MODEL)
    assert rays.same_bits(got, cases.first_rule(ray_rows, triples[:, 1]))
    default, _ = cases.first_host_rows(solver, tx, rx)
    assert not rays.same_bits(got, default)
    plain = subprocess.run([cases.DRIVER], capture_output=True, text=True, check=True)
    lines = [ln.split() for ln in plain.stdout.splitlines()]
    first = {int(ln[1]): [int(w, 16) for w in ln[2:]] for ln in lines if ln[0] == "T"}
    p0 = np.array([[0.0], [0.0], [-180.0]]), np.array([[60.0], [80.0], [-100.0]])
    mine, _ = cases.first_host_rows(solver, *p0)
    assert first[0] == cases.bits(mine[0, :5]).tolist()
    other, _ = cases.first_host_rows(solver, *p0, model=cases.OTHER_MODEL)
    assert first[1000] == cases.bits(other[0, :5]).tolist() and first[1000] != first[0]
    assert np.isnan(np.array(first[6], dtype=np.uint64).view(np.float64)).all()  # the NaN pair
