"""The ice-to-air direct ray on the GPU (iceair_kernel): batch sizes across the wave and block edges
with a padded leading dimension, one launch each, bit for bit against the one-query device route,
a permuted batch, the device against the host route, the physics of device rows against mpmath,
and another ice model.  Rows: tests/iceair_cases.py."""
import numpy as np
import pytest

from tests import iceair_cases as cases
from tests.iceray_cases import same_bits

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)
SINGLES_CAP = 320  # one-query device calls in the whole bit-identity test
PAD, SENTINEL, ST_SENTINEL = 3, -777.25, 0xAB
VALUES = [cases.RANG, cases.LANG, cases.TIME, cases.LVALUE, cases.PHYS_TIME, cases.PATH]


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _solve(solver, q, pad=0, model=None):
    """One ice_to_air_device launch of the (n, 3) rows with ld = n + pad: ((10, n) values, status,
    launches of iceair_kernel); the pad must come back untouched."""
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    n = len(q)
    cols = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(3)]
    out = torch.full((cases.FIELDS, n + pad), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.full((n + pad,), ST_SENTINEL, dtype=torch.uint8, device=dev)
    with _lib.launched("iceair_kernel") as k:
        solver.ice_to_air_device(*cols, out, st, ld=n + pad, stream=torch.cuda.current_stream(),
                                 model=model)
        torch.cuda.synchronize()
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert np.all(o[:, n:] == SENTINEL) and np.all(s[n:] == ST_SENTINEL)
    return o[:, :n], s[:n], k.count


def _batch(n):
    return cases.batch(n, np.random.default_rng(2000 + n))


@pytest.fixture(scope="module")
def thousand(solver):
    q = _batch(1000)
    o, s, launches = _solve(solver, q, pad=PAD)
    for a in (q, o, s):
        a.setflags(write=False)
    return q, o, s, launches


def test_batches_and_the_one_query_device_route(solver, thousand):
    """Batches of 1 .. 1000 rows, ld = n + 3 with sentinels in the pad: one launch each, the
    status vector equal to column 5, and -- on at most 320 picked rows in all -- the bits of the
    host entry in AIRICE_SCALAR_DEVICE mode with n = 1, which runs the same kernel."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    n_head = len(cases.head_rows())
    small = sum(n for n in BATCHES if n <= 65)
    per_large = (SINGLES_CAP - small) // sum(1 for n in BATCHES if n > 65)
    singles = 0
    for n in BATCHES:
        q, o, s, launches = thousand if n == 1000 else (_batch(n), *_solve(solver, _batch(n), PAD))
        assert launches == 1, n
        assert np.array_equal(s, o[cases.STATUS].astype(np.uint8)), n
        if n <= 65:
            pick = np.arange(n)
        else:  # the head rows, the wave and block edges, the last row, then draws
            edges = [i for i in (63, 64, 255, 256) if i < n] + [n - 1]
            pick = list(dict.fromkeys(list(range(n_head)) + edges))
            rest = np.setdiff1d(np.arange(n), pick)
            extra = np.random.default_rng(n).choice(rest, per_large - len(pick), replace=False)
            pick = np.array(pick + extra.tolist())
        with scalar_mode(_lib.SCALAR_DEVICE), _lib.launched("iceair_kernel") as k:
            ones = [solver.ice_to_air_host(*q[i]) for i in pick]
        assert k.count == len(pick), n
        singles += len(pick)
        assert same_bits(o[:, pick].T, np.array([v[:, 0] for v, _ in ones])), n
        assert np.array_equal(s[pick], np.array([b[0] for _, b in ones])), n
    assert singles <= SINGLES_CAP, singles
    # the head rows on the device: every finite one accepted, every non-finite one flagged
    q, o, s, _ = thousand
    n_fin = len(cases.FINITE_HEAD)
    assert (s[:n_fin] == cases.ACCEPTED).all()
    assert (s[n_fin:n_head] == cases.NONFINITE).all()
    assert np.isnan(o[[0, 1, 2, 3, 4, 8, 9], n_fin:n_head]).all()
    assert (o[[cases.EVALS, cases.ITERS], n_fin:n_head] == 0).all()
    assert (s[n_head:] == cases.ACCEPTED).all() and (o[cases.ITERS] <= 100).all()
    # the kernel timer sees the launch
    _lib.kernel_time("iceair_kernel")  # reset
    _lib.kernel_timing(True)
    try:
        _solve(solver, q[:64])
    finally:
        _lib.kernel_timing(False)
    ms, timed = _lib.kernel_time("iceair_kernel")
    assert timed == 1 and ms > 0


def test_a_permuted_batch_gives_permuted_results(solver, thousand):
    q, o, s, _ = thousand
    perm = np.random.default_rng(77).permutation(len(q))
    po, ps, launches = _solve(solver, np.ascontiguousarray(q[perm]), pad=PAD)
    assert launches == 1
    assert same_bits(po, o[:, perm]) and np.array_equal(ps, s[perm])


def test_device_against_the_host_route(solver):
    """4,096 rows.  The status byte is equal on every row.  On rows whose evaluation and iteration
    counts are equal, every value is within 1e-9 relative (checkzero, a residual and not a value
    with a scale of its own, within 1e-9 of x1 + L |df/dL|).  Rows whose counts differ -- ocml's and the host libm's log and tan
    straddle the 1e-6 stop -- are at most 5 % of the batch (a cap); on them the device's and the
    host's values each pass every physics bound on their own.
    Measured on an MI355X: none of the 4,087 finite rows differs in its counts (0.00 %); the worst
    value is 8.8e-13 relative and the worst checkzero 1.3e-14 of its scale."""
    q = cases.batch(4096, np.random.default_rng(4096))
    o, s, launches = _solve(solver, q)
    assert launches == 1
    dev = o.T
    host, hst = cases.host_rows(solver, q)
    assert np.array_equal(s.astype(np.int64), hst)
    fin = hst == cases.ACCEPTED
    same = fin & (dev[:, cases.EVALS] == host[:, cases.EVALS]) & \
        (dev[:, cases.ITERS] == host[:, cases.ITERS])
    a, b = dev[same][:, VALUES], host[same][:, VALUES]
    err = np.abs(a - b) / np.abs(b)
    err[a == b] = 0.0
    # checkzero is f(L) = reach(L) - x1, not a quantity with a scale of its own: 1e-9 relative in
    # L moves it by 1e-9 L |df/dL|, and df/dL <= h / (1 - L^2)^1.5 (the air leg) + 2.5 |z0| (the
    # ice leg: n^2 / (n^2 - L^2)^1.5 <= 2.5 for L < 1 < 1.35 <= n); 1e-9 of x1 for its own rounding
    L = host[same, cases.LVALUE]
    slope = q[same, 2] / (1 - L * L) ** 1.5 + 2.5 * np.abs(q[same, 0])
    cz = np.abs(dev[same, cases.CHECKZERO] - host[same, cases.CHECKZERO]) / (q[same, 1] + L * slope)
    differ = np.flatnonzero(fin & ~same)
    print(f"[iceair device vs host] {len(q)} rows, {int(same.sum())} with equal counts (worst "
          f"value {err.max():.2e} relative, worst checkzero {cz.max():.2e} of its scale), {len(differ)} "
          f"with different counts ({100.0 * len(differ) / len(q):.2f} %)")
    assert np.isfinite(a).all() and np.isfinite(b).all()
    over = np.argwhere(err > 1e-9)
    assert len(over) == 0, [(q[same][i], VALUES[c], err[i, c]) for i, c in over[:5]]
    assert (cz <= 1e-9).all()
    assert len(differ) <= len(q) * 5 // 100
    for name, vals in (("device", dev), ("host", host)):
        bad = cases.physics_failures(cases.physics_errors(q[differ], vals[differ], hst[differ]))
        assert not bad, (name, bad[:5], q[differ][[r[0] for r in bad[:5]]])


def test_physics_of_device_rows(solver):
    """The physics check of the CPU layer on 256 device rows: the head rows, then draws."""
    q = cases.batch(256, np.random.default_rng(256))
    o, s, _ = _solve(solver, q)
    rows = cases.physics_errors(q, o.T, s.astype(np.int64))
    r = np.array(rows)
    print(f"[iceair device physics] {len(r)} rows: worst reach {(r[:, 1] / r[:, 2]).max():.3g} of "
          f"its bound, time {(r[:, 3] / r[:, 4]).max():.3g}, path {(r[:, 5] / r[:, 6]).max():.3g}; "
          f"|sin(col 0) - L| {r[:, 7].max():.3g}, col 2 - col 8 {r[:, 8].max():.3g}")
    assert len(rows) == 256 - len(cases.nonfinite_rows())
    bad = cases.physics_failures(rows)
    assert not bad, (bad[:5], q[[b[0] for b in bad[:5]]])


def test_another_ice_model(solver):
    """{1.775, -0.5, 0.02} through the device entry: bit for bit the one-query device route with
    that model, within 1e-9 of the host route's rows with equal counts, and not the default's."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    q = cases.batch(65, np.random.default_rng(65))
    o, s, launches = _solve(solver, q, model=cases.OTHER_MODEL)
    assert launches == 1
    with scalar_mode(_lib.SCALAR_DEVICE):
        ones = [solver.ice_to_air_host(*row, model=cases.OTHER_MODEL) for row in q]
    assert same_bits(o.T, np.array([v[:, 0] for v, _ in ones]))
    host, hst = cases.host_rows(solver, q, model=cases.OTHER_MODEL)
    assert np.array_equal(s.astype(np.int64), hst)
    same = (hst == cases.ACCEPTED) & (o[cases.EVALS] == host[:, cases.EVALS])
    assert same.sum() >= 50
    a, b = o.T[same][:, VALUES], host[same][:, VALUES]
    assert (np.abs(a - b) <= 1e-9 * np.abs(b)).all()
    default, _, _ = _solve(solver, q)
    assert not same_bits(default[cases.LVALUE], o[cases.LVALUE])
