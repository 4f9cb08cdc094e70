"""The two-ray solutions on the GPU (icesol_kernel): batch sizes across the wave and block edges
with a padded leading dimension, bit identity across batches and orders, hand-made solver rows
that reach every block of the choice, the device against the host's pieces on the same
device-made solver rows, the attenuation of device rows against mpmath, and the host wrapper.
Rows: tests/iceray_cases.py; independent checks: tests/icesol_cases.py."""
import math

import numpy as np
import pytest

from tests import iceray_cases as rays
from tests import icesol_cases as cases

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)
PAD, SENTINEL, ST_SENTINEL = 3, -777.25, 0xAB


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _to_device(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(torch.device("cuda:0"))


def _solver_rows(solver, q):
    """iceray_kernel's (32, n) device tensor for the (n, 3) rows."""
    import torch
    cols = [_to_device(q[:, k]) for k in range(3)]
    out = torch.empty((rays.FIELDS, len(q)), dtype=torch.float64, device=cols[0].device)
    solver.ice_rays_device(*cols, out, stream=torch.cuda.current_stream())
    return out


def _solutions(solver, q, ray_rows, lower_rows=None, pad=0, a0=1.0, frequency=0.1):
    """One ice_solutions_device launch over (32, n) device tensors of solver rows, ld = n + pad:
    ((n, 18) values, status, launches of icesol_kernel); the pad must come back untouched."""
    import torch
    from airiceraytracing_amd import _lib
    n = len(q)
    cols = [_to_device(q[:, k]) for k in range(3)]
    dev = cols[0].device
    out = torch.full((cases.FIELDS, n + pad), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.full((n + pad,), ST_SENTINEL, dtype=torch.uint8, device=dev)
    with _lib.launched("icesol_kernel") as k, _lib.launched("iceray_kernel") as r:
        solver.ice_solutions_device(*cols, ray_rows, out, st, a0=a0, frequency=frequency,
                                    rays_lower=lower_rows, ld=n + pad,
                                    stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
    assert r.count == 0
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert np.all(o[:, n:] == SENTINEL) and np.all(s[n:] == ST_SENTINEL)
    return o[:, :n].T.copy(), s[:n].astype(np.int64), k.count


def _lower(q):
    return q - np.array([0.0, 0.0, 0.01])


def _solve(solver, q, pad=0, **kw):
    return _solutions(solver, q, _solver_rows(solver, q), _solver_rows(solver, _lower(q)), pad, **kw)


@pytest.fixture(scope="module")
def thousand(solver):
    q = rays.batch(1000, np.random.default_rng(2000))
    o, s, launches = _solve(solver, q, pad=PAD)
    for a in (q, o, s):
        a.setflags(write=False)
    return q, o, s, launches


def test_batches_are_one_launch_and_the_same_bits(solver, thousand):
    """Batches of the first 1 .. 1000 rows, ld = n + 3 with sentinels in the pad: one launch of
    icesol_kernel each, the status consistent with IgnoreCh, and every batch -- and the 1000 rows
    reversed -- bit for bit the rows of the 1000-row batch."""
    q, o, s, launches = thousand
    assert launches == 1
    for n in BATCHES[:-1]:
        on, sn, launches = _solve(solver, q[:n], pad=PAD)
        assert launches == 1, n
        assert rays.same_bits(on, o[:n]) and np.array_equal(sn, s[:n]), n
    ro, rs, launches = _solve(solver, np.ascontiguousarray(q[::-1]), pad=PAD)
    assert launches == 1
    assert rays.same_bits(ro[::-1], o) and np.array_equal(rs[::-1], s)
    finite = (s & cases.NONFINITE) == 0
    assert np.array_equal((s & 3)[finite], (o[:, cases.IGNORE] + 2 * o[:, cases.IGNORE + 1])[finite])
    assert (s[~finite] == cases.NONFINITE).all() and (~finite).sum() == len(rays.nonfinite_queries())
    assert (o[~finite][:, [8, 9, 14, 15]] == 0).all()
    assert np.isnan(o[~finite][:, [0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 16, 17]]).all()
    # a factor is 0.0 where its condition is not met (but for the closing rule), and without the
    # lower receivers' rows every factor is 0.0 and the rest is unchanged
    unset0 = finite & ((s & cases.FOCUS0) == 0) & (q[:, 0] != q[:, 2])
    assert (o[unset0, cases.FOCUS] == 0).all() and (o[finite & ((s & cases.FOCUS1) == 0), 17] == 0).all()
    plain, ps, _ = _solutions(solver, q, _solver_rows(solver, q), None, pad=PAD)
    assert rays.same_bits(plain[:, :cases.FOCUS], o[:, :cases.FOCUS])
    assert (plain[finite][:, cases.FOCUS:] == 0).all() and np.array_equal(ps, s & ~24)


def _synthetic_rows():
    """Hand-made solver rows: every subset of (D, R, Ra0, Ra1) present, in both orders of arrival
    -- D with Ra1 and R with Ra1 among them, which the solver never gives --, a NaN receive angle,
    the straight-line rule with Distance 0 and > 0 (and equal depths that do not meet it), and a
    non-finite row."""
    q, rows = [], []
    for present in range(16):
        for order in (1.0, -1.0):
            r = np.zeros(rays.FIELDS)
            for ray in range(4):
                ok = bool(present & (1 << ray))
                r[rays.LANG + ray] = 40.0 + 7 * ray
                r[rays.TIME + ray] = 1e-6 * (3 + order * (ray - 1.5))
                r[rays.RANG + ray] = (50.0 + 11 * ray) if ok else -1000.0
                r[rays.LVALUE + ray] = (1.30, 1.32, 1.50, 1.52)[ray]
                r[rays.PATH + ray] = 300.0 + 13 * ray
            r[rays.INCIDENCE], r[rays.ZMAX], r[rays.ZMAX + 1] = 77.0, 32.0, 38.0
            r[rays.STATUS] = present
            q.append((-150.0, 250.0, -100.0))
            rows.append(r)
    nan_rang = rows[6].copy()  # D | R with a NaN receive angle: NaN != -1000, so the ray counts
    nan_rang[rays.RANG] = np.nan
    q.append((-150.0, 250.0, -100.0))
    rows.append(nan_rang)
    for x1, time0, path0 in ((0.0, 0.0, 0.0), (0.4, 0.0, 0.0), (0.4, 0.0, 1.0), (0.4, 1e-9, 0.0)):
        r = rows[6].copy()  # D | R
        r[rays.TIME], r[rays.PATH] = time0, path0
        q.append((-120.0, x1, -120.0))
        rows.append(r)
    r = rows[0].copy()  # no ray at all, at equal depths: the rule fires on the initial slot
    r[rays.TIME], r[rays.PATH] = 0.0, 0.0
    q.append((-120.0, 0.4, -120.0))
    rows.append(r)
    r = np.full(rays.FIELDS, np.nan)
    r[rays.STATUS], r[rays.EVALS], r[rays.ITERS] = 128.0, 0.0, 0.0
    q.append((np.nan, 250.0, -100.0))
    rows.append(r)
    return np.array(q), np.array(rows)


def test_hand_made_solver_rows_reach_every_block(solver):
    """icesol_kernel on hand-made 32-column blocks against the Python restatement: exact on every
    choice column and the status.  The one value of those columns that is computed and not copied,
    the straight line's time x1 / (c / n(z0)), depends on the device's exp (within 1 ulp of the
    host's, so the quotient within 2 ulp); everything else bit for bit."""
    q, rows = _synthetic_rows()
    want, want_st, src = cases.choose_rows(q, rows)
    got, st, launches = _solutions(solver, q, _to_device(rows.T), None, pad=PAD, a0=0.7,
                                   frequency=0.5)
    assert launches == 1
    assert np.array_equal(st, want_st), (st, want_st)
    straight = np.flatnonzero(want_st & cases.STRAIGHT)
    assert len(straight) == 3 and {q[i, 1] for i in straight} == {0.0, 0.4}
    for i in straight:
        assert cases.ulps(got[i, cases.TIME], want[i, cases.TIME]) <= 2, (i, got[i, 0], want[i, 0])
        got[i, cases.TIME] = want[i, cases.TIME]
    bad = [i for i in range(len(q)) if not cases.same_choice(got[i:i + 1], want[i:i + 1])]
    assert not bad, (bad, got[bad[:1]], want[bad[:1]])
    # every pair of types the seven blocks can leave, in both orders
    pairs = {(int(a), int(b)) for a, b in got[:32, cases.TYPE:cases.TYPE + 2]}
    assert {(1, 2), (2, 1), (1, 3), (3, 1), (3, 2), (2, 3), (1, 4), (4, 1), (4, 2), (2, 4),
            (3, 4), (4, 3)} <= pairs, pairs
    # the attenuation of each slot is that of the ray it holds, by the drop-in on the host
    for i in range(len(q) - 1):
        for k in range(2):
            if src[i][k] is None:
                assert got[i, cases.ATT + k] == 0.0, (i, k)
                continue
            ray = src[i][k]
            I = cases.total_attenuation(ray + 1, 0.7, 0.5, q[i, 0], q[i, 2], rows[i, rays.LVALUE + ray])
            assert abs(got[i, cases.ATT + k] - (1 - I)) <= 1e-9 * I, (i, k, got[i, cases.ATT + k], I)
    assert (got[:, cases.FOCUS:][:-1] == 0).all()


def test_device_against_the_host_on_the_same_solver_rows(solver):
    """4,096 rows, the solver rows made on the device and read back: the choice columns and the
    status equal the restatement bit for bit; the attenuation is within 1e-9 I of the drop-in's
    GetTotalAttenuation* on the host at the device row's L, with equal NaN positions; the focusing
    factors are within 1e-9 relative of the formula on the chosen values.  No row is excluded.
    Measured on an MI355X: 6,944 attenuations, the worst 5.7e-15 I from the host's; the worst
    focusing factor 2.4e-16 relative from the formula (87 of them not bit-equal)."""
    a0, f = 0.9, 0.5
    q = rays.batch(4096, np.random.default_rng(4097))
    at_dev, lower_dev = _solver_rows(solver, q), _solver_rows(solver, _lower(q))
    got, st, launches = _solutions(solver, q, at_dev, lower_dev, a0=a0, frequency=f)
    assert launches == 1
    at_rows, lower_rows = at_dev.cpu().numpy().T, lower_dev.cpu().numpy().T
    want, want_st, src = cases.choose_rows(q, at_rows)
    low, _, _ = cases.choose_rows(_lower(q), lower_rows)
    assert np.array_equal(st & ~24, want_st), np.flatnonzero((st & ~24) != want_st)[:5]
    bad = [i for i in range(len(q)) if not cases.same_choice(got[i:i + 1], want[i:i + 1])]
    assert not bad, (bad[:5], q[bad[:5]])
    worst_att = worst_foc = 0.0
    n_att = n_foc = 0
    for i, (z0, x1, z1) in enumerate(q):
        if st[i] & cases.NONFINITE:
            continue
        for k in range(2):
            att = got[i, cases.ATT + k]
            if src[i][k] is None:
                assert att == 0.0, (i, k)
                continue
            I = cases.total_attenuation(src[i][k] + 1, a0, f, z0, z1,
                                        at_rows[i, rays.LVALUE + src[i][k]])
            assert math.isnan(att) == math.isnan(I), (i, q[i], k, att, I)
            if not math.isnan(I):
                n_att += 1
                worst_att = max(worst_att, abs(att - (1 - I)) / I if I > 0 else abs(att - 1))
        ff, bits = cases.focusing(z0, z1, got[i], low[i])
        assert st[i] & 24 == bits, (i, q[i], st[i], bits)
        for k in range(2):
            a, b = got[i, cases.FOCUS + k], ff[k]
            assert math.isnan(a) == math.isnan(b), (i, q[i], k, a, b)
            if not math.isnan(b) and a != b:
                n_foc += 1
                worst_foc = max(worst_foc, abs(a - b) / abs(b))
    print(f"[icesol device vs host] {len(q)} rows: {n_att} attenuations, worst {worst_att:.2e} I; "
          f"worst focusing factor {worst_foc:.2e} relative ({n_foc} not equal)")
    assert n_att > 4096 and worst_att <= 1e-9 and worst_foc <= 1e-9


def test_attenuation_of_device_rows_against_mpmath(solver):
    """64 device rows (the class rows, then draws), each at one of 0.1, 0.5 and 2.0 GHz in turn:
    |Att - (1 - I_mp)| <= 1e-9 I_mp + 1e-15, as in the CPU layer."""
    head = rays.class_queries()
    q = np.concatenate([head, rays.drawn(64 - len(head), np.random.default_rng(64))])
    at_dev = _solver_rows(solver, q)
    at_rows = at_dev.cpu().numpy().T
    _, _, src = cases.choose_rows(q, at_rows)
    worst, n = 0.0, 0
    for turn, f in enumerate(cases.FREQUENCIES):
        got, _, _ = _solutions(solver, q, at_dev, None, frequency=f)
        for i in range(turn, len(q), len(cases.FREQUENCIES)):
            z0, x1, z1 = q[i]
            for k in range(2):
                if src[i][k] is None:
                    continue
                ray = src[i][k]
                I, err = cases.attenuation_mp(ray + 1, f, at_rows[i, rays.LVALUE + ray], z0, z1)
                bound = cases.attenuation_bound(I)
                assert err <= 0.01 * bound
                ratio = abs(got[i, cases.ATT + k] - (1 - I)) / bound
                assert ratio <= 1.0, (q[i], f, ray, got[i, cases.ATT + k], I)
                worst, n = max(worst, ratio), n + 1
    print(f"[icesol device attenuation] {n} rays of 64 rows: worst {worst:.3e} of the bound")
    assert n > 64


def test_host_wrapper_composes_the_device_calls(solver, thousand):
    """ice_solutions_host for n = 1000 with focusing: iceray_kernel twice, icesol_kernel once, the
    bits of the composed device calls; the kernel timer sees the launch."""
    from airiceraytracing_amd import _lib
    q, o, s, _ = thousand
    _lib.kernel_time("icesol_kernel")  # reset
    _lib.kernel_timing(True)
    try:
        with _lib.launched("icesol_kernel") as k, _lib.launched("iceray_kernel") as r:
            ho, hs = solver.ice_solutions_host(q[:, 0], q[:, 1], q[:, 2], focusing=True)
    finally:
        _lib.kernel_timing(False)
    assert (r.count, k.count) == (2, 1)
    ms, timed = _lib.kernel_time("icesol_kernel")
    assert timed == 1 and ms > 0
    assert rays.same_bits(ho.T, o) and np.array_equal(hs.astype(np.int64), s)
    with _lib.launched("icesol_kernel") as k, _lib.launched("iceray_kernel") as r:
        po, ps = solver.ice_solutions_host(q[:, 0], q[:, 1], q[:, 2], a0=0.5, frequency=2.0)
    assert (r.count, k.count) == (1, 1)
    finite = (s & cases.NONFINITE) == 0
    assert rays.same_bits(po[:12], ho[:12]) and (po[16:, finite] == 0).all()
    assert np.array_equal(ps.astype(np.int64), s & ~24)
    # one pair through the one-query slot runs the same kernels
    from airiceraytracing_amd.solver import scalar_mode
    with scalar_mode(_lib.SCALAR_DEVICE), _lib.launched("icesol_kernel") as k:
        one, st1 = solver.ice_solutions_host(*q[1], focusing=True)
    assert k.count == 1 and rays.same_bits(one[:, 0], o[1]) and st1[0] == s[1]
