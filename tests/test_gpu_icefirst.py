"""The first-arrival tracer on the GPU (icefirst_geom_kernel, iceray_kernel,
icefirst_select_kernel): batch sizes across the wave and block edges, exactly one launch of each
per call and no device allocation, all eight columns bit for bit the numpy rule over
ice_rays_device rows of the same (z0, x1, z1), the one-pair device route, a permuted batch, cross
pairing against the expanded elementwise call, the choice alone over written rows, and another ice
model.  Points and the rule: tests/iceair_cases.py."""
import numpy as np
import pytest

from tests import iceair_cases as cases
from tests import iceray_cases as rays

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)
KERNELS = ("icefirst_geom_kernel", "iceray_kernel", "icefirst_select_kernel")
PAD, SENTINEL, ST_SENTINEL = 3, -777.25, 0xAB


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _points(n):
    """The head points, then drawn pairs with random origins and azimuths: (tx, rx), (3, n)."""
    rng = np.random.default_rng(3000 + n)
    htx, hrx = cases.first_head_points()
    if n <= htx.shape[1]:
        return np.ascontiguousarray(htx[:, :n]), np.ascontiguousarray(hrx[:, :n])
    dtx, drx = cases.first_points(rays.drawn(n - htx.shape[1], rng), rng)
    return (np.ascontiguousarray(np.concatenate([htx, dtx], axis=1)),
            np.ascontiguousarray(np.concatenate([hrx, drx], axis=1)))


def _trace(solver, tx, rx, pairing="elementwise", pad=0, model=None):
    """One ice_first_arrivals_device call with a caller's work buffer and ld = pairs + pad:
    ((8, pairs) values, status, launches of the three kernels, bytes torch allocated during the
    call); the pad must come back untouched."""
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    n = tx.shape[1] * rx.shape[1] if pairing == "cross" else tx.shape[1]
    t, r = torch.from_numpy(tx).to(dev), torch.from_numpy(rx).to(dev)
    out = torch.full((cases.FIRST_FIELDS, n + pad), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.full((n + pad,), ST_SENTINEL, dtype=torch.uint8, device=dev)
    work = torch.empty(solver.ice_first_arrivals_work_bytes(n), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    before = [_lib.launch_count(k) for k in KERNELS]
    allocated = torch.cuda.memory_allocated(dev)
    solver.ice_first_arrivals_device(t, r, out, work=work, pairing=pairing, status=st, ld=n + pad,
                                     stream=torch.cuda.current_stream(), model=model)
    allocated = torch.cuda.memory_allocated(dev) - allocated
    torch.cuda.synchronize()
    launches = [_lib.launch_count(k) - b for k, b in zip(KERNELS, before)]
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert np.all(o[:, n:] == SENTINEL) and np.all(s[n:] == ST_SENTINEL)
    return o[:, :n], s[:n], launches, allocated


def _rule_on_device_rows(solver, triples, model=None):
    """The numpy rule over ice_rays_device rows of the triples: (n, 8)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(triples)
    cols = [torch.from_numpy(np.ascontiguousarray(triples[:, k])).to(dev) for k in range(3)]
    out = torch.empty((rays.FIELDS, n), dtype=torch.float64, device=dev)
    solver.ice_rays_device(*cols, out, stream=torch.cuda.current_stream(), model=model)
    torch.cuda.synchronize()
    return cases.first_rule(out.cpu().numpy().T, triples[:, 1])


@pytest.fixture(scope="module")
def thousand(solver):
    tx, rx = _points(1000)
    o, s, launches, allocated = _trace(solver, tx, rx, pad=PAD)
    for a in (tx, rx, o, s):
        a.setflags(write=False)
    return tx, rx, o, s, launches, allocated


def test_batches_against_the_rule_over_device_rows(solver, thousand):
    """1 .. 1000 pairs, ld = pairs + 3: exactly one geometry, one iceray_kernel and one select
    launch per call and nothing allocated; all eight columns bit for bit the numpy rule over
    ice_rays_device rows (the select kernel adds no arithmetic but time*c); column 6 is
    np.sqrt(dx*dx + dy*dy); the status vector is column 7."""
    for n in BATCHES:
        tx, rx = _points(n)
        o, s, launches, allocated = thousand[2:] if n == 1000 else _trace(solver, tx, rx, pad=PAD)
        assert launches == [1, 1, 1] and allocated == 0, (n, launches, allocated)
        triples = cases.first_triples(tx, rx)
        off = np.flatnonzero(cases.bits(o[cases.F_X1]) != cases.bits(triples[:, 1]))
        assert len(off) == 0, (n, off[:5], o[cases.F_X1, off[:5]], triples[off[:5], 1])
        assert np.array_equal(s, o[cases.F_STATUS].astype(np.uint8)), n
        want = _rule_on_device_rows(solver, triples)
        diff = np.flatnonzero((cases.bits(o.T) != cases.bits(want)).any(axis=1))
        assert len(diff) == 0, (n, diff[:5], o.T[diff[0]], want[diff[0]])
    o, s = thousand[2], thousand[3]
    assert set(np.unique(o[cases.F_TYPE])) == {0.0, 1.0, 3.0, 4.0}
    bad = (s & rays.NONFINITE) != 0
    assert bad.sum() == len(rays.nonfinite_queries()) + 12
    assert np.isnan(o[:5, bad]).all() and (o[cases.F_TYPE, bad] == 0).all()
    r_only = s == rays.R
    assert r_only.sum() >= 2 and (o[:5, r_only] == -1000).all()


def test_the_one_pair_device_route_and_a_permuted_batch(solver, thousand):
    """On 96 picked pairs the batch is bit for bit the host entry in AIRICE_SCALAR_DEVICE mode with
    one pair, which runs the same three kernels; a permuted batch gives permuted results."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    tx, rx, o, s, _, _ = thousand
    n_head = cases.first_head_points()[0].shape[1]
    pick = list(range(n_head)) + [63, 64, 255, 256, 999]
    pick += np.random.default_rng(5).choice(np.arange(n_head, 999), 96 - len(pick),
                                            replace=False).tolist()
    before = [_lib.launch_count(k) for k in KERNELS]
    with scalar_mode(_lib.SCALAR_DEVICE):
        ones = [solver.ice_first_arrivals_host(tx[:, i:i + 1], rx[:, i:i + 1]) for i in pick]
    assert [_lib.launch_count(k) - b for k, b in zip(KERNELS, before)] == [len(pick)] * 3
    assert np.array_equal(cases.bits(o[:, pick].T), cases.bits(np.array([v[:, 0] for v, _ in ones])))
    assert np.array_equal(s[pick], np.array([b[0] for _, b in ones]))
    perm = np.random.default_rng(78).permutation(tx.shape[1])
    po, ps, launches, _ = _trace(solver, np.ascontiguousarray(tx[:, perm]),
                                 np.ascontiguousarray(rx[:, perm]), pad=PAD)
    assert launches == [1, 1, 1]
    assert np.array_equal(cases.bits(po), cases.bits(o[:, perm])) and np.array_equal(ps, s[perm])


@pytest.mark.parametrize("n_tx,n_rx", [(3, 67), (5, 256)])
def test_cross_pairing_is_the_expanded_elementwise_call(solver, n_tx, n_rx):
    """Pair t * n_rx + r = (emitter t, antenna r): bit for bit the elementwise call on the
    expanded pairs, in three launches; the host entry's cross route gives the same."""
    rng = np.random.default_rng(n_tx * 1000 + n_rx)
    tx = np.stack([20 * rng.random(n_tx), 20 * rng.random(n_tx), -400 + 300 * rng.random(n_tx)])
    rx = np.stack([600 * rng.random(n_rx) - 300, 600 * rng.random(n_rx) - 300,
                   -200 * rng.random(n_rx) - 1])
    tx[:, 0] = (1.0, np.nan, -150.0)  # an emitter row of NaN pairs
    o, s, launches, allocated = _trace(solver, tx, rx, pairing="cross", pad=PAD)
    assert launches == [1, 1, 1] and allocated == 0
    etx, erx = np.repeat(tx, n_rx, axis=1), np.tile(rx, (1, n_tx))
    eo, es, _, _ = _trace(solver, np.ascontiguousarray(etx), np.ascontiguousarray(erx))
    assert np.array_equal(cases.bits(o), cases.bits(eo)) and np.array_equal(s, es)
    assert (s[:n_rx] == rays.NONFINITE).all() and (s[n_rx:] != rays.NONFINITE).all()
    ho, hs = solver.ice_first_arrivals_host(tx, rx, pairing="cross")
    assert np.array_equal(cases.bits(ho), cases.bits(o)) and np.array_equal(hs, s)


def test_the_choice_alone_over_written_rows(solver, thousand):
    """airice_icefirst_select_launch: one launch of the select kernel over caller-held rows --
    the rows no geometry gives (a direct ray slower than Ra0, a time*c not below 1e9, NaN times,
    the reflected ray alone) -- bit for bit the numpy rule and the host entry, with padded
    strides."""
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    no, big = -1000.0, 1e9 / cases.C_LIGHT * 1.000001
    cand = [((3e-6, 1e-6, 2e-6, 4e-6), (50, 60, 70, 80), 15),
            ((3e-6, 1e-6, 2e-6, 1.5e-6), (50, 60, 70, 80), 15),
            ((2e-6, 1e-6, 2e-6, 2e-6), (50, 60, 70, 80), 15),
            ((0.0, 1e-6, 0.0, 0.0), (no, 60, no, no), 2),
            ((big, 1e-6, big * 2, 0.0), (50, 60, 70, no), 7),
            ((np.nan, 1e-6, 2e-6, 0.0), (50, 60, 70, no), 7),
            ((2e-6, 1e-6, np.nan, 0.0), (50, 60, 70, no), 7),
            ((0.0, 0.0, 5e-6, 4e-6), (no, no, 70, 80), 12),
            ((np.nan,) * 4, (np.nan,) * 4, 128)]
    n = 300  # more than one block
    rows = np.zeros((n, rays.FIELDS))
    for i in range(n):
        times, rangs, status = cand[i % len(cand)]
        rows[i, rays.LANG:rays.LANG + 4] = (10.0 + i, 20.0, 30.0 + i, 40.0)
        rows[i, rays.TIME:rays.TIME + 4] = times
        rows[i, rays.RANG:rays.RANG + 4] = rangs
        rows[i, rays.PATH:rays.PATH + 4] = (100.0, 200.0, 300.0 + i, 400.0)
        rows[i, rays.STATUS] = status
    x1 = np.arange(n, dtype=np.float64)
    want = cases.first_rule(rows, x1)
    ld_rays, ld = n + 5, n + PAD
    d_rows = torch.full((rays.FIELDS, ld_rays), SENTINEL, dtype=torch.float64, device=dev)
    d_rows[:, :n] = torch.from_numpy(np.ascontiguousarray(rows.T)).to(dev)
    out = torch.full((cases.FIRST_FIELDS, ld), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.full((ld,), ST_SENTINEL, dtype=torch.uint8, device=dev)
    before = [_lib.launch_count(k) for k in KERNELS]
    solver.ice_first_select_device(d_rows, torch.from_numpy(x1).to(dev), out, st, ld=ld,
                                   ld_rays=ld_rays, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert [_lib.launch_count(k) - b for k, b in zip(KERNELS, before)] == [0, 0, 1]
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert np.all(o[:, n:] == SENTINEL) and np.all(s[n:] == ST_SENTINEL)
    assert np.array_equal(cases.bits(o[:, :n].T), cases.bits(want))
    assert o[cases.F_TYPE, :9].tolist() == [3, 4, 1, 0, 1, 3, 1, 4, 0]
    ho, hs = solver.ice_first_select_host(rows.T, x1)
    assert np.array_equal(cases.bits(ho), cases.bits(o[:, :n])) and np.array_equal(hs, s[:n])


def test_another_ice_model(solver):
    """{1.775, -0.5, 0.02} through the device entry: the rule over that model's device rows, and
    not the default model's arrivals."""
    tx, rx = _points(257)
    o, s, launches, _ = _trace(solver, tx, rx, model=cases.OTHER_MODEL)
    assert launches == [1, 1, 1]
    want = _rule_on_device_rows(solver, cases.first_triples(tx, rx), model=cases.OTHER_MODEL)
    assert np.array_equal(cases.bits(o.T), cases.bits(want))
    default, _, _, _ = _trace(solver, tx, rx)
    assert not np.array_equal(cases.bits(default), cases.bits(o))
