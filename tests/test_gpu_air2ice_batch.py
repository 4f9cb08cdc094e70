"""The batched Brent point-to-point solve on the GPU (air2ice_kernel): bit for bit against the
one-query device route (rtf_kernel's rtf_air2ice, the same translation unit and flags), against
the oracle, order independence, the composition with the batched path sampler, and air-to-air
pairs.  Queries: tests/air2ice_cases.py."""
import numpy as np
import pytest

from tests import air2ice_cases as cases

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)
SINGLES_CAP = 320  # one-query device calls in the whole bit-identity test
PAD, SENTINEL, ST_SENTINEL = 3, -777.25, 0xAB


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _solve(solver, q, pad=0):
    """One air2ice_device launch of the (n, 4) queries with ld = n + pad: ((16, n) values, status,
    launches of air2ice_kernel); the pad must come back untouched."""
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    n = len(q)
    cols = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(4)]
    out = torch.full((cases.FIELDS, n + pad), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.full((n + pad,), ST_SENTINEL, dtype=torch.uint8, device=dev)
    with _lib.launched("air2ice_kernel") as k:
        solver.air2ice_device(*cols, out, st, ld=n + pad, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert np.all(o[:, n:] == SENTINEL) and np.all(s[n:] == ST_SENTINEL)
    return o[:, :n], s[:n], k.count


def _batch(n):
    """n queries: the class rows, the non-finite rows, then A-D draws."""
    rng = np.random.default_rng(1000 + n)
    head = np.concatenate([cases.class_queries(), cases.nonfinite_queries()])
    if n <= len(head):
        return head[:n]
    return np.concatenate([head, cases.mixed(n - len(head), rng)])


@pytest.fixture(scope="module")
def thousand(solver):
    q = _batch(1000)
    o, s, launches = _solve(solver, q, pad=PAD)
    for a in (q, o, s):
        a.setflags(write=False)
    return q, o, s, launches


def test_batch_is_bitwise_the_one_query_device_route(solver, thousand):
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    n_head = len(cases.CLASS_ROWS) + len(cases.nonfinite_queries())
    small = sum(n for n in BATCHES if n <= 65)
    per_large = (SINGLES_CAP - small) // sum(1 for n in BATCHES if n > 65)
    singles = 0
    for n in BATCHES:
        q, o, s, launches = thousand if n == 1000 else (_batch(n), *_solve(solver, _batch(n), PAD))
        assert launches == 1, n
        assert np.array_equal(s, o[cases.STATUS].astype(np.uint8)), n
        if n <= 65:
            pick = np.arange(n)
        else:  # the class and non-finite rows, the wave and block edges, the last row, then draws
            edges = [i for i in (63, 64, 255, 256) if i < n] + [n - 1]
            pick = list(dict.fromkeys(list(range(n_head)) + edges))
            rest = np.setdiff1d(np.arange(n), pick)
            extra = np.random.default_rng(n).choice(rest, per_large - len(pick), replace=False)
            pick = np.array(pick + extra.tolist())
        with scalar_mode(_lib.SCALAR_DEVICE), _lib.launched("rtf_kernel") as k, \
                _lib.launched("air2ice_kernel") as kb:
            ref = np.array([solver.rtf_eval(_lib.RTF_AIR2ICE, q[i]) for i in pick])
        assert (k.count, kb.count) == (len(pick), 0), n
        singles += len(pick)
        cases.assert_same_bits(o[:, pick].T, ref, what=n)
    assert singles <= SINGLES_CAP, singles
    # one query through the host entry point in device mode is the kernel too
    _lib.kernel_time("air2ice_kernel")  # reset
    _lib.kernel_timing(True)
    try:
        with scalar_mode(_lib.SCALAR_DEVICE), _lib.launched("air2ice_kernel") as kb:
            o1, s1 = solver.air2ice_host(*cases.KAT)
    finally:
        _lib.kernel_timing(False)
    ms, timed = _lib.kernel_time("air2ice_kernel")
    assert kb.count == 1 and timed == 1 and ms > 0
    q, o, s, _ = thousand
    kat = len(cases.CLASS_ROWS) - 1
    cases.assert_same_bits(o1[:, 0], o[:, kat])
    assert s1[0] == s[kat]


def test_batch_against_the_oracle(solver, oracle_medium):
    """4,096 rows, 60 % A, 20 % B, 10 % C, 10 % D.  Status, probe steps and layer count equal on
    every row; rows whose status has a UB-end, bad-bracket or max-iter bit on those fields only;
    every other row within 1e-9 relative (floor 1e-6) with equal NaN positions, except at most 4
    root-window rows: launch angles that differ by no more than 1e-9 relative, iteration counts
    that differ by at most one, every value within 1e-8.  The values are the twelve physical
    columns, as test_brent_cli._check_air2ice compares them; the Brent iteration count (column 13)
    is not one of them: where f at the last iterates is within its rounding, ocml and the host's
    libm end the search some iterations apart on the same root (measured: 172 of these 4,096 rows,
    by -3 .. +4 iterations, their values within 1.5e-13)."""
    rng = np.random.default_rng(4096)
    q = cases.mixed(4096, rng, parts=(("A", 6), ("B", 2), ("C", 1), ("D", 1)))
    o, s, launches = _solve(solver, q)
    assert launches == 1
    got = o.T
    ref = cases.oracle_rows(oracle_medium, q)
    for col in (cases.STATUS, cases.PROBES, cases.LAYERS):
        assert np.array_equal(got[:, col], ref[:, col]), col
    assert np.array_equal(s, ref[:, cases.STATUS].astype(np.uint8))
    st = ref[:, cases.STATUS].astype(np.int64)
    full = (st & (1 | 2 | 16)) == 0
    ab = np.arange(4096) < 4096 * 8 // 10  # the A and B rows
    assert (~full & ab).sum() < 0.01 * ab.sum()
    err = cases.rel_err(got[:, :12], ref[:, :12])
    err[~full] = 0.0
    over = (err > 1e-9).any(axis=1)
    theta_g, theta_r = got[:, 2], ref[:, 2]
    window = (over & (theta_g != theta_r) & (np.abs(theta_g - theta_r) <= 1e-9 * np.abs(theta_r)) &
              (np.abs(got[:, cases.ITERS] - ref[:, cases.ITERS]) <= 1) &
              (err <= 1e-8).all(axis=1))
    strict = np.where(window[:, None], 0.0, err)
    print(f"[air2ice batch vs oracle] {int(full.sum())} rows on values, {int(window.sum())} "
          f"root-window rows, worst rel outside them {float(strict.max()):.2e}, "
          f"inside {float(err[window].max()) if window.any() else 0.0:.2e}, iteration counts "
          f"differ on {int(((got[:, cases.ITERS] != ref[:, cases.ITERS]) & full).sum())} rows")
    assert not (over & ~window).any(), q[over & ~window][:5]
    assert window.sum() <= 4, q[window]


def test_order_independence(solver, thousand):
    q, o, s, _ = thousand
    perm = np.random.default_rng(7).permutation(len(q))
    op, sp, launches = _solve(solver, q[perm])
    assert launches == 1
    cases.assert_same_bits(op, o[:, perm])
    assert np.array_equal(sp, s[perm])


def test_launch_angles_feed_the_path_sampler(solver):
    """64 status-0 rows of A at one depth: column 2 stays on the device as ray_paths_device's
    launch angles; the sampled ray's horizontal distance in air is the solve's (column 3)."""
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    ice, depth, n = 3000.0, 150.0, 64
    cand = cases.draw("A", 200, np.random.default_rng(64))
    cand[:, 3] = depth
    _, s, _ = _solve(solver, cand)
    q = cand[s == 0][:n]
    assert len(q) == n
    txh, dist = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 1])
    cols = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(4)]
    out = torch.empty((cases.FIELDS, n), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream()
    solver.air2ice_device(*cols, out, stream=st)
    offsets = solver.ray_paths_plan(txh, ice, depth)
    summary = torch.empty((6, n), dtype=torch.float64, device=dev)
    assert out[2].is_contiguous()
    solver.ray_paths_device(out[2], txh, ice, depth, offsets, summary, None, None, stream=st)
    torch.cuda.synchronize()
    o, sm = out.cpu().numpy(), summary.cpu().numpy()
    rel = np.abs(sm[0] - o[3]) / np.abs(o[3])
    print(f"[air2ice -> ray paths] THD in air max rel {rel.max():.2e}")
    assert rel.max() <= 1e-9
    # paths_between(solver="brent") is that composition; the default is the MultiRay one
    ps, po, px, pz, pst = solver.paths_between(txh, dist, depth, ice, solver="brent")
    rs, ro, rx, rz = solver.ray_paths_host(o[2], txh, ice, depth)
    assert np.array_equal(po, offsets) and np.array_equal(ro, offsets)
    assert np.array_equal(pst, np.zeros(n, dtype=np.uint8))
    for a, b in ((ps, rs), (px, rx), (pz, rz)):
        cases.assert_same_bits(a, b)
    cases.assert_same_bits(ps, sm)
    m = 8  # the default keeps the MultiRayAirIceRefraction solve (slot 10)
    ds, do, dx, dz, dst = solver.paths_between(txh[:m], dist[:m], depth, ice)
    sol, sst = solver.solve_host(txh[:m], dist[:m], np.full(m, -depth), ice,
                                 variant=_lib.VARIANT_MULTIRAY)
    es, eo, ex, ez = solver.ray_paths_host(sol[10], txh[:m], ice, depth)
    assert np.array_equal(dst, sst) and np.array_equal(do, eo)
    for a, b in ((ds, es), (dx, ex), (dz, ez)):
        cases.assert_same_bits(a, b)


def test_air_to_air_batch(solver, oracle_medium):
    """The three AirRayTracing geometries of test_air_ray_cli_stdout in one batch."""
    import oracle
    from airiceraytracing_amd import _lib
    geo = [(5000.0, 3100.0, 1000.0), (3100.0, 5000.0, 1000.0), (60000.0, 3000.0, 45000.0)]
    tx, rx, dist = (np.array(c) for c in zip(*geo))
    with _lib.launched("air2ice_kernel") as k:
        out, st, flipped = solver.air_to_air_host(tx, rx, dist)
    assert k.count == 1
    assert flipped.tolist() == [False, True, False]
    for i, (t, r, d) in enumerate(geo):
        ref = oracle.rtf_eval(oracle_medium, oracle.RTF_AIR2ICE, (max(t, r), d, min(t, r), 0.0))
        if t < r:
            ref[4] = 180 - ref[4]
        assert st[i] == int(ref[cases.STATUS]) == 0
        assert np.array_equal(out[12:, i], ref[12:])
        err = cases.rel_err(out[None, :12, i], ref[None, :12])
        assert err.max() <= 1e-9, (geo[i], out[:, i], ref)
        assert abs(out[3, i] - d) < 1e-3
