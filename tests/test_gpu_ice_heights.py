"""The minimizer kernels and the table lookup on the GPU at ice heights other than 3000 m.

Every other GPU test of roots_kernel, roots_sorted_kernel, the stage-2 bodies and the lookup's
fallback has the ice at 3000 m, so they have only run with bottom_layer == 0 and one fixed
air_slim(M, 3000).  Here (generators and the host-route twins in tests/test_ice_heights_cpu.py):

1. the batched solve of both variants at every ICE_HEIGHTS entry against the oracle;
2. the per-block ice endpoint (IceAirPre) against the per-lane recompute, bit for bit, with the
   ice in layers 0, 1 and 2, and against the one-query kernel;
3. the CoREAS entry (IN_CM: ice_cm / 100) at every height;
4. a trace batch whose ice height changes per query (all four layer-span classes of
   query_bucket), block-local and grouped, against the oracle and each other;
5. the guarded bisection against the every-midpoint form at ice 0 and 9000 m;
6. the table lookup and its minimizer fallback (IN_CM100) over ice at 0 and 4000 m, single and
   multi-antenna launches;
7. Tx within 50 m of the ice, where the geometric path in air takes a measured absolute bound
   (DESIGN.md §3).

n = 2 * 1024 + 37 per batch: two full roots_kernel blocks and a ragged third."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import parity
from tests import test_ice_heights_cpu as cpu
from tests.test_ice_heights_cpu import (GEO_AIR_NEAR_ICE_ATOL_M, GEO_AIR_SLOT, ICE_HEIGHTS,
                                        ICE_PARAMS, NEAR_ICE_HEIGHTS, NEAR_N, VARIANTS,
                                        ice_height_queries, mixed_ice_trace_queries,
                                        near_ice_queries, oracle_solve)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTHREADS = min(16, os.cpu_count() or 1)
N_BATCH = 2 * 1024 + 37


@pytest.fixture(scope="module")
def solvers():
    return {v: cpu.make_solver(v) for v in VARIANTS}


def _report(name, rep, extra=""):
    print(f"[{name}] n={rep['n']} max_rel={rep['max_rel']:.3e} max_abs={rep['max_abs']:.3e} "
          f"bad={rep['n_bad']} cols={rep['bad_cols']} {extra}")


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    if a.dtype.kind == "f":
        bad = np.argwhere(a.view(np.int64) != b.view(np.int64))
    else:
        bad = np.argwhere(a != b)
    assert bad.size == 0, f"{bad.shape[0]} differing entries, first {bad[:5].tolist()}"


def _solve_device(s, txh, dist, depth, ice):
    """solve_device on host arrays: (out (fields, n), status) as numpy."""
    import torch
    from airiceraytracing_amd import VARIANT_PYWRAPPER, _lib
    dev = torch.device("cuda:0")
    n = txh.size
    fields = _lib.PYSOLVE_FIELDS if s.variant == VARIANT_PYWRAPPER else _lib.SOLVE_FIELDS
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (txh, dist, depth)]
    out = torch.empty((fields, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    s.solve_device(t[0], t[1], t[2], ice, out, st, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), st.cpu().numpy()


def _hdtip_device(s, src, dist, dep, ice_cm):
    import torch
    dev = torch.device("cuda:0")
    n = src.size
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (src, dist, dep)]
    out = torch.empty((9, n), dtype=torch.float64, device=dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    s.hdtip_device(t[0], t[1], t[2], ice_cm, out, ok, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), ok.cpu().numpy()


def _trace_device(s, depth, ice, txh, dist):
    import torch
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (depth, ice, txh, dist)]
    out = torch.empty((depth.size, 10), dtype=torch.float64, device=dev)
    s.trace_ice_to_air_device(*t, out, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------ 1. batched solve
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ice", ICE_PARAMS)
def test_solve_batch_vs_oracle(solvers, oracle_medium, oracle_medium_py, ice, variant):
    """2085 queries per ice height through roots_kernel (one launch, no one-query kernel) and the
    variant's stage 2: status equal on the pinned rows, the unpinned flags equal on every row,
    every column within 1e-9, pinned share over 0.95."""
    from airiceraytracing_amd import _lib
    txh, dist, depth = ice_height_queries(ice, N_BATCH, seed=200 + ICE_HEIGHTS.index(ice))
    with _lib.launched("roots_kernel") as kr, _lib.launched("scalar_solve_kernel") as k1:
        out, st = _solve_device(solvers[variant], txh, dist, depth, ice)
    assert kr.count == 1 and k1.count == 0
    ref, rst, floors = oracle_solve(variant, oracle_medium, oracle_medium_py, txh, dist, depth, ice,
                                    nthreads=NTHREADS)
    mask = (rst & oracle.SOLVE_UNPINNED) == 0
    rep = parity.compare_columns(out, ref, floors, mask=mask)
    _report(f"solve {variant} ice={ice!r}", rep, f"pinned={mask.mean():.4f}")
    assert mask.mean() > 0.95
    np.testing.assert_array_equal(st[mask], rst[mask])
    np.testing.assert_array_equal(st & oracle.SOLVE_UNPINNED, rst & oracle.SOLVE_UNPINNED)
    assert rep["ok"], rep


# ------------------------------------------------------------------ 2. pre against recompute
def _in_ice_block(ice, seed):
    """1024 queries with the antenna in the ice (a full roots_kernel block), and as many with it
    in the air as the mixed batches below need."""
    txh, dist, depth = ice_height_queries(ice, 1400, seed=seed)
    k = np.flatnonzero(depth < 0)[:1024]
    assert k.size == 1024
    rng = np.random.default_rng(seed + 1)
    m = 32 * 1024
    up = rng.uniform(1.0, 240.0, m)
    air = (rng.uniform(ice + 500.0, 1e5, m), rng.uniform(0.0, 5e4, m), up)
    return (txh[k], dist[k], depth[k]), air


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ice", [pytest.param(2835.0, id="layer0"), pytest.param(4000.0, id="layer1"),
                                 pytest.param(9000.0, id="layer2")])
def test_block_ice_endpoint_equals_recompute(solvers, ice, variant):
    """RootSearch::begin takes the block's IceAirPre when no lane of the wave has another ice
    height (__ballot(g.ice != pre->x) == 0), else bottom_layer / air_slim per lane; both form
    air_slim(M, ice, n) of the same value, so the results must be the same bits.

    (a) 1024 in-ice queries alone: one block, every wave on the block's copy.
    (b) the same with an Rx-in-air query in place of every 64th (lane 0 of every wave as loaded).
        roots_kernel sorts its block by straight-line angle before solving, so this alone does not
        put an Rx-in-air query into every wave that is solved; hence
    (b2) 32 blocks, each holding 32 of the queries at fixed places among 992 Rx-in-air queries: no
        64 lanes of a full block can then be free of a shifted ice height, wherever the sort puts
        them, so every wave recomputes.
    (c) a strided 16 of them through the one-query kernel (AIRICE_SCALAR_DEVICE, n = 1).
    The queries (a) shares with (b), (b2) and (c) must agree bit for bit, status included."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    s = solvers[variant]
    (txh, dist, depth), air = _in_ice_block(ice, seed=500 + int(ice))
    with _lib.launched("roots_kernel") as kr:
        out_a, st_a = _solve_device(s, txh, dist, depth, ice)
    assert kr.count == 1
    # (b)
    q = [a.copy() for a in (txh, dist, depth)]
    lane0 = np.arange(0, 1024, 64)
    for a, f in zip(q, air):
        a[lane0] = f[:lane0.size]
    assert (q[2][lane0] > 0).all()
    out_b, st_b = _solve_device(s, *q, ice)
    keep = np.setdiff1d(np.arange(1024), lane0)
    _bits_equal(st_a[keep], st_b[keep])
    _bits_equal(out_a[:, keep], out_b[:, keep])
    # (b2)
    big = [f.copy() for f in air]
    assert big[0].size == 32 * 1024  # full blocks only: a ragged wave could hold in-ice lanes alone
    place = (np.arange(1024) // 32) * 1024 + (np.arange(1024) % 32) * 32 + 5
    for a, f in zip(big, (txh, dist, depth)):
        a[place] = f
    blocks = place // 1024
    assert np.bincount(blocks, minlength=32).max() == 32 and (np.delete(big[2], place) > 0).all()
    out_c, st_c = _solve_device(s, *big, ice)
    _bits_equal(st_a, st_c[place])
    _bits_equal(out_a, out_c[:, place])
    # (c)
    pick = np.arange(7, 1024, 64)
    with scalar_mode(_lib.SCALAR_DEVICE), _lib.launched("scalar_solve_kernel") as k1:
        for i in pick:
            o, so = s.solve_host(txh[i:i + 1], dist[i:i + 1], depth[i:i + 1], ice)
            _bits_equal(o[:, 0], out_a[:, i])
            assert so[0] == st_a[i], (i, so[0], st_a[i])
    assert k1.count == pick.size
    assert np.isfinite(out_a[10]).mean() > 0.95  # the compared rows hold solved launch angles


# ------------------------------------------------------------------ 3. the CoREAS entry
@pytest.mark.parametrize("ice", ICE_PARAMS)
def test_hdtip_vs_oracle(solvers, oracle_medium, ice):
    """GetHorizontalDistanceToIntersectionPoint in cm (IN_CM: Q.ice / 100 feeds the block's ice
    endpoint and load_query), 1061 queries: one full block and 37 lanes."""
    n = 1024 + 37
    txh, dist, depth = ice_height_queries(ice, n, seed=600 + ICE_HEIGHTS.index(ice))
    src, dcm, pcm, ice_cm = txh * 100, dist * 100, depth * 100, 100 * ice
    out, ok = _hdtip_device(solvers["multiray"], src, dcm, pcm, ice_cm)
    ref, rok, rst = oracle.hdtip_batch(oracle_medium, src, dcm, pcm, ice_cm, nthreads=NTHREADS)
    mask = (rst & oracle.SOLVE_UNPINNED) == 0
    rep = parity.compare_columns(out, ref, parity.HDTIP_FLOORS, mask=mask)
    _report(f"hdtip ice={ice!r}", rep, f"pinned={mask.mean():.4f} ok={rok[mask].mean():.4f}")
    assert mask.mean() > 0.95
    assert np.array_equal(ok.astype(bool)[mask], rok[mask])
    assert rep["ok"], rep


# ------------------------------------------------------------------ 4. trace, ice per query
N_TRACE, TRACE_SEED = 4096 + 37, 43

CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from airiceraytracing_amd import AirIceSolver, VARIANT_PYWRAPPER, _lib
from tests.test_ice_heights_cpu import mixed_ice_trace_queries
n, seed, path = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
dev = torch.device("cuda:0")
s = AirIceSolver(variant=VARIANT_PYWRAPPER)
t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in mixed_ice_trace_queries(n, seed)]
out = torch.empty((n, 10), dtype=torch.float64, device=dev)
_lib.kernel_timing(True)  # the timer of the grouping passes tells the two schedules apart
with _lib.launched("roots_kernel") as kr:
    s.trace_ice_to_air_device(*t, out, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
_lib.kernel_timing(False)
np.savez(path, trace=out.cpu().numpy(), root_launches=kr.count,
         group_passes=_lib.kernel_time("group_passes")[1])
"""


def _run_child(group_min, path):
    env = dict(os.environ)
    env["AIRICE_GROUP_MIN"] = str(group_min)
    env.pop("AIRICE_SOLVE_STATS", None)
    env.pop("AIRICE_BISECT_EXACT", None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(N_TRACE), str(TRACE_SEED), path],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.load(path)


@pytest.fixture(scope="module")
def mixed_trace(solvers, oracle_medium_py):
    q = mixed_ice_trace_queries(N_TRACE, TRACE_SEED)
    ref = oracle.py_trace_batch(oracle_medium_py, *q, nthreads=NTHREADS)
    return q, ref, _trace_device(solvers["pywrapper"], *q)


def _assert_trace_matches(name, out, ref):
    solved = ref[:, 0] != -1000
    assert np.array_equal(out[:, 0] != -1000, solved)
    rep = parity.compare_columns(out.T, ref.T, parity.TRACE_FLOORS)
    _report(name, rep, f"solved={solved.mean():.4f}")
    assert rep["ok"], rep
    # +-0.03 of the oracle's own share (the masks are equal, so this holds the batch itself to
    # a share one can recognise: 0.97 and more)
    assert abs((out[:, 0] != -1000).mean() - solved.mean()) <= 0.03


def test_trace_mixed_ice_vs_oracle(mixed_trace, oracle_medium_py):
    (depth, ice, txh, dist), ref, out = mixed_trace
    span = cpu.span_classes(oracle_medium_py, txh, ice)
    assert set(span.tolist()) == {0, 1, 2, 3}
    # one wave of the batch as loaded holds several ice heights
    assert min(np.unique(ice[w * 64:(w + 1) * 64]).size for w in range(N_TRACE // 64)) >= 3
    _assert_trace_matches("trace mixed ice", out, ref)


def test_trace_mixed_ice_grouped_equals_block_local(mixed_trace, tmp_path):
    """The same batch in two fresh processes, AIRICE_GROUP_MIN=0 (roots_kernel) and =1
    (roots_sorted_kernel, whose sort key holds the layer span): bit-identical, and the grouped one
    against the oracle."""
    _, ref, out = mixed_trace
    local = _run_child(0, str(tmp_path / "local.npz"))
    grouped = _run_child(1, str(tmp_path / "grouped.npz"))
    assert int(local["root_launches"]) == 1 and int(local["group_passes"]) == 0
    assert int(grouped["root_launches"]) == 1 and int(grouped["group_passes"]) == 1
    _bits_equal(local["trace"], grouped["trace"])
    _bits_equal(local["trace"], out)
    _assert_trace_matches("trace mixed ice, grouped", grouped["trace"], ref)


# ------------------------------------------------------------------ 5. guard replay
def _both(fn):
    old = os.environ.pop("AIRICE_BISECT_EXACT", None)
    try:
        fast = fn()
        os.environ["AIRICE_BISECT_EXACT"] = "1"
        exact = fn()
    finally:
        os.environ.pop("AIRICE_BISECT_EXACT", None)
        if old is not None:
            os.environ["AIRICE_BISECT_EXACT"] = old
    return fast, exact


@pytest.mark.parametrize("ice", [pytest.param(0.0, id="0"), pytest.param(9000.0, id="9000")])
def test_guard_replay(solvers, ice):
    """AIRICE_BISECT_EXACT=1 (f at every midpoint) against the guarded bisection: bit-identical
    solve and trace outputs (the _both pattern of tests/test_gpu_bisect_replay.py)."""
    txh, dist, depth = ice_height_queries(ice, N_BATCH, seed=700 + int(ice))
    (out_f, st_f), (out_e, st_e) = _both(
        lambda: _solve_device(solvers["multiray"], txh, dist, depth, ice))
    _bits_equal(st_f, st_e)
    _bits_equal(out_f, out_e)
    ices = np.full(txh.size, ice)
    fast, exact = _both(lambda: _trace_device(solvers["pywrapper"], depth, ices, txh, dist))
    _bits_equal(fast, exact)
    assert (fast[:, 0] != -1000).mean() > 0.5


# ------------------------------------------------------------------ 6. table lookup
LOOKUP_GRID = (250.0, 92.0, 180.0, 0.5)  # height step (m), start / stop angle, angle step (deg)
LOOKUP_DEPTHS_CM = (-20000.0, 5000.0)
LOOKUP_NQ = 2000


class LookupCase:
    """Both antennas' coarse tables over one ice height (one tables_device launch), each with its
    own parity.lookup_queries."""

    def __init__(self, solver, ice_cm):
        import torch
        from airiceraytracing_amd import make_grid
        self.solver, self.ice_cm = solver, ice_cm
        self.dev = torch.device("cuda:0")
        self.grids = [make_grid(d, ice_cm, *LOOKUP_GRID) for d in LOOKUP_DEPTHS_CM]
        self.buffers = [torch.empty((11, g.n_rays), dtype=torch.float32, device=self.dev)
                        for g in self.grids]
        solver.tables_device(self.grids, self.buffers, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        self.hosts = [b.cpu().numpy() for b in self.buffers]
        self.tables = [solver.lookup_table(b, g) for b, g in zip(self.buffers, self.grids)]
        self.queries = [parity.lookup_queries(h, LOOKUP_NQ) for h in self.hosts]

    def run_single(self, a, src, dist):
        import torch
        n = src.size
        ts, td = (torch.from_numpy(np.ascontiguousarray(x)).to(self.dev) for x in (src, dist))
        tp = torch.full((n,), LOOKUP_DEPTHS_CM[a], dtype=torch.float64, device=self.dev)
        out = torch.empty((9, n), dtype=torch.float64, device=self.dev)
        ok = torch.empty(n, dtype=torch.uint8, device=self.dev)
        fl = torch.empty(n, dtype=torch.uint8, device=self.dev)
        self.solver.table_lookup_device(self.tables[a], ts, td, tp, self.ice_cm, out, ok, fl,
                                        stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        return out.cpu().numpy(), ok.cpu().numpy(), fl.cpu().numpy()


@pytest.fixture(scope="module", params=[0.0, 400000.0], ids=["ice0", "ice4000m"])
def lookup_case(request, solvers):
    return LookupCase(solvers["multiray"], request.param)


@pytest.mark.parametrize("a", [0, 1], ids=["rx-200m", "rx+50m"])
def test_lookup_vs_oracle(lookup_case, oracle_medium, a):
    """GetHorizontalDistanceToIntersectionPoint_Table over ice at 0 m and 4000 m, antenna 200 m
    deep and 50 m up, on make_grid(depth, ice_cm, 250.0, 92.0, 180.0, 0.5) (the oracle flags 2 to
    5 fallback rows of 2514 on each of the four tables, so this grid needed no coarsening): flags
    and ok equal, non-fallback lanes bit-identical, fallback lanes (IN_CM100) at 1e-9 where the
    oracle's solve of the x100 arguments is pinned -- the rules of tests/test_gpu_lookup.py."""
    c = lookup_case
    src, dist = c.queries[a]
    dep = np.full(src.size, LOOKUP_DEPTHS_CM[a])
    out, ok, fl = c.run_single(a, src, dist)
    og = oracle.grid_init(LOOKUP_DEPTHS_CM[a], c.ice_cm, *LOOKUP_GRID)
    assert (og.table_rows, og.angle_steps) == (c.grids[a].table_rows, c.grids[a].angle_steps)
    rout, rok, rfl = oracle.table_lookup_batch(oracle_medium, oracle.lookup_table(c.hosts[a], og),
                                               src, dist, dep, c.ice_cm, nthreads=NTHREADS)
    assert np.array_equal(fl, rfl), np.flatnonzero(fl != rfl)[:10]
    fb = (rfl & oracle.LOOKUP_FALLBACK) != 0
    assert fb.any(), "no fallback row: IN_CM100 did not run at this ice height"
    x, y = out[:, ~fb], rout[:, ~fb]
    same = (x == y) | (np.isnan(x) & np.isnan(y))
    assert same.all(), np.argwhere(~same)[:10]
    assert np.array_equal(ok[~fb], rok[~fb])
    idx = np.flatnonzero(fb)
    fst = np.array([oracle.air2ice(oracle_medium, src[i], dist[i], c.ice_cm / 100, dep[i])[1]
                    for i in idx])
    mask = (fst & oracle.SOLVE_UNPINNED) == 0
    assert np.array_equal(ok[idx][mask], rok[idx][mask])
    rep = parity.compare_columns(out[:, idx], rout[:, idx], parity.HDTIP_FLOORS, mask=mask)
    _report(f"lookup ice_cm={c.ice_cm} depth_cm={LOOKUP_DEPTHS_CM[a]}", rep,
            f"ok={int(ok.sum())} fallback={idx.size} (masked {int((~mask).sum())})")
    assert rep["ok"], rep
    # The x100 arguments put most fallback sources above the atmosphere (no air layer): unpinned
    # for the rule above, which over ice at 4000 m leaves it no row.  The probe's outcome there
    # is replayed without evaluations and compares under the oracle's zeroed-state model, as
    # tests/test_gpu_parity.py::test_solve_no_air_layer has it for the batched solve: those rows
    # are held to the oracle as well.
    noair = (fst & oracle.SOLVE_NO_AIR_LAYER) != 0
    assert (mask | noair).any()
    assert np.array_equal(ok[idx][noair], rok[idx][noair])
    rep = parity.compare_columns(out[:, idx], rout[:, idx], parity.HDTIP_FLOORS, mask=noair)
    _report("  the no-air-layer fallback rows", rep)
    assert rep["ok"], rep


def test_lookup_multi_equals_single(lookup_case):
    """The same sources through table_lookup_multi_device with both antennas (lookup_multi_kernel,
    one launch): bit-identical to one table_lookup_device launch per antenna."""
    import torch
    from airiceraytracing_amd import _lib
    c = lookup_case
    src = c.queries[0][0]
    dist = np.stack([c.queries[0][1], c.queries[1][1]])
    n = src.size
    assert dist.shape == (2, n)
    single = [c.run_single(a, src, dist[a]) for a in (0, 1)]
    out = torch.empty((9, 2 * n), dtype=torch.float64, device=c.dev)
    ok = torch.empty(2 * n, dtype=torch.uint8, device=c.dev)
    fl = torch.empty(2 * n, dtype=torch.uint8, device=c.dev)
    with _lib.launched("lookup_multi_kernel") as km:
        work = c.solver.table_lookup_multi_device(
            c.tables, [0, 1], list(LOOKUP_DEPTHS_CM), torch.from_numpy(src).to(c.dev),
            torch.from_numpy(dist).to(c.dev), c.ice_cm, out, ok, fl,
            stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
    del work
    assert km.count == 1
    out, ok, fl = out.cpu().numpy().reshape(9, 2, n), ok.cpu().numpy().reshape(2, n), \
        fl.cpu().numpy().reshape(2, n)
    for a in (0, 1):
        _bits_equal(out[:, a], single[a][0])
        _bits_equal(ok[a], single[a][1])
        _bits_equal(fl[a], single[a][2])
    assert (np.concatenate([s[2] for s in single]) & oracle.LOOKUP_FALLBACK).any()


# ------------------------------------------------------------------ 7. Tx close to the ice
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ice", NEAR_ICE_HEIGHTS)
def test_near_ice_solve_vs_oracle(solvers, oracle_medium, oracle_medium_py, ice, variant):
    """Tx 0.5, 1, 10 and 50 m over the ice: every column but the geometric path in air under the
    unchanged rule, that column within GEO_AIR_NEAR_ICE_ATOL_M (measured)."""
    txh, dist, depth = near_ice_queries(ice, NEAR_N, seed=300 + int(ice))
    out, st = _solve_device(solvers[variant], txh, dist, depth, ice)
    ref, rst, floors = oracle_solve(variant, oracle_medium, oracle_medium_py, txh, dist, depth, ice)
    mask = (rst & oracle.SOLVE_UNPINNED) == 0
    rep = cpu.compare_except_geo_air(out, ref, floors, GEO_AIR_SLOT[variant], mask,
                                     GEO_AIR_NEAR_ICE_ATOL_M[variant])
    _report(f"near ice {variant} ice={ice}", rep,
            f"pinned={mask.mean():.4f} geo_air_max_abs={rep['geo_air_max_abs']:.3e}")
    cpu.assert_every_offset_pinned(mask)
    np.testing.assert_array_equal(st[mask], rst[mask])
    np.testing.assert_array_equal(st & oracle.SOLVE_UNPINNED, rst & oracle.SOLVE_UNPINNED)
    assert rep["ok"], rep
    assert rep["geo_air_ok"], rep


def _near_ice_all():
    parts = [near_ice_queries(ice, NEAR_N, seed=300 + int(ice)) + (np.full(NEAR_N, ice),)
             for ice in NEAR_ICE_HEIGHTS]
    return parts, [np.concatenate([p[k] for p in parts]) for k in range(4)]


def test_near_ice_hdtip_and_trace_vs_oracle(solvers, oracle_medium, oracle_medium_py):
    """The entry points that report the same geometric path: the CoREAS entry's
    geometricalPathLengthInAir (cm) and Py_TraceIceToAir's slot 3."""
    parts, (txh, dist, depth, ice) = _near_ice_all()
    for t, d, p, i in parts:
        ice_cm = 100 * float(i[0])
        out, ok = _hdtip_device(solvers["multiray"], t * 100, d * 100, p * 100, ice_cm)
        ref, rok, rst = oracle.hdtip_batch(oracle_medium, t * 100, d * 100, p * 100, ice_cm)
        mask = (rst & oracle.SOLVE_UNPINNED) == 0
        rep = cpu.compare_except_geo_air(out, ref, parity.HDTIP_FLOORS, GEO_AIR_SLOT["hdtip"], mask,
                                         GEO_AIR_NEAR_ICE_ATOL_M["hdtip_cm"])
        _report(f"near ice hdtip ice_cm={ice_cm}", rep,
                f"geo_air_max_abs={rep['geo_air_max_abs']:.3e} cm")
        cpu.assert_every_offset_pinned(mask)
        assert np.array_equal(ok.astype(bool)[mask], rok[mask])
        assert rep["ok"] and rep["geo_air_ok"], rep
    out = _trace_device(solvers["pywrapper"], depth, ice, txh, dist)
    ref = oracle.py_trace_batch(oracle_medium_py, depth, ice, txh, dist)
    solved = ref[:, 0] != -1000
    assert np.array_equal(out[:, 0] != -1000, solved) and solved.sum() >= 32
    assert np.array_equal(out[~solved], ref[~solved])
    rep = cpu.compare_except_geo_air(out.T, ref.T, parity.TRACE_FLOORS, GEO_AIR_SLOT["trace"],
                                     solved, GEO_AIR_NEAR_ICE_ATOL_M["trace"])
    _report("near ice trace", rep, f"solved={solved.mean():.4f} "
            f"geo_air_max_abs={rep['geo_air_max_abs']:.3e}")
    assert rep["ok"] and rep["geo_air_ok"], rep


@pytest.mark.parametrize("variant", VARIANTS)
def test_near_ice_device_error_against_exact(solvers, oracle_medium, oracle_medium_py, variant):
    """The device's geometric path in air against the 50-digit evaluation at the device's own
    launch angle: off by no more than twice what the oracle is off by on the same rows."""
    pytest.importorskip("mpmath")
    worst, sets = cpu.near_ice_oracle_errors(variant, oracle_medium, oracle_medium_py)
    m = oracle_medium_py if variant == "pywrapper" else oracle_medium
    slot = GEO_AIR_SLOT[variant]
    dev_worst = 0.0
    for txh, dist, depth, ice, rows in sets:
        out, _ = _solve_device(solvers[variant], txh, dist, depth, ice)
        eff = ice + np.maximum(depth, 0.0)
        err = cpu.geo_air_errors(m, txh, eff, out[10], out[slot], rows)
        dev_worst = max(dev_worst, float(err.max()))
    print(f"[near ice {variant}] max |geo_air - exact|: oracle {worst:.4e} m, device "
          f"{dev_worst:.4e} m")
    assert worst <= cpu.GEO_AIR_ORACLE_ERR_M[variant]
    assert dev_worst <= 2 * worst
