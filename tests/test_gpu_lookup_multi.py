"""The multi-antenna table lookup (airice_table_lookup_launch_multi, lookup_multi_kernel) on the
GPU: n_ant antennas x n_src sources in one launch give the bits of one single-antenna launch per
antenna, and the oracle's lookup on the same tables under the tolerances of test_gpu_lookup.

Four antennas over ice at 3000 m: depths -200 m, -100 m, -200 m (shares table 0) and +50 m (in the
air: another LoopStopHeight and row count), tables on the coarse grid of test_lookup_oracle
(250 m x 0.2 deg).  5014 sources: 39 blocks of 128 lanes and a 22-lane tail; the distance rows
and the output columns have strides that are no multiple of anything."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTHREADS = min(16, os.cpu_count() or 1)
ICE_CM = 300000.0
DEPTHS = [-20000.0, -10000.0, -20000.0, 5000.0]
ANTENNA_TABLE = [0, 1, 0, 2]
GRID = (250.0, 90.1, 180.0, 0.2)  # height step, start angle, stop angle, angle step
NQ, SEED = 4000, 99
N_SRC = 5014


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


class Case:
    """The tables (one tables_device launch), the queries and the single-antenna results."""

    def __init__(self, solver):
        import torch
        from airiceraytracing_amd import dedupe_depths, make_grid
        self.solver = solver
        self.dev = torch.device("cuda:0")
        distinct, amap = dedupe_depths(DEPTHS)
        assert amap == ANTENNA_TABLE and len(distinct) == 3
        self.distinct = distinct
        self.grids = [make_grid(d, ICE_CM, *GRID) for d in distinct]
        self.buffers = [torch.empty((11, g.n_rays), dtype=torch.float32, device=self.dev)
                        for g in self.grids]
        solver.tables_device(self.grids, self.buffers, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert self.grids[2].n_rays != self.grids[0].n_rays  # the antenna in the air
        self.hosts = [b.cpu().numpy() for b in self.buffers]
        self.unpacked = [solver.lookup_table(b, g) for b, g in zip(self.buffers, self.grids)]
        self.packed = [solver.lookup_table(b, g) for b, g in zip(self.buffers, self.grids)]
        for t in self.packed:
            solver.lookup_pack(t, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        src, _ = parity.lookup_queries(self.hosts[0], NQ, seed=SEED)
        assert src.size == N_SRC
        self.src = src
        self.dist = np.stack([parity.lookup_queries(self.hosts[ANTENNA_TABLE[a]], NQ,
                                                    seed=SEED + a)[1] for a in range(4)])
        assert self.dist.shape == (4, N_SRC)
        self.d_src = torch.from_numpy(src).to(self.dev)
        self.ld_dist = N_SRC + 13
        d_dist = torch.zeros((4, self.ld_dist), dtype=torch.float64, device=self.dev)
        d_dist[:, :N_SRC] = torch.from_numpy(self.dist).to(self.dev)
        self.d_dist = d_dist[:, :N_SRC]  # row stride ld_dist
        self.single = self.run_single(self.packed, N_SRC)

    def run_single(self, tables, n_src, antennas=range(4)):
        """One table_lookup_device launch per antenna: [(out (9, n), ok, flags)]."""
        import torch
        res = []
        for a in antennas:
            out = torch.empty((9, n_src), dtype=torch.float64, device=self.dev)
            ok = torch.empty(n_src, dtype=torch.uint8, device=self.dev)
            fl = torch.empty(n_src, dtype=torch.uint8, device=self.dev)
            dep = torch.full((n_src,), DEPTHS[a], dtype=torch.float64, device=self.dev)
            self.solver.table_lookup_device(tables[ANTENNA_TABLE[a]], self.d_src[:n_src],
                                            self.d_dist[a, :n_src].contiguous(), dep, ICE_CM, out,
                                            ok, fl, stream=torch.cuda.current_stream())
            torch.cuda.synchronize()
            res.append((out.cpu().numpy(), ok.cpu().numpy(), fl.cpu().numpy()))
        return res

    def run_multi(self, tables, n_src, antennas=range(4), pad=5):
        """One multi launch: (out (9, n_ant, n_src), ok (n_ant, n_src), flags, launches of
        lookup_multi_kernel, launches of lookup_kernel)."""
        import torch
        from airiceraytracing_amd import _lib
        antennas = list(antennas)
        n_ant = len(antennas)
        ld = n_ant * n_src + pad
        out = torch.full((9, ld), -7.0, dtype=torch.float64, device=self.dev)
        ok = torch.full((n_ant * n_src,), 9, dtype=torch.uint8, device=self.dev)
        fl = torch.full((n_ant * n_src,), 9, dtype=torch.uint8, device=self.dev)
        dist = self.d_dist[antennas[0]:antennas[-1] + 1, :n_src]
        with _lib.launched("lookup_multi_kernel") as km, _lib.launched("lookup_kernel") as k1:
            self.solver.table_lookup_multi_device(
                tables, [ANTENNA_TABLE[a] for a in antennas], [DEPTHS[a] for a in antennas],
                self.d_src[:n_src], dist, ICE_CM, out, ok, fl, ld=ld,
                stream=torch.cuda.current_stream())
            torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, n_ant * n_src:] == -7.0).all()  # the padding of the columns is untouched
        return (o[:, :n_ant * n_src].reshape(9, n_ant, n_src),
                ok.cpu().numpy().reshape(n_ant, n_src), fl.cpu().numpy().reshape(n_ant, n_src),
                km.count, k1.count)


@pytest.fixture(scope="module")
def case(solver):
    return Case(solver)


def _assert_same(multi, single, antennas=range(4)):
    out, ok, fl = multi[:3]
    for j, a in enumerate(antennas):
        so, sk, sf = single[j]
        assert np.array_equal(out[:, j], so, equal_nan=True), (a, np.argwhere(
            ~((out[:, j] == so) | (np.isnan(out[:, j]) & np.isnan(so))))[:5])
        assert np.array_equal(ok[j], sk), a
        assert np.array_equal(fl[j], sf), a


def test_bit_identical_to_single_antenna_launches(case):
    from airiceraytracing_amd import LOOKUP_FALLBACK
    assert case.ld_dist == N_SRC + 13 and case.d_dist.stride(0) == case.ld_dist
    multi = case.run_multi(case.packed, N_SRC)
    assert multi[3] == 1 and multi[4] == 0  # one multi launch, no single-antenna launch in it
    _assert_same(multi, case.single)
    fb = [int(np.count_nonzero(case.single[a][2] & LOOKUP_FALLBACK)) for a in range(4)]
    print(f"[lookup multi] fallback lanes per antenna: {fb}")
    assert fb[0] > 0, "no fallback lane for antenna 0: the in-place minimizer path is untested"


def test_oracle_parity(case, oracle_medium):
    """tests/test_gpu_lookup.py::_run_case per antenna, on the multi launch's outputs."""
    out, ok, fl = case.run_multi(case.packed, N_SRC)[:3]
    for a in range(4):
        t = ANTENNA_TABLE[a]
        og = oracle.grid_init(case.distinct[t], ICE_CM, *GRID)
        dep = np.full(N_SRC, DEPTHS[a])
        src, dist = case.src, case.dist[a]
        rout, rok, rfl = oracle.table_lookup_batch(
            oracle_medium, oracle.lookup_table(case.hosts[t], og), src, dist, dep, ICE_CM,
            nthreads=NTHREADS)
        assert np.array_equal(fl[a], rfl), (a, np.flatnonzero(fl[a] != rfl)[:10])
        fb = (rfl & oracle.LOOKUP_FALLBACK) != 0
        x, y = out[:, a][:, ~fb], rout[:, ~fb]
        same = (x == y) | (np.isnan(x) & np.isnan(y))
        assert same.all(), (a, np.argwhere(~same)[:10])
        assert np.array_equal(ok[a][~fb], rok[~fb])
        idx = np.flatnonzero(fb)
        mask = np.ones(idx.size, dtype=bool)
        for j, i in enumerate(idx):
            _, st = oracle.air2ice(oracle_medium, src[i], dist[i], ICE_CM / 100, dep[i])
            mask[j] = (st & oracle.SOLVE_UNPINNED) == 0
        if idx.size:
            assert np.array_equal(ok[a][idx][mask], rok[idx][mask])
            rep = parity.compare_columns(out[:, a][:, idx], rout[:, idx], parity.HDTIP_FLOORS,
                                         mask=mask)
            assert rep["ok"], (a, rep)
        print(f"[lookup multi, antenna {a}] fallback={idx.size} (masked {int((~mask).sum())})")


def test_mixed_packed_and_unpacked_tables(case):
    mixed = [case.packed[0], case.unpacked[1], case.packed[2]]
    assert mixed[1].entries is None and mixed[0].entries and mixed[2].entries
    _assert_same(case.run_multi(mixed, N_SRC), case.single)


@pytest.mark.parametrize("n_src", [1, 127, 129])
def test_small_source_counts(case, n_src):
    multi = case.run_multi(case.packed, n_src, pad=3)
    assert multi[3] == 1
    _assert_same(multi, case.run_single(case.packed, n_src))


def test_one_antenna(case):
    """n_ant = 1: the antenna in the air, alone (table index 2 of 3)."""
    multi = case.run_multi(case.packed, N_SRC, antennas=[3])
    assert multi[3] == 1
    _assert_same(multi, [case.single[3]], antennas=[3])


def test_antenna_tables_lookup(case, solver):
    import torch
    at = solver.antenna_tables(DEPTHS, ICE_CM, *GRID, stream=torch.cuda.current_stream())
    assert at.antenna_table == ANTENNA_TABLE and len(at.tables) == 3
    assert all(t.entries for t in at.tables)
    for b, ref in zip(at.buffers, case.buffers):
        assert torch.equal(b.view(torch.int32), ref.view(torch.int32))
    out, ok, fl = at.lookup(case.d_src, case.d_dist, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert tuple(out.shape) == (9, 4, N_SRC) and tuple(ok.shape) == (4, N_SRC)
    _assert_same((out.cpu().numpy(), ok.cpu().numpy(), fl.cpu().numpy()), case.single)


def test_cpp_table_lookup_batch_multi(tmp_path):
    """tests/cpp/multiray_lookup_multi_driver.cpp: the caller's AntennaDepths /
    AntennaTableAlreadyMade send antenna 2 to table 0; every antenna of TableLookupBatchMulti is
    bit-identical to TableLookupBatch."""
    exe = os.path.join(ROOT, "tests", "cpp", "multiray_lookup_multi_driver")
    assert os.path.exists(exe), "build with __graft_entry__.build()"
    with open(os.path.join(ROOT, "airiceraytracing_amd", "data", "Atmosphere.dat.gz"), "rb") as f:
        (tmp_path / "Atmosphere.dat").write_bytes(gzip.decompress(f.read()))
    env = dict(os.environ, AIRICE_LAUNCH_REPORT="1")
    run = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stderr
    r = json.loads(run.stdout)
    assert r["tables"] == 2
    rows = np.array(r["rows"])
    assert rows.shape == (27, 4)
    assert (rows[:, 3] == 1).all(), rows[rows[:, 3] != 1]
    assert rows[:, 2].any() and not rows[:, 2].all()  # both values of the returned bool occur
    counts = dict(kv.split("=") for kv in run.stderr.split("airice launches:")[1].split())
    assert int(counts["lookup_multi_kernel"]) == 1 and int(counts["lookup_kernel"]) == 3
