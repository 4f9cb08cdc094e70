"""The two-layer (double-exponential) firn on the GPU: the layered table kernels (cold, warm,
multi-antenna), the layered rays kernel and the Python keyword, on one small grid -- ice at
3216 m, 49 rows x 129 launch angles (rows straddle blocks, the last block is partial), the Summit
firn.  The reference is the composition of three one-layer oracle tables (tests/firn_cases.py),
the bound the project's parity rule (tests/parity.py; float tables within 1 ulp)."""
import ctypes

import numpy as np
import pytest

from tests import firn_cases as fc
from tests import parity

pytestmark = pytest.mark.gpu

ICE_CM = fc.ICE_M * 100.0
GRID = (ICE_CM, 2000.0, 90.1, 180.0, 0.7)  # after the depth: ice, height step, angle grid
ROWS, COLS = 49, 129


@pytest.fixture(scope="module")
def firn():
    from airiceraytracing_amd import Firn
    return Firn.summit()


@pytest.fixture(scope="module")
def solver():
    """A solver whose medium carries the Summit A_ice (B_ice / C_ice: the defaults, ignored)."""
    from airiceraytracing_amd import AirIceSolver
    s = AirIceSolver()
    s.medium = fc.lib_medium(s.medium)
    return s


@pytest.fixture(scope="module")
def upper_solver():
    """(A, B[0], C[0]) as a one-layer medium."""
    from airiceraytracing_amd import AirIceSolver
    s = AirIceSolver()
    s.medium = fc.lib_medium(s.medium, B=fc.SUMMIT_B[0], C=fc.SUMMIT_C[0])
    return s


@pytest.fixture(autouse=True)
def empty_air_cache():
    """Every test starts with no unpinned air record or key."""
    from airiceraytracing_amd import _lib
    st = _lib.air_cache_stats()
    _lib.air_cache_limits(total_bytes=0)
    _lib.air_cache_limits(st["entry_limit"], st["total_limit"])
    yield
    _lib.air_cache_limits(st["entry_limit"], st["total_limit"])


def _grid(depth_m):
    from airiceraytracing_amd import make_grid
    g = make_grid(depth_m * 100.0, *GRID)
    assert (g.table_rows, g.angle_steps) == (ROWS, COLS)
    return g


def _bits(t):
    import torch
    return t.view(torch.int32)


def _build(s, g, firn=None, full=False, **kw):
    import torch
    n = kw.get("row_count", g.table_rows) * g.angle_steps
    t = torch.full((11, n), float("nan"), dtype=torch.float32, device="cuda:0")
    f = torch.full((18, n), float("nan"), dtype=torch.float64, device="cuda:0") if full else None
    s.table_device(g, t, f, firn=firn, **kw)
    torch.cuda.synchronize()
    return (t, f) if full else t


@pytest.fixture(scope="module")
def cold_100(solver, firn):
    """The layered table at -100 m built with the air-record cache off: every build is cold."""
    from airiceraytracing_amd import _lib
    st = _lib.air_cache_stats()
    _lib.air_cache_limits(0, 0)
    t = _build(solver, _grid(-100.0), firn)
    _lib.air_cache_limits(st["entry_limit"], st["total_limit"])
    return t


def test_full_output(solver, firn, oracle_medium):
    """Depth -100 m with d_full: all 18 doubles of every ray against the composition, the float
    table within 1 ulp of it, the same NaNs."""
    from airiceraytracing_amd import _lib
    g = _grid(-100.0)
    with _lib.launched("table_kernel") as k:
        t, f = _build(solver, g, firn, full=True)
    assert k.count == 1
    ref_t, ref_f = fc.compose_table(oracle_medium, -10000.0, *GRID)
    got_t, got_f = t.cpu().numpy(), f.cpu().numpy()
    rep = parity.compare_columns(got_f, ref_f, parity.RAY_FLOORS)
    print(f"[firn table] {g.n_rays} rays: max_rel={rep['max_rel']:.3e} "
          f"per column {['%.1e' % v for v in rep['max_rel_per_col']]}")
    assert rep["ok"], rep
    assert np.array_equal(np.isnan(got_t), np.isnan(ref_t))
    ulp = parity.float_ulp_diff(got_t, ref_t)
    print(f"[firn table] float table: {ulp} ulp")
    assert ulp <= 1
    assert np.isnan(got_t).any() and not np.isnan(got_t[[2, 9, 10]]).all()


def test_cold_warm_reuse(solver, firn, cold_100):
    """Three builds of one grid (key, fill, warm) are one table; a second depth on the same grid
    reads the same air record and equals its own cold build."""
    import torch
    from airiceraytracing_amd import _lib
    g = _grid(-100.0)
    before = _lib.air_cache_stats()
    tabs, fills, filled = [], [], []
    for _ in range(3):
        with _lib.launched("air_part_kernel") as f, _lib.launched("table_kernel") as k:
            tabs.append(_build(solver, g, firn))
        assert k.count == 1
        fills.append(f.count)
        filled.append(_lib.air_cache_stats()["filled"] - before["filled"])
    assert fills == [0, 1, 0], fills        # the air part is traced once, at the second build
    assert filled == [0, 1, 1], filled      # and the third build read it: the warm kernel
    for t in tabs:
        assert torch.equal(_bits(t), _bits(cold_100))
    # a second depth: no new key, no new fill -- warm at once
    g40 = _grid(-40.0)
    with _lib.launched("air_part_kernel") as f:
        warm40 = _build(solver, g40, firn)
    assert f.count == 0 and _lib.air_cache_stats()["keys"] - before["keys"] == 1
    st = _lib.air_cache_stats()
    _lib.air_cache_limits(0, 0)
    cold40 = _build(solver, g40, firn)
    _lib.air_cache_limits(st["entry_limit"], st["total_limit"])
    assert torch.equal(_bits(warm40), _bits(cold40))
    assert not torch.equal(_bits(warm40), _bits(cold_100))


def test_no_cache_crossing(solver, firn, cold_100):
    """A one-layer table (the default ice model) of the same grid keeps its own air record: it is
    the same before and after the layered builds, and the layered table after it."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib
    plain = AirIceSolver()
    g = _grid(-100.0)
    before = [_build(plain, g) for _ in range(3)]
    keys0 = _lib.air_cache_stats()["keys"]
    layered = [_build(solver, g, firn) for _ in range(3)]
    assert _lib.air_cache_stats()["keys"] == keys0 + 1  # the Summit launch has a key of its own
    after = [_build(plain, g) for _ in range(3)]
    for t in before + after:
        assert torch.equal(_bits(t), _bits(before[0]))
    again = _build(solver, g, firn)
    for t in layered + [again]:
        assert torch.equal(_bits(t), _bits(cold_100))
    assert not torch.equal(_bits(before[0]), _bits(cold_100))


def test_multi_antenna(solver, upper_solver, firn):
    """-5, -14.9, -15 and -150 m in one launch: each table is its single launch's, the first two
    the one-layer build's with (A, B[0], C[0])."""
    import torch
    from airiceraytracing_amd import _lib
    depths = (-5.0, -14.9, -15.0, -150.0)
    grids = [_grid(d) for d in depths]
    tabs = [torch.full((11, g.n_rays), float("nan"), dtype=torch.float32, device="cuda:0")
            for g in grids]
    with _lib.launched("table_kernel") as k:
        solver.tables_device(grids, tabs, firn=firn)
    torch.cuda.synchronize()
    assert k.count == 1
    for d, g, t in zip(depths, grids, tabs):
        assert torch.equal(_bits(t), _bits(_build(solver, g, firn))), d
    for g, t in zip(grids[:2], tabs[:2]):
        assert torch.equal(_bits(t), _bits(_build(upper_solver, g)))
    assert not torch.equal(_bits(tabs[2]), _bits(_build(upper_solver, grids[2])))


def test_row_slab(solver, firn, cold_100):
    g = _grid(-100.0)
    slab = _build(solver, g, firn, row_begin=7, row_count=5)
    assert slab.shape[1] == 5 * COLS
    import torch
    assert torch.equal(_bits(slab), _bits(cold_100[:, 7 * COLS:12 * COLS].contiguous()))


def test_rays(solver, firn):
    """airice_rays_launch_firn with n = 1, 2 and 1,000 against airice_rays_host_firn; the one-ray
    launch is the same ray inside the batch, bit for bit."""
    import torch
    from airiceraytracing_amd import _lib
    launch, txh, _ = fc.draw(1000, seed=99)
    host = solver.rays_host(launch, txh, fc.ICE_M, -100.0, True, firn=firn)
    d_launch, d_txh = (torch.from_numpy(a).cuda() for a in (launch, txh))
    outs = {}
    for n in (1, 2, 1000):
        out = torch.full((18, n), float("nan"), dtype=torch.float64, device="cuda:0")
        with _lib.launched("rays_kernel") as k:
            solver.rays_device(d_launch[:n].contiguous(), d_txh[:n].contiguous(), fc.ICE_M, -100.0,
                               True, out, firn=firn)
        torch.cuda.synchronize()
        assert k.count == 1
        outs[n] = out.cpu().numpy()
        rep = parity.compare_columns(outs[n], host[:, :n], parity.RAY_FLOORS)
        print(f"[firn rays] n={n}: max_rel={rep['max_rel']:.3e}")
        assert rep["ok"], (n, rep)
    assert np.array_equal(outs[1].view(np.uint64), outs[1000][:, :1].view(np.uint64))
    assert np.array_equal(outs[2].view(np.uint64), outs[1000][:, :2].view(np.uint64))


def test_python(solver, firn, cold_100):
    """table_device(firn=) and antenna_tables(firn=) build the C calls' bits; lookup answers the
    AIRICE_LOOKUP_FALLBACK lanes with NaN / ok = 0 and leaves every other lane as the lookup
    gave it."""
    import torch
    from airiceraytracing_amd import AntennaTables, _lib
    g = _grid(-100.0)
    t = torch.full((11, g.n_rays), float("nan"), dtype=torch.float32, device="cuda:0")
    _lib.check(_lib.lib().airice_table_launch_firn(
        ctypes.byref(solver.medium), ctypes.byref(firn), ctypes.byref(g), 0, g.table_rows,
        _lib.ptr(t), None, g.n_rays, None), "airice_table_launch_firn")
    torch.cuda.synchronize()
    assert torch.equal(_bits(t), _bits(cold_100))
    assert torch.equal(_bits(_build(solver, g, firn)), _bits(t))
    at = solver.antenna_tables([-10000.0, -500.0, -10000.0], ICE_CM, *GRID[1:], firn=firn)
    torch.cuda.synchronize()
    assert at.firn is firn and at.antenna_table == [0, 1, 0]
    assert torch.equal(_bits(at.buffers[0]), _bits(cold_100))
    src_cm, dist_cm = parity.lookup_queries(cold_100.cpu().numpy(), 512)
    d_src = torch.from_numpy(src_cm).cuda()
    d_dist = torch.from_numpy(np.stack([dist_cm] * 3)).cuda()
    out, ok, fl = at.lookup(d_src, d_dist)
    raw = AntennaTables(solver, ICE_CM, at.grids, at.buffers, at.tables, at.antenna_table,
                        at.depths_cm).lookup(d_src, d_dist)
    torch.cuda.synchronize()
    fb = (fl & _lib.LOOKUP_FALLBACK) != 0
    print(f"[firn lookup] {int(fb.sum())} fallback lanes of {fb.numel()}")
    assert fb.any() and not fb.all()
    assert torch.equal(fl, raw[2])
    assert torch.isnan(out[:, fb]).all() and (ok[fb] == 0).all()
    keep = ~fb
    assert torch.equal(out[:, keep].view(torch.int64), raw[0][:, keep].view(torch.int64))
    assert torch.equal(ok[keep], raw[1][keep])


def test_cpp_make_ray_tracing_tables_layered(tmp_path, cold_100):
    """MultiRayAirIceRefraction::MakeRayTracingTablesLayered through a C++ caller
    (tests/cpp/multiray_layered_driver.cpp): the -100 m table is airice_table_launch_firn's, the
    -5 m table the one-layer MakeRayTracingTable's with (A, B[0], C[0])."""
    import gzip
    import json
    import os
    import subprocess
    from tests.conftest import ATMOSPHERE_GZ, ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "multiray_layered_driver")
    assert os.path.exists(exe), "built by `make -C airiceraytracing_amd/csrc layered_driver`"
    out = tmp_path / "table.f32"
    with open(ATMOSPHERE_GZ, "rb") as f:  # the drop-in reads Atmosphere.dat from its directory
        (tmp_path / "Atmosphere.dat").write_bytes(gzip.decompress(f.read()))
    run = subprocess.run([exe, str(out)], capture_output=True, text=True, cwd=tmp_path,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    rep = json.loads(run.stdout.strip().splitlines()[-1])
    assert rep == {"tables": 3, "entries": ROWS * COLS, "angle_steps": COLS, "height_steps": ROWS,
                   "shallow_equals_one_layer": 1}
    got = np.fromfile(out, dtype=np.float32).reshape(11, ROWS * COLS)
    assert np.array_equal(got.view(np.int32), cold_100.cpu().numpy().view(np.int32))
