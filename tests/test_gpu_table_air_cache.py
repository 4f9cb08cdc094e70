"""The table launch's air record (air_part_kernel, the warm table_kernel): from its third build on,
an 11-column table of a launch seen before reads every ray's air part from a per-launch device
record and traces the ice segment only.  Such a table is bit for bit the cold one, for every
antenna depth over the grid; the record's cache follows the row / sine caches' life cycle (key,
fill, read; pinned under graph capture) inside its own byte limits."""
import numpy as np
import pytest

import oracle
from tests import parity

pytestmark = pytest.mark.gpu

# table column c is the f32 cast of dummy[RAY_COLUMN[c]] (.cc:2101-2111)
RAY_COLUMN = [1, 2, 7, 6, 11, 3, 14, 15, 16, 17, 13]


@pytest.fixture(autouse=True)
def empty_air_cache():
    """Every test starts with no unpinned air record or key (switching the cache off forgets
    them), so the key and fill counts below do not depend on what ran before."""
    from airiceraytracing_amd import _lib
    st = _lib.air_cache_stats()
    _lib.air_cache_limits(total_bytes=0)
    _lib.air_cache_limits(st["entry_limit"], st["total_limit"])
    yield


def _bits(t):
    import torch
    return t.view(torch.int32)


def _build(s, g, **kw):
    import torch
    n = kw.get("row_count", g.table_rows) * g.angle_steps
    t = torch.full((11, n), float("nan"), dtype=torch.float32, device="cuda:0")
    s.table_device(g, t, **kw)
    return t


def _per_lane(s, g, row_begin=0, row_count=None):
    """The table rays_kernel gives: launch angle and Tx height of every entry from one 18-double
    build (a launch that never touches the air record), traced per lane, cast as the table is."""
    import torch
    rows = g.table_rows - row_begin if row_count is None else row_count
    n = rows * g.angle_steps
    t = torch.empty((11, n), dtype=torch.float32, device="cuda:0")
    full = torch.empty((18, n), dtype=torch.float64, device="cuda:0")
    s.table_device(g, t, full, row_begin=row_begin, row_count=rows)
    rays = torch.empty((18, n), dtype=torch.float64, device="cuda:0")
    s.rays_device(full[11].contiguous(), full[1].contiguous(), g.stop_height, g.depth_m,
                  bool(g.in_ice), rays)
    torch.cuda.synchronize()
    return rays[RAY_COLUMN].to(torch.float32)


LIFE_CYCLE_GRIDS = {
    "500m_x_2deg": (-20000.0, 300000.0, 500.0, 92.0, 180.0, 2.0),        # 195 x 45 = 8,775 rays
    "20_rows_x_900": (-20000.0, 300000.0, 5105.0, 90.1, 180.0, 0.1),     # more columns than a block
    "3_columns": (-20000.0, 300000.0, 100.0, 178.0, 180.0, 1.0),         # 971 x 3, 86 rows a block
    "under_a_wave": (-20000.0, 300000.0, 20000.0, 170.0, 180.0, 2.0),    # 5 x 6 = 30 rays
    "4_blocks_and_1": (-20000.0, 300000.0, 4000.0, 100.0, 180.0, 2.0),   # 25 x 41 = 1,025 rays
}


@pytest.mark.parametrize("name", list(LIFE_CYCLE_GRIDS))
def test_key_fill_read_builds_are_one_table(name, oracle_medium):
    """Three builds of one grid -- key only, fill, read -- give identical bits; the first is within
    1 f32 ulp of the oracle with the same NaNs; the third has the per-lane rays' NaN positions and
    their bits everywhere else (every bit: test_warm_table_is_the_per_lane_rays_table).
    Every grid ends with the Tx-on-the-ice row (no air layer); the 90.1-degree grid has the NaN
    columns."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    args = LIFE_CYCLE_GRIDS[name]
    s = AirIceSolver()
    g = make_grid(*args)
    shape = {"500m_x_2deg": (195, 45), "20_rows_x_900": (20, 900), "3_columns": (971, 3),
             "under_a_wave": (5, 6), "4_blocks_and_1": (25, 41)}[name]
    assert (g.table_rows, g.angle_steps) == shape
    assert g.height_steps == g.table_rows  # the last row is the forced Tx = ice height one
    before = _lib.air_cache_stats()
    tabs, fills, warm = [], [], []
    for _ in range(3):
        with _lib.launched("air_part_kernel") as f, _lib.launched("table_kernel") as k:
            tabs.append(_build(s, g))
        torch.cuda.synchronize()
        assert k.count == 1
        fills.append(f.count)
        warm.append(_lib.air_cache_stats())
    assert fills == [0, 1, 0], fills
    assert [w["keys"] - before["keys"] for w in warm] == [1, 1, 1], (before, warm)
    assert [w["filled"] - before["filled"] for w in warm] == [0, 1, 1], (before, warm)
    assert warm[1]["bytes"] - before["bytes"] == 32 * g.n_rays
    assert torch.equal(_bits(tabs[0]), _bits(tabs[1]))
    assert torch.equal(_bits(tabs[0]), _bits(tabs[2]))
    ref = oracle.table_rows(oracle_medium, oracle.grid_init(*args), 0, g.table_rows)
    got = tabs[0].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert parity.float_ulp_diff(got, ref) <= 1
    if name == "20_rows_x_900":
        assert np.isnan(got).any() and not np.isnan(got).all()
    assert got[0, -1] == np.float32(g.stop_height)  # the last row: Tx on the ice
    lanes = _per_lane(s, g)
    assert torch.equal(torch.isnan(tabs[2]), torch.isnan(lanes))
    assert torch.equal(_bits(torch.nan_to_num(tabs[2], nan=0.0)),
                       _bits(torch.nan_to_num(lanes, nan=0.0)))


@pytest.mark.parametrize("name", list(LIFE_CYCLE_GRIDS))
def test_warm_table_is_the_per_lane_rays_table(name):
    """The third (warm) build equals, bit for bit, the f32 casts of rays_device's 18 doubles in the
    table's column mapping -- NaNs included: on the 90.1-degree grid the air sums of the steepest
    rays are NaN, and ray_air_part hands every kernel the same NaN for them (before it did, the
    table kernel stored 0xffc00000 as geo_air where the rays' doubles cast to 0x7fc00000, in 33 of
    that grid's 198,000 entries)."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    s = AirIceSolver()
    g = make_grid(*LIFE_CYCLE_GRIDS[name])
    for _ in range(3):
        with _lib.launched("air_part_kernel") as f:
            t = _build(s, g)
        torch.cuda.synchronize()
    assert f.count == 0 and _lib.air_cache_stats()["filled"] >= 1
    assert torch.equal(_bits(t), _bits(_per_lane(s, g)))


def test_depths_of_one_grid_share_one_air_record():
    """Three new in-ice depths over one grid: ONE air key, ONE fill (at the second depth); every
    table is the per-lane rays' table.  Then an antenna in the air (its grid stops higher: its own
    key), a second ice height, and the two solver variants built alternately: all bit for bit the
    per-lane tables, cold, filling and warm.  (The table launch folds either variant's medium with
    MultiRay's pi -- MakeRayTracingTable is MultiRay's -- so the two variants share ONE key.)"""
    import torch
    from airiceraytracing_amd import AirIceSolver, VARIANT_MULTIRAY, VARIANT_PYWRAPPER, _lib, make_grid
    s = AirIceSolver()
    before = _lib.air_cache_stats()
    with _lib.launched("air_part_kernel") as f:
        for d in (-23100.0, -41700.0, -8800.0):
            g = make_grid(d, 300000.0, 131.0, 91.35, 180.0, 1.3)
            assert torch.equal(_bits(_build(s, g)), _bits(_per_lane(s, g))), d
    after = _lib.air_cache_stats()
    assert f.count == 1
    assert after["keys"] - before["keys"] == 1, (before, after)
    assert after["filled"] - before["filled"] == 1, (before, after)
    for args in ((5000.0, 300000.0, 131.0, 91.35, 180.0, 1.3),     # in the air: in_ice = 0
                 (-23100.0, 310000.0, 131.0, 91.35, 180.0, 1.3)):  # ice at 3,100 m
        g = make_grid(*args)
        assert g.in_ice == (args[0] < 0)
        want = _per_lane(s, g)
        for rep in range(3):
            assert torch.equal(_bits(_build(s, g)), _bits(want)), (args, rep)
    g = make_grid(-23100.0, 300000.0, 171.0, 91.35, 180.0, 1.3)
    solvers = [AirIceSolver(variant=v) for v in (VARIANT_MULTIRAY, VARIANT_PYWRAPPER)]
    want = [_per_lane(sv, g) for sv in solvers]
    k0 = _lib.air_cache_stats()["keys"]
    for rep in range(3):
        for sv, w in zip(solvers, want):
            assert torch.equal(_bits(_build(sv, g)), _bits(w)), rep
    assert _lib.air_cache_stats()["keys"] - k0 == 1


def test_row_slab_with_padded_stride():
    """A row_begin / row_count slab with ld > its rays, built three times: each time the matching
    part of the whole table (itself warm by then), the padding untouched; the slab has its own key."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    s = AirIceSolver()
    g = make_grid(-20000.0, 300000.0, 300.0, 91.1, 180.0, 0.7)
    whole = [_build(s, g) for _ in range(3)][2]
    begin, count = 37, 101
    assert begin + count < g.table_rows
    n, first = count * g.angle_steps, begin * g.angle_steps
    k0 = _lib.air_cache_stats()["keys"]
    for rep in range(3):
        slab = torch.full((11, n + 53), -7.0, dtype=torch.float32, device="cuda:0")
        s.table_device(g, slab, None, row_begin=begin, row_count=count, ld=slab.shape[1])
        torch.cuda.synchronize()
        assert torch.equal(_bits(slab[:, :n]), _bits(whole[:, first:first + n])), rep
        assert bool((slab[:, n:] == -7.0).all()), rep
    assert _lib.air_cache_stats()["keys"] - k0 == 1
    # the last rows too (the Tx-on-the-ice row is the slab's last)
    begin = g.table_rows - 3
    for rep in range(3):
        slab = _build(s, g, row_begin=begin, row_count=3)
        torch.cuda.synchronize()
        assert torch.equal(_bits(slab), _bits(whole[:, begin * g.angle_steps:])), rep


def test_captured_launches_pin_or_fall_back():
    """Under graph capture a launch whose air record is filled reads it and pins it; one whose
    record is not filled runs the cold kernel.  Replays give the uncaptured tables bit for bit,
    also after enough new grids to evict every unpinned entry."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    s = AirIceSolver()
    g_hot = make_grid(-20000.0, 300000.0, 110.0, 92.3, 180.0, 1.1)
    g_new = make_grid(-17000.0, 300000.0, 95.0, 91.2, 180.0, 0.9)  # not built before
    for _ in range(3):
        want_hot = _build(s, g_hot)
        torch.cuda.synchronize()
    t_hot = torch.full_like(want_hot, float("nan"))
    t_new = torch.full((11, g_new.n_rays), float("nan"), dtype=torch.float32, device="cuda:0")
    before = _lib.air_cache_stats()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with _lib.launched("air_part_kernel") as f:
                s.table_device(g_hot, t_hot, stream=side)
                s.table_device(g_new, t_new, stream=side)
    torch.cuda.synchronize()
    after = _lib.air_cache_stats()
    assert f.count == 0
    assert after["pinned"] - before["pinned"] == 1, (before, after)
    assert after["keys"] == before["keys"] and after["filled"] == before["filled"], (before, after)
    graph.replay()
    torch.cuda.synchronize()
    want_new = _build(s, g_new)  # uncaptured, after the capture: its key is new only now
    torch.cuda.synchronize()
    assert _lib.air_cache_stats()["keys"] == after["keys"] + 1
    assert torch.equal(_bits(t_hot), _bits(want_hot))
    assert torch.equal(_bits(t_new), _bits(want_new))
    # 70 new small grids, each built twice (key, then fill): every unpinned entry is evicted
    for a in range(70):
        ga = make_grid(-20000.0, 300000.0 + a + 1, 5100.0, 92.5 + 1e-6 * (a + 1), 180.0, 7.0)
        _build(s, ga)
        _build(s, ga)
    torch.cuda.synchronize()
    st = _lib.air_cache_stats()
    assert st["keys"] <= 64 + st["pinned"], st
    assert st["pinned"] == after["pinned"], st
    t_hot.fill_(float("nan"))
    t_new.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(t_hot), _bits(want_hot))
    assert torch.equal(_bits(t_new), _bits(want_new))


def test_two_streams_read_a_record_filled_on_a_third():
    """The fill is enqueued on one stream; two other streams build two more depths of the grid
    right behind it (no host synchronisation in between): they wait on the fill's event."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    s = AirIceSolver()
    args = (300000.0, 60.0, 91.4, 180.0, 0.6)
    grids = [make_grid(d, *args) for d in (-15000.0, -26000.0, -37000.0, -48000.0)]
    want = [_per_lane(s, g) for g in grids]
    tabs = [torch.full((11, g.n_rays), float("nan"), dtype=torch.float32, device="cuda:0")
            for g in grids]
    st = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    with _lib.launched("air_part_kernel") as f:
        s.table_device(grids[0], tabs[0], stream=st[0])  # key
        s.table_device(grids[1], tabs[1], stream=st[0])  # fill, ahead of this table on st[0]
        s.table_device(grids[2], tabs[2], stream=st[1])
        s.table_device(grids[3], tabs[3], stream=st[2])
    torch.cuda.synchronize()
    assert f.count == 1
    for t, w in zip(tabs, want):
        assert torch.equal(_bits(t), _bits(w))


def test_limits_and_switching_the_cache_off():
    """A launch whose record is above the per-record limit is never cached -- no key, no fill, the
    same table --; lowering the total frees records down to it; with the total at 0 every launch
    is the cold one.  The limits are put back as they were."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    s = AirIceSolver()
    g = make_grid(-20000.0, 300000.0, 210.0, 92.6, 180.0, 1.4)
    want = _per_lane(s, g)
    st0 = _lib.air_cache_stats()
    assert st0["entry_limit"] >= 32 * 8_730_000 and st0["total_limit"] >= st0["entry_limit"]
    try:
        _lib.air_cache_limits(entry_bytes=32 * g.n_rays - 1)
        with _lib.launched("air_part_kernel") as f:
            for rep in range(3):
                assert torch.equal(_bits(_build(s, g)), _bits(want)), rep
        st = _lib.air_cache_stats()
        assert f.count == 0
        assert (st["keys"], st["filled"], st["bytes"]) == (st0["keys"], st0["filled"], st0["bytes"])
        _lib.air_cache_limits(entry_bytes=32 * g.n_rays)  # exactly fits
        with _lib.launched("air_part_kernel") as f:
            for rep in range(3):
                assert torch.equal(_bits(_build(s, g)), _bits(want)), rep
        st = _lib.air_cache_stats()
        assert f.count == 1 and st["bytes"] >= 32 * g.n_rays  # filled once, then read
        _lib.air_cache_limits(total_bytes=0)  # off: the unpinned records go, pinned ones stay
        off = _lib.air_cache_stats()
        assert off["keys"] == off["filled"] == off["pinned"] and off["total_limit"] == 0, off
        with _lib.launched("air_part_kernel") as f:
            for rep in range(3):
                assert torch.equal(_bits(_build(s, g)), _bits(want)), rep
        assert f.count == 0
        assert _lib.air_cache_stats()["filled"] == off["filled"]
    finally:
        _lib.air_cache_limits(st0["entry_limit"], st0["total_limit"])
    end = _lib.air_cache_stats()
    assert (end["entry_limit"], end["total_limit"]) == (st0["entry_limit"], st0["total_limit"])
