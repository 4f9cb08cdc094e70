"""The warm table kernel's record layout and store order: the air record is two planes of 16-byte
entries (double2 {vinc, thd_air}, then float4 {col3, col8, col6, col7}) read with two 16-byte
loads per lane ahead of the block's barrier, and the seven columns that need nothing from the ice
segment (0, 3, 4, 5, 6, 7, 8) are stored before it is traced, columns 1, 2, 9 and 10 after it.
Every case makes the three builds of a launch -- key, fill, read -- into a table pre-filled with a
sentinel bit pattern whose column stride is larger than its rays, and asks that the third build is
bit for bit the first and the per-lane rays' table, and that no float past the rays was written.

Shapes: the smallest at which the layout and the store order can go wrong -- one ray, a partial
wave, one ray either side of a wave and of a block, more than one block, a count above 2,048 that
is no multiple of 8 (the float plane then starts off a 128-byte line), one column (every lane a new
row), more columns than a block has lanes (with the 90.1-degree grid's NaN air sums), row slabs
with row_begin > 0, strides n + 3 and n + 64."""
import pytest

from tests.test_gpu_table_air_cache import _bits, _per_lane, empty_air_cache  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5AA5A5  # as a float 1.5387e16: no table entry

ONE_COLUMN = (-20000.0, 300000.0, 100.0, 180.0, 180.0, 1.0)       # 971 x 1
UNDER_A_WAVE = (-20000.0, 300000.0, 20000.0, 170.0, 180.0, 2.0)   # 5 x 6 = 30 rays
FOUR_BLOCKS_AND_1 = (-20000.0, 300000.0, 4000.0, 100.0, 180.0, 2.0)  # 25 x 41 = 1,025 rays
THREE_COLUMNS = (-20000.0, 300000.0, 100.0, 178.0, 180.0, 1.0)    # 971 x 3 = 2,913 rays
WIDE_ROWS = (-20000.0, 300000.0, 5105.0, 90.1, 180.0, 0.1)        # 20 x 900, NaN air sums

# name: (grid, row_begin, row_count or None for the whole grid, rays, stride - rays)
CASES = {
    "1_ray": (ONE_COLUMN, 5, 1, 1, 3),
    "30_rays": (UNDER_A_WAVE, 0, None, 30, 64),
    "63_rays": (ONE_COLUMN, 7, 63, 63, 3),
    "64_rays": (ONE_COLUMN, 7, 64, 64, 64),
    "65_rays": (ONE_COLUMN, 7, 65, 65, 3),
    "255_rays": (ONE_COLUMN, 11, 255, 255, 64),
    "256_rays": (ONE_COLUMN, 11, 256, 256, 3),
    "257_rays": (ONE_COLUMN, 700, 257, 257, 64),
    "1025_rays": (FOUR_BLOCKS_AND_1, 0, None, 1025, 3),
    "2913_rays": (THREE_COLUMNS, 0, None, 2913, 64),
    "3_columns_slab": (THREE_COLUMNS, 201, 683, 2049, 3),
    "900_columns": (WIDE_ROWS, 0, None, 18000, 3),
    "900_columns_slab": (WIDE_ROWS, 3, 2, 1800, 64),
}


def _sentinel_table(ld):
    import torch
    return torch.full((11, ld), SENTINEL, dtype=torch.int32, device="cuda:0").view(torch.float32)


def _build(s, g, n, pad, row_begin=0, row_count=None, stream=None):
    """One build into a sentinel-filled table of stride n + pad; returns the whole tensor."""
    t = _sentinel_table(n + pad)
    s.table_device(g, t, None, row_begin=row_begin, row_count=row_count, ld=n + pad, stream=stream)
    return t


def _padding_untouched(t, n):
    return bool((_bits(t[:, n:]) == SENTINEL).all())


@pytest.mark.parametrize("name", list(CASES))
def test_key_fill_read_builds_with_padded_stride(name):
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    args, begin, count, n, pad = CASES[name]
    s = AirIceSolver()
    g = make_grid(*args)
    rows = g.table_rows - begin if count is None else count
    assert rows * g.angle_steps == n, (g.table_rows, g.angle_steps)
    assert begin + rows <= g.table_rows
    if args is ONE_COLUMN:
        assert g.angle_steps == 1
    if args is WIDE_ROWS:
        assert g.angle_steps > 256
    before = _lib.air_cache_stats()
    tabs, fills, stats = [], [], []
    for _ in range(3):
        with _lib.launched("air_part_kernel") as f, _lib.launched("table_kernel") as k:
            tabs.append(_build(s, g, n, pad, begin, rows))
        torch.cuda.synchronize()
        assert k.count == 1
        assert _padding_untouched(tabs[-1], n)
        fills.append(f.count)
        stats.append(_lib.air_cache_stats())
    assert fills == [0, 1, 0], fills
    assert [w["filled"] - before["filled"] for w in stats] == [0, 1, 1], (before, stats)
    assert stats[1]["bytes"] - before["bytes"] == 32 * n
    assert stats[2]["bytes"] - before["bytes"] == 32 * n
    assert torch.equal(_bits(tabs[0]), _bits(tabs[1]))
    assert torch.equal(_bits(tabs[0]), _bits(tabs[2]))
    lanes = _per_lane(s, g, begin, rows)
    assert torch.equal(_bits(tabs[2][:, :n]), _bits(lanes))
    if name == "900_columns":
        nan = torch.isnan(tabs[2][:, :n])
        assert bool(nan.any()) and not bool(nan.all())
    assert not bool((_bits(tabs[2][:, :n]) == SENTINEL).any())  # every entry was stored


def test_depths_share_the_early_columns():
    """An antenna above the ice (in_ice == 0: nothing is traced behind the early stores) against
    the per-lane rays, then two in-ice depths over one grid reading one record: the seven early
    columns are the record's and the grid's, equal bit for bit between the depths; the four late
    ones come from the ice segment and differ."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    s = AirIceSolver()
    rest = (300000.0, 131.0, 91.35, 180.0, 1.3)
    g_air = make_grid(5000.0, *rest)
    assert g_air.in_ice == 0
    n = g_air.n_rays
    want = _per_lane(s, g_air)
    for rep in range(3):
        t = _build(s, g_air, n, 3)
        torch.cuda.synchronize()
        assert torch.equal(_bits(t[:, :n]), _bits(want)), rep
        assert _padding_untouched(t, n), rep
    shallow, deep = make_grid(-8800.0, *rest), make_grid(-41700.0, *rest)
    assert shallow.in_ice == 1 and deep.in_ice == 1 and shallow.n_rays == deep.n_rays
    n = shallow.n_rays
    before = _lib.air_cache_stats()
    with _lib.launched("air_part_kernel") as f:
        _build(s, shallow, n, 64)            # key
        _build(s, deep, n, 64)               # fill
        t_shallow = _build(s, shallow, n, 64)  # read
        t_deep = _build(s, deep, n, 64)        # read
    torch.cuda.synchronize()
    after = _lib.air_cache_stats()
    assert f.count == 1
    assert after["keys"] - before["keys"] == 1 and after["filled"] - before["filled"] == 1
    assert after["bytes"] - before["bytes"] == 32 * n
    for g, t in ((shallow, t_shallow), (deep, t_deep)):
        assert torch.equal(_bits(t[:, :n]), _bits(_per_lane(s, g)))
        assert _padding_untouched(t, n)
    for c in (0, 3, 4, 5, 6, 7, 8):
        assert torch.equal(_bits(t_shallow[c, :n]), _bits(t_deep[c, :n])), c
    for c in (1, 2, 9, 10):
        assert not torch.equal(_bits(t_shallow[c, :n]), _bits(t_deep[c, :n])), c


def test_warm_build_on_a_second_stream_behind_the_fill():
    """The record is filled on one stream; a second stream builds another depth of the grid right
    behind it with no host synchronisation in between: its record loads, now ahead of the block's
    barrier, still run behind the fill's event."""
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib, make_grid
    s = AirIceSolver()
    rest = (300000.0, 60.0, 91.4, 180.0, 0.6)
    grids = [make_grid(d, *rest) for d in (-15000.0, -26000.0, -37000.0)]
    n = grids[0].n_rays
    want = [_per_lane(s, g) for g in grids]
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with _lib.launched("air_part_kernel") as f:
        tabs = [_build(s, grids[0], n, 3, stream=first),    # key
                _build(s, grids[1], n, 3, stream=first),    # fill, ahead of this table
                _build(s, grids[2], n, 3, stream=second)]   # read, behind the fill's event
    torch.cuda.synchronize()
    assert f.count == 1
    for t, w in zip(tabs, want):
        assert torch.equal(_bits(t[:, :n]), _bits(w))
        assert _padding_untouched(t, n)
