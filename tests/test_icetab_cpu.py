"""The in-ice interpolation tables without a GPU: header and exports, the grid helpers, the pack
rule and the host lookup bit for bit against the numpy restatement (tests/icetab_cases.py), the
image round trip, the argument checks, and the drop-in's SetTable / GetInterpolatedValue through
its own driver, plain and under ASan + UBSan."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import icetab_cases as cases
from tests.conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "cpp", "icetab_driver")
DRIVER_ASAN = os.path.join(ROOT, "tests", "cpp", "icetab_driver_asan")


@pytest.fixture(scope="module")
def synthetic():
    """The synthetic image (aligned for the library), its descriptors and column values, and the
    edge queries with the restatement's answers, computed once."""
    from airiceraytracing_amd import _lib
    plain, descs, values = cases.synthetic_image()
    image = _lib.aligned_doubles(plain.size)
    image[:] = plain
    q = cases.edge_queries()
    ref, ref_st = cases.lookup_ref_batch(plain, len(descs), q)
    for a in (image, descs, q, ref, ref_st, *values):
        a.setflags(write=False)
    return image, descs, values, q, ref, ref_st


def _lookup(image, n_ant, q):
    from airiceraytracing_amd import solver
    out, st = solver.icetab_lookup_host(image, n_ant, q[:, 1], q[:, 2], q[:, 0].astype(np.int32))
    return out.T.copy(), st.astype(np.int64)


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import AirIceSolver, IceTables, _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    assert "--- in-ice interpolation tables ---" in header
    for name in ("grid_init", "grid", "layout", "pack_host", "work_bytes", "build_launch",
                 "build_host", "lookup_launch", "lookup_host"):
        assert f"int airice_icetab_{name}(" in header, name
        assert f"airice_icetab_{name}" in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), f"airice_icetab_{name}")
    for macro in ("AIRICE_ICETAB_DESC 8", "AIRICE_ICETAB_RECORD 16", "AIRICE_ICETAB_PARAMS 13",
                  "AIRICE_ICETAB_CELL 1", "AIRICE_ICETAB_IDW 2", "AIRICE_ICETAB_BAD_ANTENNA 4"):
        assert f"#define {macro}" in header, macro
    for kernel in ("icetab_points_kernel", "icetab_pack_kernel", "icetab_lookup_kernel"):
        assert _lib.launch_count(kernel) >= 0
        assert _lib.kernel_time(kernel, reset=False) == (0.0, 0)
    with open(os.path.join(ROOT, "include", "IceRayTracing.hh")) as f:
        dropin = f.read()
    for name in ("SetNumberOfAntennas", "MakeTable", "GetInterpolatedValue", "MakeTables",
                 "GetInterpolatedValues", "GetInterpolatedValuesBatch", "SetTable"):
        assert f"{name}(" in dropin, name
    assert "MakeTable and its" not in dropin
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    for mangled in ("_ZN13IceRayTracing19SetNumberOfAntennasEi", "_ZN13IceRayTracing9MakeTableEdddi",
                    "_ZN13IceRayTracing20GetInterpolatedValueEddii"):
        assert f" T {mangled}\n" in nm, mangled
    assert (_lib.ICETAB_DESC, _lib.ICETAB_RECORD, _lib.ICETAB_PARAMS) == (8, 16, 13)
    assert callable(AirIceSolver.ice_tables) and callable(AirIceSolver.ice_tables_from_values)
    assert callable(IceTables.lookup) and callable(IceTables.lookup_host) and callable(IceTables.values)


@pytest.mark.parametrize("hit", [0.0, 20.0, 20.1, 150.0])
@pytest.mark.parametrize("depth", [-5.0, -10.0, -10.1, -300.0, -10.5])
def test_grid_init_is_the_reference_set_up(hit, depth):
    """airice_icetab_grid_init against the restatement, field for field; -10.5 is a depth with
    |depth| > 10 and depth + 10 >= 0 false, -5 one with depth + 10 >= 0."""
    from airiceraytracing_amd import icetab_grid_init
    got = icetab_grid_init(hit, depth, -37.5)
    want = cases.grid_init_ref(hit, depth, -37.5)
    assert cases.same_bits(got, want), (got, want)
    assert (got[4], got[5]) == (401, 201)
    assert got[0] == (0.0 if hit <= 20 else hit - 20)
    assert got[1] == (-20.0 if (abs(depth) <= 10 or depth + 10 >= 0) else depth - 10)


def test_grid_rejects_what_is_no_grid():
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    d = np.zeros(8)
    ok = dict(xs=0.0, zs=-1.0, dx=0.1, dz=0.1, nx=2, nz=2, rx=-1.0)
    assert L.airice_icetab_grid(*ok.values(), _lib.ptr(d)) == 0
    assert list(d) == [0.0, -1.0, 0.1, 0.1, 2.0, 2.0, 0.0, -1.0]
    for key, bad, word in (("nx", 1, "nx"), ("nz", 1, "nz"), ("nz", -3, "nz"), ("dx", 0.0, "x_step"),
                           ("dx", -0.1, "x_step"), ("dx", math.nan, "x_step"),
                           ("dz", math.inf, "z_step"), ("dz", 0.0, "z_step")):
        a = dict(ok)
        a[key] = bad
        assert L.airice_icetab_grid(*a.values(), _lib.ptr(d)) == -1, (key, bad)
        assert word in L.airice_last_error().decode()
    assert L.airice_icetab_grid(*ok.values(), None) == -1
    assert "desc8" in L.airice_last_error().decode()


def test_layout_is_the_documented_one(synthetic):
    """Header of n_ant x 8 doubles padded to a multiple of 16; records of 16 doubles, antenna after
    antenna; first_record counts records from the image's base."""
    from airiceraytracing_amd import solver
    _, descs, _, *_ = synthetic
    got, size = solver.icetab_descs([g[:6] + (0.0, g[6]) for g in cases.GRIDS])
    assert cases.same_bits(got, descs)
    assert list(got[:, 6]) == [2.0, 2.0 + 20, 2.0 + 20 + 63] and size == 16 * (2 + 20 + 63 + 65)
    for n_ant, header in ((1, 16), (2, 16), (3, 32), (4, 32), (5, 48)):
        d, size = solver.icetab_descs([cases.GRIDS[0][:6] + (0.0, -1.0)] * n_ant)
        assert d[0, 6] == header // 16 and size == header + n_ant * 20 * 16


def _hand_rows():
    """18-column rows and status bytes for the pack: both values of each IgnoreCh, incidence 100
    and not, each focus bit set and clear, a NaN factor with its bit set, a non-finite row."""
    rows, status = [], []
    base = np.array([1e-6, 2e-6, 300.0, 310.0, 60.0, 120.0, 61.0, 121.0, 1, 1, 100.0, 47.5, 0.7,
                     0.6, 1, 2, 1.25, 0.75])
    for ig0 in (0, 1):
        for ig1 in (0, 1):
            for inc in (100.0, 47.5):
                for bits in (0, 8, 16, 24):
                    r = base.copy()
                    r[8], r[9], r[11] = ig0, ig1, inc
                    rows.append(r)
                    status.append(ig0 | 2 * ig1 | bits)
    for k, bit in ((0, 8), (1, 16)):  # a NaN factor whose bit is set becomes 1
        r = base.copy()
        r[16 + k] = np.nan
        rows.append(r)
        status.append(3 | bit)
        rows.append(r.copy())  # and with the bit clear the column is not read at all
        status.append(3)
    r = np.full(18, np.nan)  # what icesol leaves for a non-finite row
    r[[8, 9, 14, 15]] = 0
    rows.append(r)
    status.append(128)
    return np.array(rows), np.array(status, dtype=np.uint8)


def test_pack_is_the_reference_statement_by_statement():
    from airiceraytracing_amd import solver
    rows, status = _hand_rows()
    got = solver.icetab_pack_host(rows.T, status)
    assert got.shape == (len(rows), 16)
    for i in range(len(rows)):
        want = cases.pack_ref(rows[i], int(status[i]))
        assert cases.same_bits(got[i], want), (i, rows[i], status[i])
        assert got[i, 13] == status[i] and got[i, 14] == 0 and got[i, 15] == 0
    assert (got[-1, :13] == -1000).all()          # the non-finite row
    # the factors: 1.0 unless the bit is set, the column's value when it is, 1.0 for a NaN
    full = (rows[:, 8] != 0) & (rows[:, 9] != 0)
    for i in np.nonzero(full)[0]:
        for k, bit in ((0, 8), (1, 16)):
            f = rows[i, 16 + k]
            want = f if (status[i] & bit and not np.isnan(f)) else 1.0
            assert got[i, 5 + 6 * k] == want, (i, k)


def test_lookup_host_is_the_reference_statement_by_statement(synthetic):
    image, descs, values, q, ref, ref_st = synthetic
    got, st = _lookup(image, len(descs), q)
    for i in range(len(q)):
        assert cases.same_bits(got[i], ref[i]), (i, q[i], got[i], ref[i])
    assert np.array_equal(st, ref_st)
    # the cases are all there: every status, all 16 subsets on the slot-0 group, both NaN routes
    assert {0, 1, 3, 4} <= set(st.tolist())
    n_ant = len(descs)
    inside = (st & cases.CELL) != 0
    assert ((got[~inside] == -1000).all())
    nan_q = np.isnan(q[:, 1]) | np.isnan(q[:, 2]) | np.isinf(q[:, 1]) | np.isinf(q[:, 2])
    assert nan_q.sum() == 7 * n_ant and (st[nan_q] == 0).all()
    assert (st[(q[:, 0] < 0) | (q[:, 0] >= n_ant)] == cases.BAD_ANTENNA).all()


def test_holes_take_the_inverse_distance_branch(synthetic):
    """Inside each hole cell: the parameters of the holed slots are the inverse-distance mean of
    the valid corners (-1000 for four missing corners), the other parameters stay bilinear; a
    query on a valid node of a hole cell gives inf/inf and so -1000."""
    image, descs, values, *_ = synthetic
    n_ant = len(descs)
    for a, bx, bz, slots, subset in cases.hole_cells():
        xs, zs, dx, dz = cases.GRIDS[a][:4]
        x = cases.position(xs, dx, bx) + 0.3 * dx
        z = cases.position(zs, dz, bz) + 0.6 * dz
        got, st = _lookup(image, n_ant, np.array([[a, x, z]]))
        want, want_st = cases.lookup_ref(np.asarray(image), n_ant, a, x, z)
        assert cases.same_bits(got[0], want) and st[0] == want_st
        assert st[0] == (cases.CELL | (cases.IDW if subset else 0)), (a, bx, bz)
        slots = list(slots)
        if subset == 0b1111:
            assert (got[0, slots] == -1000).all()
        elif subset:
            corners = [values[a][slots, bx + di, bz + dj] for di, dj in cases.CORNERS]
            valid = [c for k, c in enumerate(corners) if not subset >> k & 1]
            assert (got[0, slots] != -1000).all()
            assert (got[0, slots] >= np.min(valid, axis=0) - 1e-9).all()
            assert (got[0, slots] <= np.max(valid, axis=0) + 1e-9).all()
        if subset not in (0, 0b1111):  # on a valid node of the hole cell
            k = [k for k in range(4) if not subset >> k & 1][0]
            di, dj = cases.CORNERS[k]
            xn, zn = cases.position(xs, dx, bx + di), cases.position(zs, dz, bz + dj)
            if di == 0 and dj == 0:  # the node that floor() assigns to this very cell
                node, nst = _lookup(image, n_ant, np.array([[a, xn, zn]]))
                assert nst[0] == cases.CELL | cases.IDW and (node[0, slots] == -1000).all()


def test_nodes_of_a_hole_free_antenna_return_their_values(synthetic):
    """Antenna 0 has no holes: a query on any node below the upper stops returns that node's 13
    values bit for bit (one bilinear weight is exactly 1, the others exactly 0).  A node on an
    upper stop returns -1000 where floor() gives the last index -- always on antenna 1, whose
    steps are binary fractions; on antenna 0's 0.1 m steps the quotient of a stop can round below
    the index, and then the reference, the restatement and the library read the last cell, whose
    weight at that node is again exactly 1."""
    image, descs, values, *_ = synthetic
    for a in (0, 1):
        xs, zs, dx, dz, nx, nz, _ = cases.GRIDS[a]
        nodes = [(ix, iz) for ix in range(nx) for iz in range(nz)]
        q = np.array([(a, cases.position(xs, dx, ix), cases.position(zs, dz, iz))
                      for ix, iz in nodes])
        got, st = _lookup(image, len(descs), q)
        for i, (ix, iz) in enumerate(nodes):
            below = ix < nx - 1 and iz < nz - 1
            if a == 0 and (below or st[i]):
                assert st[i] == cases.CELL and cases.same_bits(got[i], values[0][:, ix, iz]), (ix, iz)
            elif not below:
                assert st[i] == 0 and (got[i] == -1000).all(), (a, ix, iz)


def test_image_round_trip(synthetic):
    """The package's own assembly of the image from column values is the documented layout, and
    values() gives the columns back bit for bit (the host half of ice_tables_from_values)."""
    from airiceraytracing_amd import solver
    image, descs, values, *_ = synthetic
    mine, d = solver.icetab_image_from_values([g[:6] + (0.0, g[6]) for g in cases.GRIDS], values)
    assert mine.ctypes.data % 128 == 0
    assert cases.same_bits(d, descs) and cases.same_bits(mine, np.asarray(image))
    for a in range(len(descs)):
        back = solver.icetab_values(mine, d, a)
        assert back.shape == values[a].shape and cases.same_bits(back, values[a])


def test_argument_checks_need_no_device(synthetic):
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    image, descs, *_ = synthetic
    p = ctypes.c_void_p(4096)  # aligned, never dereferenced
    odd = ctypes.c_void_p(4096 + 64)
    names = ("icetab_points_kernel", "icetab_pack_kernel", "icetab_lookup_kernel", "iceray_kernel",
             "icesol_kernel")
    counts = [_lib.launch_count(k) for k in names]
    err = lambda: L.airice_last_error().decode()  # noqa: E731

    def look(fn, **kw):
        a = dict(image=p, n_ant=3, ant=None, x=p, z=p, n=8, out=p, ld=8, status=None)
        a.update(kw)
        extra = (None,) if fn is L.airice_icetab_lookup_launch else ()
        return fn(*a.values(), *extra)

    for fn in (L.airice_icetab_lookup_launch, L.airice_icetab_lookup_host):
        assert look(fn, n=0, image=None, x=None, z=None, out=None) == 0
        for name in ("image", "x", "z", "out"):
            assert look(fn, **{name: None}) == -1 and f"({name})" in err(), name
        assert look(fn, image=odd) == -1 and "aligned" in err()
        assert look(fn, ld=7) == -1 and "ld (7)" in err()
        assert look(fn, n_ant=0) == -1 and "n_ant" in err()

    d = np.array(descs)
    size = ctypes.c_size_t(0)
    assert L.airice_icetab_work_bytes(_lib.ptr(d), 3, ctypes.byref(size)) == 0
    positions = 20 + 63 + 65
    assert size.value >= 8 * (4 + 64 + 18) * positions

    def build(**kw):
        a = dict(model=None, image=p, descs=_lib.ptr(d), n_ant=3, a0=1.0, f=0.1, work=p,
                 bytes=size.value, stream=None)
        a.update(kw)
        return L.airice_icetab_build_launch(*a.values())

    for name in ("image", "work", "descs"):
        assert build(**{name: None}) == -1 and f"({name})" in err(), name
    assert build(n_ant=0) == -1 and "n_ant" in err()
    assert build(n_ant=33) == -1 and "n_ant" in err()
    assert build(image=odd) == -1 and "image" in err()
    assert build(bytes=size.value - 1) == -1 and "work_bytes" in err()
    for bad in (math.nan, math.inf):
        assert build(a0=bad) == -1 and "a0" in err()
    for bad in (math.nan, math.inf, 0.0, -0.1):
        assert build(f=bad) == -1 and "frequency_ghz" in err()
    m = np.array((1.78, 0.43, 0.0132))
    assert build(model=_lib.ptr(m)) == -1 and "model3" in err()
    stale = d.copy()
    stale[1, 6] += 1
    assert build(descs=_lib.ptr(stale)) == -1 and "first_record" in err()
    assert L.airice_icetab_build_host(None, odd, _lib.ptr(d), 3, 1.0, 0.1) == -1 and "image" in err()
    assert L.airice_icetab_build_host(None, p, _lib.ptr(d), 3, 1.0, -1.0) == -1
    assert "frequency_ghz" in err()
    assert [_lib.launch_count(k) for k in names] == counts


def _driver_lines(run):
    got = {}
    for line in run.stdout.splitlines():
        tag, key, *words = line.split()
        if tag == "T":
            got.setdefault("T", {})[key] = np.array([int(words[0], 16)], dtype=np.uint64).view(np.float64)[0]
        else:
            got.setdefault(tag, {})[int(key)] = np.array([int(w, 16) for w in words],
                                                         dtype=np.uint64).view(np.float64)
    return got


def test_drop_in_reads_are_the_host_lookup(synthetic, tmp_path):
    """SetNumberOfAntennas, SetTable, GetInterpolatedValues and 13 calls of GetInterpolatedValue
    through the stand-alone driver on the synthetic tables and the edge queries: lookup_host's
    bits.  The driver's antennas are the image's; antenna index 3 and beyond have no table."""
    image, descs, values, q, ref, _ = synthetic
    q = q[np.abs(q[:, 0]) < 100]  # the driver takes AntNum as an int
    words = [float(len(descs))]
    for a in range(len(descs)):
        words += list(descs[a]) + list(values[a].ravel())
    words += [float(len(q))] + list(q.ravel())
    path = os.path.join(str(tmp_path), "tables.bin")
    np.array(words, dtype=np.float64).tofile(path)
    run = subprocess.run([DRIVER, "set", path], capture_output=True, text=True, check=True)
    assert run.stderr == "", run.stderr
    got = _driver_lines(run)
    mine, _ = _lookup(image, len(descs), q)
    assert len(got["V"]) == len(got["G"]) == len(q)
    for i in range(len(q)):
        assert cases.same_bits(got["Q"][i], q[i])
        assert cases.same_bits(got["V"][i], mine[i]), (i, q[i])
        assert cases.same_bits(got["G"][i], mine[i]), (i, q[i])


def _builtin_image():
    """The driver's built-in tables (tests/cpp/icetab_driver.cpp, builtin()) restated."""
    from airiceraytracing_amd import solver
    grids = ((0.0, -20.0, 0.5, 0.25, 5, 4), (10.0, -3.5, 0.25, 0.5, 4, 6))
    descs, values = [], []
    for a, g in enumerate(grids):
        nx, nz = g[4], g[5]
        c, ix, iz = np.meshgrid(np.arange(13.0), np.arange(float(nx)), np.arange(float(nz)),
                                indexing="ij")
        v = 100.0 * c + 10.0 * ix + iz + 0.5 * a
        if a == 1:
            v[:6, 1, 2] = -1000
            v[6:, 2, 3] = -1000
        values.append(v)
        descs.append(g + (0.0, -1.0 - a))
    return solver.icetab_image_from_values(descs, values)


def test_driver_under_sanitizers():
    """tests/cpp/icetab_driver.cpp with the drop-in and the host route compiled in under ASan and
    UBSan (its own program, nothing preloaded): a clean exit, the same output as the build that
    links the library, lookup_host's bits, and the documented -1000 cases."""
    run = subprocess.run([DRIVER_ASAN], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lib = subprocess.run([DRIVER], capture_output=True, text=True, check=True)
    assert run.stdout == lib.stdout
    got = _driver_lines(run)
    image, descs = _builtin_image()
    q = np.array([got["Q"][i] for i in range(len(got["Q"]))])
    assert len(q) == 2 * 16 * 24
    mine, st = _lookup(image, 2, q)
    assert {0, 1, 3} <= set(st.tolist())
    for i in range(len(q)):
        assert cases.same_bits(got["V"][i], mine[i]) and cases.same_bits(got["G"][i], mine[i]), q[i]
    t = got["T"]
    for name in ("rtParameter=-1", "rtParameter=13", "AntNum=2(no-table)", "AntNum=3(beyond)", "AntNum=-1",
                 "SetNumberOfAntennas(0)"):
        assert t[name] == -1000.0, name
    inside, _ = _lookup(image, 2, np.array([[0, 1.0, -19.5]]))
    assert t["inside"] == inside[0, 0] != -1000 and t["replaced"] == 7.0
