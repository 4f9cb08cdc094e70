"""The in-ice interpolation tables on the GPU: icetab_lookup_kernel against the host lookup on the
synthetic images (batch sizes across the wave and block edges, mixed antennas, a padded leading
dimension), the four-launch build against the existing pair entries packed on the host, holes from
real rays, the reference's own 401 x 201 grid once, and the drop-in's MakeTable /
GetInterpolatedValue / GetInterpolatedValuesBatch through its driver.
Rules and synthetic tables: tests/icetab_cases.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import icetab_cases as cases
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(ROOT, "tests", "cpp", "icetab_driver")
BATCHES = (1, 63, 64, 65, 255, 256, 257, 1000)
PAD, SENTINEL, ST_SENTINEL = 3, -777.25, 0xAB
KERNELS = ("icetab_points_kernel", "iceray_kernel", "icesol_kernel", "icetab_pack_kernel",
           "icetab_lookup_kernel")
# 9 x 7, 13 x 5 and 10 x 13 positions (63, 65, 130: wave and block edges fall inside and between
# antennas), receivers at different depths.  The third sits on the edge of the shadow zone of a
# receiver 2 m deep -- transmitters 68.3 .. 69.2 m away, 3.6 .. 2.4 m deep, on the reference's own
# 0.1 m steps: towards the surface the second ray and then both rays disappear.
BUILD_GRIDS = ((100.0, -52.0, 0.5, 0.25, 9, 7, -40.0),
               (20.0, -12.5, 0.3, 0.7, 13, 5, -8.0),
               (68.3, -3.6, 0.1, 0.1, 10, 13, -2.0))


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


def _dev(a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(torch.device("cuda:0"))


class _counted:
    """Launch counts of the five kernels of this feature over a block."""

    def __enter__(self):
        from airiceraytracing_amd import _lib
        self._ctx = [_lib.launched(k) for k in KERNELS]
        for c in self._ctx:
            c.__enter__()
        return self

    def __exit__(self, *exc):
        for c in self._ctx:
            c.__exit__(*exc)
        self.counts = tuple(c.count for c in self._ctx)
        return False


@pytest.fixture(scope="module")
def synthetic(solver):
    """The synthetic tables on the device, and 1000 drawn queries with mixed antennas."""
    _, descs, values = cases.synthetic_image()
    tables = solver.ice_tables_from_values([g[:6] + (0.0, g[6]) for g in cases.GRIDS], values)
    q = cases.drawn_queries(1000, np.random.default_rng(2727))
    q.setflags(write=False)
    return tables, q


def _lookup(tables, q, pad=PAD, with_ant=True):
    """One IceTables.lookup over the (n, 3) queries, ld = n + pad, sentinels in the pad and after
    the status: ((n, 13) values, status, launch counts)."""
    import torch
    n = len(q)
    ant = _dev(q[:, 0], np.int32) if with_ant else None
    x, z = _dev(q[:, 1]), _dev(q[:, 2])
    out = torch.full((cases.PARAMS, n + pad), SENTINEL, dtype=torch.float64, device=x.device)
    st = torch.full((n + pad,), ST_SENTINEL, dtype=torch.uint8, device=x.device)
    with _counted() as c:
        tables.lookup(x, z, ant=ant, out=out, status=st, ld=n + pad,
                      stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
    o, s = out.cpu().numpy(), st.cpu().numpy()
    assert np.all(o[:, n:] == SENTINEL) and np.all(s[n:] == ST_SENTINEL)
    return o[:, :n].T.copy(), s[:n].astype(np.int64), c.counts


@pytest.fixture(scope="module")
def thousand(synthetic):
    tables, q = synthetic
    o, s, counts = _lookup(tables, q)
    for a in (o, s):
        a.setflags(write=False)
    return o, s, counts


def test_lookup_is_the_host_lookup_bit_for_bit(synthetic, thousand):
    """1000 queries, antennas mixed inside every wave: one launch of icetab_lookup_kernel and of
    nothing else; values and status are lookup_host's on the same image."""
    tables, q = synthetic
    o, s, counts = thousand
    assert counts == (0, 0, 0, 0, 1)
    want, want_st = tables.lookup_host(q[:, 1], q[:, 2], q[:, 0].astype(np.int32))
    assert cases.same_bits(o, want.T) and np.array_equal(s, want_st)
    ant = q[:64, 0]
    assert len(set(ant.tolist())) >= 3  # mixed inside the first wave
    assert {0, 1, 3, 4} <= set(s.tolist())
    # and the restatement agrees on a sample (the CPU suite checks every case)
    image = np.asarray(tables.host_image())
    for i in range(0, 1000, 50):
        ref, ref_st = cases.lookup_ref(image, 3, int(q[i, 0]), q[i, 1], q[i, 2])
        assert cases.same_bits(o[i], ref) and s[i] == ref_st, q[i]


@pytest.mark.parametrize("n", BATCHES[:-1])
def test_batches_are_one_launch_and_the_same_bits(synthetic, thousand, n):
    tables, q = synthetic
    o, s, _ = thousand
    on, sn, counts = _lookup(tables, q[:n])
    assert counts == (0, 0, 0, 0, 1)
    assert cases.same_bits(on, o[:n]) and np.array_equal(sn, s[:n])


def test_reversed_batch_and_null_antennas(synthetic, thousand):
    tables, q = synthetic
    o, s, _ = thousand
    ro, rs, counts = _lookup(tables, np.ascontiguousarray(q[::-1]))
    assert counts == (0, 0, 0, 0, 1)
    assert cases.same_bits(ro[::-1], o) and np.array_equal(rs[::-1], s)
    # d_ant NULL: every query reads antenna 0
    q0 = np.array(q)
    q0[:, 0] = 0
    want, want_st, _ = _lookup(tables, q0)
    got, got_st, counts = _lookup(tables, q, with_ant=False)
    assert counts == (0, 0, 0, 0, 1)
    assert cases.same_bits(got, want) and np.array_equal(got_st, want_st)
    assert (want_st & cases.BAD_ANTENNA == 0).all()


# ---- the build -----------------------------------------------------------------------------------
def _build(grids, a0=1.0, frequency=0.1):
    """airice_icetab_build_launch into an image followed by a sentinel record: (image as numpy
    without the sentinel, descs, launch counts)."""
    import torch
    from airiceraytracing_amd import _lib, solver as sv
    L = _lib.lib()
    descs, size = sv.icetab_descs([g[:6] + (0.0, g[6]) for g in grids])
    work = ctypes.c_size_t(0)
    _lib.check(L.airice_icetab_work_bytes(_lib.ptr(descs), len(descs), ctypes.byref(work)), "work")
    dev = torch.device("cuda:0")
    image = torch.full((size + 16,), SENTINEL, dtype=torch.float64, device=dev)
    buf = torch.empty((work.value + 7) // 8, dtype=torch.float64, device=dev)
    with _counted() as c:
        _lib.check(L.airice_icetab_build_launch(None, _lib.ptr(image), _lib.ptr(descs), len(descs),
                                                a0, frequency, _lib.ptr(buf), work.value,
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "build")
        torch.cuda.synchronize()
    h = image.cpu().numpy()
    assert (h[size:] == SENTINEL).all()
    return h[:size].copy(), descs, c.counts


def _pair_records(solver, desc, picks=None):
    """The records of a grid by the existing pair entries on numpy-made points: ice_rays_device
    twice (the receiver, and 1 cm lower), ice_solutions_device once, packed by pack_host."""
    import torch
    from airiceraytracing_amd import _lib, solver as sv
    xs, zs, dx, dz, nx, nz, _, rx = desc
    nx, nz = int(nx), int(nz)
    ix, iz = np.divmod(np.arange(nx * nz) if picks is None else np.asarray(picks), nz)
    z0 = np.float64(zs) + np.float64(dz) * iz.astype(np.float64)
    x1 = np.float64(xs) + np.float64(dx) * ix.astype(np.float64)
    z1 = np.full(len(ix), rx)
    lower = z1 - np.float64(0.01)
    n = len(ix)
    d = [_dev(a) for a in (z0, x1, z1, lower)]
    rays = torch.empty((_lib.ICERAY_FIELDS, n), dtype=torch.float64, device=d[0].device)
    rays_lower = torch.empty_like(rays)
    out = torch.empty((_lib.ICESOL_FIELDS, n), dtype=torch.float64, device=d[0].device)
    st = torch.empty(n, dtype=torch.uint8, device=d[0].device)
    stream = torch.cuda.current_stream()
    solver.ice_rays_device(d[0], d[1], d[2], rays, stream=stream)
    solver.ice_rays_device(d[0], d[1], d[3], rays_lower, stream=stream)
    solver.ice_solutions_device(d[0], d[1], d[2], rays, out, st, rays_lower=rays_lower,
                                stream=stream)
    torch.cuda.synchronize()
    return sv.icetab_pack_host(out.cpu().numpy(), st.cpu().numpy())


@pytest.fixture(scope="module")
def joint():
    image, descs, counts = _build(BUILD_GRIDS)
    image.setflags(write=False)
    return image, descs, counts


def test_build_is_four_launches_and_the_pair_entries_bits(solver, joint):
    """Three antennas, 258 positions: one launch each of icetab_points_kernel, iceray_kernel,
    icesol_kernel and icetab_pack_kernel; the header as laid out; every record bit for bit what
    ice_rays_device (twice) and ice_solutions_device give on numpy-made points, packed by
    pack_host; the sentinel after the image untouched."""
    image, descs, counts = joint
    assert counts == (1, 1, 1, 1, 0)
    assert list(descs[:, 6]) == [2.0, 65.0, 130.0] and image.size == 16 * (2 + 63 + 65 + 130)
    assert cases.same_bits(image[:24], descs.ravel()) and (image[24:32] == 0).all()
    for a in range(3):
        first, cells = int(descs[a, 6]), int(descs[a, 4] * descs[a, 5])
        got = image[first * 16:(first + cells) * 16].reshape(cells, 16)
        want = _pair_records(solver, descs[a])
        assert cases.same_bits(got, want), a
        assert (got[:, 14:] == 0).all()
    # real tables: both rays over most of the deep antennas' grids
    assert (image[32:32 + 63 * 16].reshape(63, 16)[:, :12] != -1000).all()


def test_each_antenna_alone_is_its_slice(joint):
    image, descs, _ = joint
    for a in range(3):
        alone, d, counts = _build(BUILD_GRIDS[a:a + 1])
        assert counts == (1, 1, 1, 1, 0), a
        first, cells = int(descs[a, 6]), int(descs[a, 4] * descs[a, 5])
        assert d[0, 6] == 1 and alone.size == 16 + cells * 16
        assert cases.same_bits(alone[16:], image[first * 16:(first + cells) * 16]), a
        assert cases.same_bits(alone[:6], descs[a, :6]) and alone[7] == descs[a, 7]


def test_holes_from_real_rays(solver):
    """The third antenna's grid crosses the edge of the receiver's shadow zone on the reference's
    own 0.1 m steps (confirmed beforehand on the host route, ice_solutions_host one position per
    call: at zT = -3.0 m both rays exist up to xT = 68.7 m and only the first beyond, at -2.9 m
    only the first up to 68.5 m and none beyond).  So its table has cells with both -1000 and
    valid corners in the slot-1 group; lookups inside them take the inverse-distance branch and
    equal lookup_host on the copied-back image."""
    g = BUILD_GRIDS[2]
    tables = solver.ice_tables(0.0, 0.0, None, grids=[g[:6] + (0.0, g[6])])
    v = tables.values(0)
    nx, nz = v.shape[1:]
    missing = (v[6:12] == -1000).all(axis=0)
    assert ((v[6:12] == -1000).any(axis=0) == missing).all()  # a slot is missing as a whole
    corners = missing[:-1, :-1].astype(int) + missing[:-1, 1:] + missing[1:, :-1] + missing[1:, 1:]
    mixed = np.argwhere((corners > 0) & (corners < 4))
    assert len(mixed) >= 1
    import torch
    q = np.array([(0, cases.position(g[0], g[2], bx) + 0.37 * g[2],
                   cases.position(g[1], g[3], bz) + 0.61 * g[3]) for bx, bz in mixed])
    st = torch.zeros(len(q), dtype=torch.uint8, device="cuda:0")
    out = tables.lookup(_dev(q[:, 1]), _dev(q[:, 2]), status=st)
    torch.cuda.synchronize()
    got, got_st = out.cpu().numpy(), st.cpu().numpy()
    assert (got_st == cases.CELL | cases.IDW).all()
    want, want_st = tables.lookup_host(q[:, 1], q[:, 2])
    assert cases.same_bits(got, want) and np.array_equal(got_st, want_st)
    assert (got[6:12] != -1000).all()  # the mean of the valid corners
    image = np.asarray(tables.host_image())
    for i in range(len(q)):
        ref, ref_st = cases.lookup_ref(image, 1, 0, q[i, 1], q[i, 2])
        assert cases.same_bits(got[:, i], ref) and got_st[i] == ref_st


def test_the_reference_grid_once(solver):
    """ice_tables(150, -100, [-100]): MakeTable's own 401 x 201 positions in four launches; 1000
    records drawn at random are the pair entries' bits; lookup at 1000 random interior points is
    lookup_host."""
    import torch
    rng = np.random.default_rng(2614)
    with _counted() as c:
        tables = solver.ice_tables(150.0, -100.0, [-100.0], stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
    assert c.counts == (1, 1, 1, 1, 0)
    d = tables.descs[0]
    assert list(d) == [130.0, -110.0, 0.1, 0.1, 401.0, 201.0, 1.0, -100.0]
    image = np.asarray(tables.host_image())
    assert image.size == 16 + 401 * 201 * 16
    picks = rng.choice(401 * 201, 1000, replace=False)
    got = image[16:].reshape(401 * 201, 16)[picks]
    assert cases.same_bits(got, _pair_records(solver, d, picks))
    x = rng.uniform(130.0, 170.0, 1000)
    z = rng.uniform(-110.0, -90.0, 1000)
    st = torch.zeros(1000, dtype=torch.uint8, device="cuda:0")
    out = tables.lookup(_dev(x), _dev(z), status=st, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    want, want_st = tables.lookup_host(x, z)
    assert cases.same_bits(out.cpu().numpy(), want) and np.array_equal(st.cpu().numpy(), want_st)
    assert (want_st & cases.CELL).all() and (want[:6] != -1000).all()


def _driver_lines(stdout):
    got = {}
    for line in stdout.splitlines():
        tag, key, *words = line.split()
        got.setdefault(tag, {})[int(key)] = np.array([int(w, 16) for w in words],
                                                     dtype=np.uint64).view(np.float64)
    return got


@pytest.mark.parametrize("mode", ["make", "makes"])
def test_drop_in_make_table_is_the_python_path(solver, tmp_path, mode):
    """SetNumberOfAntennas, MakeTable per antenna (or one MakeTables) and GetInterpolatedValue in
    a child process: the bits of ice_tables(...).lookup_host for the same arguments;
    GetInterpolatedValuesBatch equals the 13 scalar calls per query.  AntNum 2 has no table."""
    hit, depth, zr = 35.0, -14.0, (-6.0, -25.0)
    rng = np.random.default_rng(3212)
    n = 300
    q = np.empty((n, 3))
    q[:, 0] = rng.integers(0, 3, n)
    q[:, 1] = rng.uniform(hit - 21.0, hit + 21.0, n)
    q[:, 2] = rng.uniform(depth - 10.5, depth + 10.5, n)
    path = os.path.join(str(tmp_path), "make.bin")
    np.array([hit, depth, len(zr), *zr, n, *q.ravel()], dtype=np.float64).tofile(path)
    run = subprocess.run([DRIVER, mode, path], capture_output=True, text=True, check=True)
    assert run.stderr == "", run.stderr
    got = _driver_lines(run.stdout)
    tables = solver.ice_tables(hit, depth, zr)
    known = q[:, 0] < 2
    want, want_st = tables.lookup_host(q[:, 1], q[:, 2], np.where(known, q[:, 0], 2).astype(np.int32))
    assert (want_st & cases.CELL).sum() > n // 3
    for i in range(n):
        assert cases.same_bits(got["G"][i], want[:, i]), (i, q[i])
        assert cases.same_bits(got["V"][i], want[:, i]), (i, q[i])
        assert cases.same_bits(got["B"][i][:13], got["G"][i]), (i, q[i])
        assert got["B"][i][13] == want_st[i]
