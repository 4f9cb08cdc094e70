"""The in-ice ray-path samplers on the GPU: icepath_consts_kernel and icepath_kernel against the
host route over the same solver rows, batch shapes around the wave and the tile, independence of
the batch and its order, the physics of device samples, the masks and the kernel timer."""
import numpy as np
import pytest

from tests import icepath_cases as cases
from tests import iceray_cases as rc

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
N_ALL = 257
N_SINGLE = 80  # one-pair calls in all
KERNELS = ("icepath_consts_kernel", "icepath_kernel")


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


@pytest.fixture(scope="module")
def solved(solver):
    """257 pairs (the shape rows at the head), the solver's rows for them from the host route --
    what both the device and the host samplers read -- and the host route's paths."""
    q = cases.batch(N_ALL, np.random.default_rng(2033))
    out, st = rc.host_rows(solver, q)
    paths = cases.host_paths(q, out, st)
    for a in (q, out, st):
        a.setflags(write=False)
    return q, out, st, paths


def run_device(solver, q, out, mask=15, status=None, pad=64):
    """One airice_icepath_launch over pairs q with the solver rows out (n, 32) uploaded.
    Returns (offsets, count, x, z, launches of the two kernels); x and z were filled with SENTINEL
    and are `pad` slots longer than the plan."""
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    n = len(q)
    q, out = np.array(q, dtype=np.float64), np.array(out, dtype=np.float64)  # own, writable copies
    cols = [torch.from_numpy(q[:, k].copy()).to(dev) for k in range(3)]
    rays = torch.from_numpy(out.T.copy()).to(dev)
    z0h, z1h = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 2])
    off = solver.ice_ray_paths_plan(z0h, z1h, status, mask)
    total = int(off[-1])
    x = torch.full((total + pad,), SENTINEL, dtype=torch.float64, device=dev)
    z = torch.full((total + pad,), SENTINEL, dtype=torch.float64, device=dev)
    count = torch.full((4 * n,), -1, dtype=torch.int64, device=dev)
    with _lib.launched(KERNELS[0]) as a, _lib.launched(KERNELS[1]) as b:
        work = solver.ice_ray_paths_device(cols[0], cols[1], cols[2], rays, off, count, x, z,
                                           z0_host=z0h, z1_host=z1h, status=status, rays=mask,
                                           stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
    del work
    return off, count.cpu().numpy(), x.cpu().numpy(), z.cpu().numpy(), (a.count, b.count)


def segment(off, count, x, z, s):
    return x[off[s]:off[s] + count[s]], z[off[s]:off[s] + count[s]]


@pytest.fixture(scope="module")
def whole(solver, solved):
    q, out, st, _ = solved
    got = run_device(solver, q, out)
    for a in got[:4]:
        a.setflags(write=False)
    return got


@pytest.fixture(scope="module")
def singles(solver, solved):
    """The first 80 pairs, one pair per call."""
    q, out, st, _ = solved
    return [run_device(solver, q[i:i + 1], out[i:i + 1], pad=1) for i in range(N_SINGLE)]


def check_untouched(off, count, x, z, n):
    """d_count <= capacity; every slot past a count and past offsets[4n] is still the sentinel."""
    cap = np.diff(off)
    assert (count >= 0).all() and (count <= cap).all()
    written = np.zeros(len(x), dtype=bool)
    for s in range(4 * n):
        written[off[s]:off[s] + count[s]] = True
    for a in (x, z):
        assert (a[~written] == SENTINEL).all()
        assert not (a[written] == SENTINEL).any() and np.isfinite(a[written]).all()
    assert not written[off[-1]:].any() and len(x) > off[-1]


def check_against_host(q, st, paths, off, count, x, z, n):
    """Counts and every z equal the host route's; |dx| <= 1e-9 max(1 m, x1).  Returns max |dx|."""
    worst = 0.0
    for i in range(n):
        for ray in range(4):
            s = 4 * i + ray
            if (i, ray) not in paths:
                assert count[s] == 0, (q[i], ray)
                continue
            hx, hz = paths[(i, ray)]
            dx, dz = segment(off, count, x, z, s)
            assert count[s] == len(hz), (q[i], ray, count[s], len(hz))
            assert rc.same_bits(dz, hz), (q[i], ray)
            err = np.abs(dx - hx).max()
            assert err <= 1e-9 * max(1.0, abs(q[i, 1])), (q[i], ray, err)
            worst = max(worst, err)
    return worst


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batches(solver, solved, whole, singles, n):
    q, out, st, paths = solved
    if n == N_ALL:
        off, count, x, z, launches = whole
    else:
        off, count, x, z, launches = run_device(solver, q[:n], out[:n])
    assert launches == (1, 1)
    check_untouched(off, count, x, z, n)
    worst = check_against_host(q, st, paths, off, count, x, z, n)
    print(f"[icepath gpu] n = {n}: {int(count.sum())} samples of {int((count > 0).sum())} rays, "
          f"device against host route max |dx| = {worst:.2e} m")
    assert {ray for (i, ray) in paths if i < n} == ({1, 2} if n == 1 else {0, 1, 2, 3})
    # the same pairs one pair per call: bit for bit
    for i in range(min(n, N_SINGLE)):
        so, sc, sx, sz, sl = singles[i]
        assert sl == ((1, 1) if so[-1] > 0 else (0, 0))
        for ray in range(4):
            a = segment(off, count, x, z, 4 * i + ray)
            b = segment(so, sc if so[-1] > 0 else np.zeros(4, dtype=np.int64), sx, sz, ray)
            assert rc.same_bits(a[0], b[0]) and rc.same_bits(a[1], b[1]), (q[i], ray)
    # the batch reversed: bit for bit
    roff, rcount, rx, rz, _ = run_device(solver, q[:n][::-1], out[:n][::-1])
    for i in range(n):
        for ray in range(4):
            a = segment(off, count, x, z, 4 * i + ray)
            b = segment(roff, rcount, rx, rz, 4 * (n - 1 - i) + ray)
            assert rc.same_bits(a[0], b[0]) and rc.same_bits(a[1], b[1]), (q[i], ray)


def test_physics_of_device_samples(solved, whole):
    """At most 200 device samples of at most 40 accepted rays against mpmath quadrature:
    |x - integral| <= 1e-9 max(1 m, x1)."""
    q, out, st, paths = solved
    off, count, x, z, _ = whole
    dev = {(i, ray): segment(off, count, x, z, 4 * i + ray) for (i, ray) in paths}
    got = np.array(cases.physics_samples(q, out, st, dev, np.random.default_rng(11)))
    print(f"[icepath gpu physics] {len(got)} samples: worst {got[:, 3].max():.2e} m, "
          f"{np.max(got[:, 3] / got[:, 4]):.2e} of its bound")
    assert len(got) >= 100 and set(got[:, 1]) == {0.0, 1.0, 2.0, 3.0}
    bad = got[got[:, 3] > got[:, 4]]
    assert len(bad) == 0, (bad[:5], q[bad[:5, 0].astype(int)])


def test_masks_shrink_the_plan_and_keep_the_bits(solver, solved, whole):
    q, out, st, paths = solved
    off, count, x, z, _ = whole
    n = 65
    for mask, status in ((rc.D, None), (15, np.ascontiguousarray(st[:n], dtype=np.uint8)),
                         (rc.R | rc.RA0, np.ascontiguousarray(st[:n], dtype=np.uint8))):
        moff, mcount, mx, mz, launches = run_device(solver, q[:n], out[:n], mask=mask,
                                                    status=status)
        assert launches == (1, 1) and 0 < moff[-1] < off[4 * n]
        check_untouched(moff, mcount, mx, mz, n)
        for i in range(n):
            for ray in range(4):
                s = 4 * i + ray
                if mask & (1 << ray):
                    a, b = segment(off, count, x, z, s), segment(moff, mcount, mx, mz, s)
                    assert rc.same_bits(a[0], b[0]) and rc.same_bits(a[1], b[1]), (q[i], ray)
                else:
                    assert mcount[s] == 0 and moff[s + 1] == moff[s]
                if status is not None and not status[i] & (1 << ray):
                    assert moff[s + 1] == moff[s]


def test_host_entry_and_timer(solver, solved, whole):
    """airice_icepath_host (ice_ray_paths_host: solver, plan and paths in one call) gives the
    device launch's samples where the device solver's row is the host route's, and the kernel
    timer reports both kernels."""
    from airiceraytracing_amd import _lib
    q, out, st, paths = solved
    off, count, x, z, _ = whole
    n = 40
    _lib.kernel_timing(True)
    try:
        for k in KERNELS:
            _lib.kernel_time(k, reset=True)
        hoff, hcount, hx, hz = solver.ice_ray_paths_host(q[:n, 0], q[:n, 1], q[:n, 2])
        times = {k: _lib.kernel_time(k, reset=True) for k in KERNELS}
    finally:
        _lib.kernel_timing(False)
    for k in KERNELS:
        ms, launches = times[k]
        assert launches == 1 and ms > 0.0, (k, times[k])
    dout, dst = solver.ice_rays_host(q[:n, 0], q[:n, 1], q[:n, 2])
    assert (hcount <= np.diff(hoff)).all()
    same = 0
    for i in range(n):
        for ray in range(4):
            s = 4 * i + ray
            accepted = bool(dst[i] & (1 << ray)) and not dst[i] & rc.NONFINITE
            assert (hcount[s] > 0) == accepted, (q[i], ray)
            if not accepted or dst[i] != st[i]:
                continue
            hzs = hz[hoff[s]:hoff[s] + hcount[s]]
            L_same = dout[rc.LVALUE + ray, i] == out[i, rc.LVALUE + ray]
            if L_same and (ray < 2 or dout[rc.ZMAX + ray - 2, i] == out[i, rc.ZMAX + ray - 2]):
                a = segment(off, count, x, z, s)
                assert rc.same_bits(a[1], hzs) and rc.same_bits(
                    a[0], hx[hoff[s]:hoff[s] + hcount[s]]), (q[i], ray)
                same += 1
            elif ray < 2:  # the depths of D and R need no L
                assert rc.same_bits(segment(off, count, x, z, s)[1], hzs)
    print(f"[icepath gpu host entry] {same} rays with the host route's L: the same bits")
