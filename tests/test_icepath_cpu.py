"""The in-ice ray-path samplers (airice_icepath_plan / _launch / _host / _one_host, the
IceRayTracing::GetFull*RayPath drop-in) without a GPU: header and exports, the host plan, the host
route against a restatement of the reference's depth chain and against numerical integration, the
drop-in bit for bit (also as its own program under ASan + UBSan), and the launch's argument
checks."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import icepath_cases as cases
from tests import iceray_cases as rc
from tests.conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "cpp", "icepath_driver")
DRIVER_ASAN = os.path.join(ROOT, "tests", "cpp", "icepath_driver_asan")
N_DRAWN = 300
KERNELS = ("icepath_consts_kernel", "icepath_kernel", "iceray_kernel")


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


@pytest.fixture(scope="module")
def rows(solver):
    """The head rows and 300 drawn rows, solved and sampled on the host route once."""
    q = np.concatenate([cases.head_rows(), rc.drawn(N_DRAWN, np.random.default_rng(2031))])
    out, st = rc.host_rows(solver, q)
    paths = cases.host_paths(q, out, st)
    for a in (q, out, st):
        a.setflags(write=False)
    return q, out, st, paths


def _plan(q, status=None, mask=15):
    from airiceraytracing_amd import _lib
    z0, z1 = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 2])
    st = None if status is None else np.ascontiguousarray(status, dtype=np.uint8)
    off = np.full(4 * len(q) + 1, -1, dtype=np.int64)
    work = ctypes.c_size_t(0)
    assert _lib.lib().airice_icepath_plan(_lib.ptr(z0), _lib.ptr(z1), _lib.ptr(st), len(q), mask,
                                          _lib.ptr(off), ctypes.byref(work)) == 0
    return off, work.value


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import AirIceSolver, _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    for name in ("airice_icepath_plan", "airice_icepath_launch", "airice_icepath_host",
                 "airice_icepath_one_host"):
        assert f"int {name}(" in header, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    for kernel in KERNELS[:2]:
        assert f'"{kernel}"' in header
        assert _lib.launch_count(kernel) >= 0  # the counter and the timer exist
        assert _lib.kernel_time(kernel, reset=False) == (0.0, 0)
    with open(os.path.join(ROOT, "include", "IceRayTracing.hh")) as f:
        dropin = f.read()
    for name in ("GetFullDirectRayPath", "GetFullReflectedRayPath", "GetFullRefractedRayPath",
                 "PlotAndStoreRays"):
        assert f"void {name}(" in dropin, name
    for name in ("ice_ray_paths_plan", "ice_ray_paths_work_bytes", "ice_ray_paths_device",
                 "ice_ray_paths_host"):
        assert callable(getattr(AirIceSolver, name)), name


def test_plan_capacities(rows):
    q, out, st, paths = rows
    off, work = _plan(q)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and work > 0
    cap = np.diff(off).reshape(-1, 4)
    bad = ~((q[:, 0] <= 0) & (q[:, 0] >= -50000) & (q[:, 2] <= 0) & (q[:, 2] >= -50000))
    assert bad.sum() == 6 and (cap[bad] == 0).all()  # the rows with a NaN or infinite depth
    assert (cap[~bad] > 0).all()
    # exact D and R capacities are the host route's counts, the Ra capacity bounds the Ra count
    for (i, ray), (x, z) in paths.items():
        if ray < 2:
            assert cap[i, ray] == len(z), (q[i], ray)
        else:
            assert cap[i, ray] >= len(z) > 0, (q[i], ray)
            assert cap[i, ray] == cap[i, 1] + 1
    assert {ray for _, ray in paths} == {0, 1, 2, 3}
    # the shape rows' direct counts, each row followed by its flip
    assert [int(c) for c in cap[:10:2, 0]] == list(cases.DIRECT_COUNTS)
    assert [int(c) for c in cap[1:10:2, 0]] == list(cases.DIRECT_COUNTS)
    # a depth above the surface, and one below the reference's 100,000 steps
    extra = np.array([(-100.0, 10.0, 1e-3), (-50000.5, 10.0, -10.0), (-50000.0, 10.0, -10.0)])
    cx = np.diff(_plan(extra)[0]).reshape(-1, 4)
    assert (cx[:2] == 0).all() and cx[2, 0] == 2 * 49990 + 2
    # masked kinds get 0 and the others keep their capacity; so do kinds whose status bit is clear
    for mask in (rc.D, rc.R | rc.RA1, 0):
        cm = np.diff(_plan(q, mask=mask)[0]).reshape(-1, 4)
        for ray in range(4):
            assert (cm[:, ray] == (cap[:, ray] if mask & (1 << ray) else 0)).all()
    cs = np.diff(_plan(q, status=st)[0]).reshape(-1, 4)
    for ray in range(4):
        on = (st & (1 << ray)) != 0
        assert (cs[on, ray] == cap[on, ray]).all() and (cs[~on, ray] == 0).all()
    assert (cs[(st & rc.NONFINITE) != 0] == 0).all()
    assert _plan(q[:0])[0].tolist() == [0]


def test_host_route_follows_the_reference_chain(rows):
    q, out, st, paths = rows
    worst, moved, total = 0.0, 0, 0
    n_shape, n_head = len(cases.shape_rows()), len(cases.head_rows())
    for (i, ray), (x, z) in paths.items():
        z0, x1, z1 = q[i]
        zmax = out[i, rc.ZMAX + ray - 2] if ray >= 2 else 0.0
        ref, n1 = cases.reference_depths(ray, z0, z1, zmax)
        assert len(z) == len(x)
        if n_shape <= i < n_head:
            # the solver's class and edge rows are not part of the chain comparison: two-decimal
            # depths can put a chain's last step within an ulp of z0, where rounding once and the
            # running chain disagree about the duplicate closing sample (-536.68 from -44.18:
            # 987 samples here, 986 in the chain)
            assert abs(len(z) - len(ref)) <= 1, (q[i], ray, len(z), len(ref))
            if len(z) != len(ref):  # the depths before the closing samples still agree
                m = min(len(z), len(ref)) - 2
                assert m <= 0 or cases.ulp_distance(z[:m], ref[:m]).max() <= 1.0
                print("[icepath chain] count", len(z), "here,", len(ref), "in the chain:", q[i], ray)
                ref = z
        assert len(z) == len(ref), (q[i], ray, len(z), len(ref))
        d = cases.ulp_distance(z, ref)
        worst, moved, total = max(worst, d.max()), moved + int((d > 0).sum()), total + len(z)
        assert np.isfinite(x).all() and np.isfinite(z).all(), (q[i], ray)
        # the ends: the upper of the two depths first, the lower last; x runs between 0 and x1
        # (to the residual the solver's search stopped at)
        hi, lo = max(z0, z1), min(z0, z1)
        tol = abs(rc.checkzero(ray, out[i, rc.LVALUE + ray], z0, x1, z1)) + 1e-9 * max(1.0, abs(x1))
        assert z[0] == hi and z[-1] == lo
        first, last = (x1, 0.0) if z0 <= z1 else (0.0, x1)
        assert abs(x[0] - first) <= tol and abs(x[-1] - last) <= tol, (q[i], ray, x[0], x[-1])
        if ray >= 2:  # the apex sample is there and finite
            assert z[n1] == -zmax and np.isfinite(x[n1]), (q[i], ray)
    print(f"[icepath chain] {len(paths)} rays, {total} samples: {moved} depths differ from the "
          f"running chain, the worst by {worst:.2f} ulp")
    assert worst <= 1.0
    # the shape rows: their direct counts, the duplicate closing sample, R's sample at exactly 0
    for j, want in enumerate(cases.DIRECT_COUNTS):
        for i in (2 * j, 2 * j + 1):
            if st[i] & rc.D:  # (the solver finds no direct ray 0.3 m deep over 60 m, nor a flat one)
                assert len(paths[(i, 0)][1]) == want, q[i]
            # the count needs no accepted ray: any L below n samples the same depths
            assert len(cases.one_host(0, *q[i], 0.5)[1]) == want
    assert all(st[i] & rc.D for i in range(2, 8))
    z = paths[(2, 0)][1]
    assert z[-1] == z[-2] == -177.0
    assert (paths[(10, 1)][1] == 0.0).sum() == 1
    # the refracted ray whose first leg is one sample
    i = 11
    assert tuple(q[i]) == cases.SINGLE_LEG1_ROW and st[i] & rc.RA0
    zs = paths[(i, 2)][1]
    assert zs[0] == q[i, 2] and zs[1] == -out[i, rc.ZMAX] and zs[1] > zs[0] and zs[2] < zs[1]


def test_flip_gives_x1_minus_x(rows):
    q, out, st, paths = rows
    seen = 0
    for i in range(0, 8, 2):  # each shape row and its flip (equal depths are their own flip)
        assert st[i] == st[i + 1]
        for ray in range(4):
            if not st[i] & (1 << ray):
                continue
            # the flipped pair's solver row holds the same L (the searches take Tx below Rx)
            assert out[i, rc.LVALUE + ray] == out[i + 1, rc.LVALUE + ray]
            (x, z), (xf, zf) = paths[(i, ray)], paths[(i + 1, ray)]
            assert rc.same_bits(z, zf) and rc.same_bits(q[i, 1] - x, xf), (q[i], ray)
            seen += 1
    assert seen >= 8
    assert rc.same_bits(paths[(8, 1)][0], paths[(9, 1)][0])
    # rows 1 and 8 of the solver's classes are each other's flip, with a refracted ray
    a, b = 12 + 1, 12 + 8
    assert tuple(q[a, [0, 2]]) == tuple(q[b, [2, 0]])
    for ray in (1, 2):
        assert rc.same_bits(q[a, 1] - paths[(a, ray)][0], paths[(b, ray)][0])


def test_physics_of_the_samples(rows):
    """At most 200 samples (first, last, the leg joints, 2 drawn per ray) of at most 40 accepted
    rays against mpmath quadrature at 30 digits: |x - integral| <= 1e-9 max(1 m, x1)."""
    q, out, st, paths = rows
    got = np.array(cases.physics_samples(q, out, st, paths, np.random.default_rng(7)))
    print(f"[icepath physics] {len(got)} samples of {len(set(map(tuple, got[:, :2])))} rays: worst "
          f"{got[:, 3].max():.2e} m, {np.max(got[:, 3] / got[:, 4]):.2e} of its bound")
    assert len(got) >= 100 and set(got[:, 1]) == {0.0, 1.0, 2.0, 3.0}
    bad = got[got[:, 3] > got[:, 4]]
    assert len(bad) == 0, (bad[:5], q[bad[:5, 0].astype(int)])


def test_one_host_arguments():
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    cnt = ctypes.c_int64(-1)
    x, z = np.zeros(4), np.zeros(4)
    args = (-50.3, 60.0, -50.0, 1.3, 0.0)
    assert L.airice_icepath_one_host(None, rc.D, *args, _lib.ptr(x), _lib.ptr(z), 4,
                                     ctypes.byref(cnt)) == 0 and cnt.value == 2
    assert L.airice_icepath_one_host(None, rc.D, *args, _lib.ptr(x), _lib.ptr(z), 1,
                                     ctypes.byref(cnt)) == -1 and cnt.value == 2
    assert "cap" in L.airice_last_error().decode()
    assert L.airice_icepath_one_host(None, rc.D, *args, None, _lib.ptr(z), 4,
                                     ctypes.byref(cnt)) == -1
    assert "(x)" in L.airice_last_error().decode()
    assert L.airice_icepath_one_host(None, rc.D, *args, _lib.ptr(x), _lib.ptr(z), 4, None) == -1
    assert "(count)" in L.airice_last_error().decode()
    for kind in (0, 3, 16, rc.NONFINITE):
        assert L.airice_icepath_one_host(None, kind, *args, _lib.ptr(x), _lib.ptr(z), 4,
                                         ctypes.byref(cnt)) == -1
        assert "kind" in L.airice_last_error().decode()
    # no samples, and no error: non-finite values, depths outside the ice, a negative zmax
    for bad in ((np.nan, 60.0, -50.0, 1.3, 0.0), (-50.3, np.inf, -50.0, 1.3, 0.0),
                (-50.3, 60.0, 0.5, 1.3, 0.0), (-50.3, 60.0, -50.0, np.nan, 0.0)):
        assert L.airice_icepath_one_host(None, rc.D, *bad, None, None, 0, ctypes.byref(cnt)) == 0
        assert cnt.value == 0, bad
    assert L.airice_icepath_one_host(None, rc.RA0, -180.0, 500.0, -100.0, 1.66, -1.0, None, None,
                                     0, ctypes.byref(cnt)) == 0 and cnt.value == 0
    # another ice model changes the samples, the default one given explicitly does not
    a = cases.one_host(0, -180.0, 100.0, -100.0, 1.3)
    b = cases.one_host(0, -180.0, 100.0, -100.0, 1.3, model=(1.78, -0.43, 0.0132))
    c = cases.one_host(0, -180.0, 100.0, -100.0, 1.3, model=(1.775, -0.45, 0.014))
    assert rc.same_bits(a[0], b[0]) and rc.same_bits(a[1], c[1]) and not rc.same_bits(a[0], c[0])


def test_solver_host_route_is_one_host(solver, rows):
    """ice_ray_paths_host for one pair runs on the calling thread and returns the host route."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    q, out, st, paths = rows
    before = [_lib.launch_count(k) for k in KERNELS]
    with scalar_mode(_lib.SCALAR_HOST):
        for i in (0, 2, 10, 11, 13, 16, 24, 30):
            off, count, x, z = solver.ice_ray_paths_host(*q[i])
            assert (count <= np.diff(off)).all()
            for ray in range(4):
                if st[i] & (1 << ray) and not st[i] & rc.NONFINITE:
                    lo = off[ray]
                    assert rc.same_bits(x[lo:lo + count[ray]], paths[(i, ray)][0]), (q[i], ray)
                    assert rc.same_bits(z[lo:lo + count[ray]], paths[(i, ray)][1]), (q[i], ray)
                else:
                    assert count[ray] == 0 and off[ray + 1] == off[ray]
        off, count, x, z = solver.ice_ray_paths_host(*q[0], rays=rc.R)
        assert count.tolist() == [0, len(paths[(0, 1)][0]), 0, 0]
    assert [_lib.launch_count(k) for k in KERNELS] == before


def _driver_paths(program, q, tmp_path):
    path = os.path.join(tmp_path, "rows.bin")
    np.ascontiguousarray(q, dtype=np.float64).tofile(path)
    run = subprocess.run([program, path], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    got = {"X": {}, "Z": {}, "P": set()}
    for line in run.stdout.splitlines():
        tag, row, *words = line.split()
        if tag == "P":
            got["P"].add(int(row))
            continue
        ray, words = int(words[0]), words[1:]
        got[tag][(int(row), ray)] = np.array([int(w, 16) for w in words],
                                             dtype=np.uint64).view(np.float64)
    return got, run.stdout


def test_drop_in_is_the_host_route_bit_for_bit(rows, tmp_path):
    """tests/cpp/icepath_driver.cpp: the three GetFull* functions with the solver's L and zmax
    append airice_icepath_one_host's samples, and PlotAndStoreRays returns -- in the program linked
    against the library and in the one compiled with the drop-in under ASan + UBSan (its own
    program, nothing preloaded)."""
    q, out, st, paths = rows
    n = len(cases.head_rows()) + 40
    got, text = _driver_paths(DRIVER, q[:n], str(tmp_path))
    want = {k: v for k, v in paths.items() if k[0] < n}
    assert set(got["X"]) == set(got["Z"]) == set(want) and got["P"] == set(range(n))
    for key, (x, z) in want.items():
        assert rc.same_bits(got["X"][key], x) and rc.same_bits(got["Z"][key], z), (q[key[0]], key)
    _, text_asan = _driver_paths(DRIVER_ASAN, q[:n], str(tmp_path))
    assert text_asan == text
    run = subprocess.run([DRIVER_ASAN], capture_output=True, text=True)  # its fixed pairs
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout == subprocess.run([DRIVER], capture_output=True, text=True,
                                        check=True).stdout


# ---- argument checks, in the vocabulary of test_hostcall_checks.py --------------------------------
N = 8


def _fake(k):
    return ctypes.c_void_p(0x100000 * (k + 1))  # 16-byte aligned, never dereferenced


def _launch_args():
    """airice_icepath_launch's arguments for 8 real host pairs and device pointers nothing maps;
    every call below is refused before a device call."""
    q = cases.head_rows()[:N]
    z0, z1 = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 2])
    off, work = _plan(q)
    names = ["model3", "d_z0", "d_x1", "d_z1", "d_rays", "ld_rays", "z0", "z1", "status", "n",
             "ray_mask", "offsets", "d_work", "work_bytes", "d_count", "d_x", "d_z", "cap",
             "stream"]
    from airiceraytracing_amd import _lib
    vals = [None, _fake(0), _fake(1), _fake(2), _fake(3), N, _lib.ptr(z0), _lib.ptr(z1), None, N,
            15, _lib.ptr(off), _fake(4), work, _fake(5), _fake(6), _fake(7), int(off[-1]), None]
    return names, vals, (z0, z1, off)


def _host_args():
    q = cases.head_rows()[:N]
    cols = [np.ascontiguousarray(q[:, k]) for k in range(3)]
    off, _ = _plan(q)
    keep = cols + [off, np.zeros((32, N)), np.zeros(4 * N, dtype=np.int64),
                   np.zeros(int(off[-1])), np.zeros(int(off[-1]))]
    from airiceraytracing_amd import _lib
    names = ["model3", "z0", "x1", "z1", "rays", "ld_rays", "status", "n", "ray_mask", "offsets",
             "count", "x", "z", "cap"]
    vals = [None, _lib.ptr(cols[0]), _lib.ptr(cols[1]), _lib.ptr(cols[2]), _lib.ptr(keep[4]), N,
            None, N, 15, _lib.ptr(off), _lib.ptr(keep[5]), _lib.ptr(keep[6]), _lib.ptr(keep[7]),
            int(off[-1])]
    return names, vals, keep


def test_launch_argument_checks_need_no_device():
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    before = [_lib.launch_count(k) for k in KERNELS]

    def err():
        return L.airice_last_error().decode()

    for fn, (names, vals, keep), poison in (
            (L.airice_icepath_launch, _launch_args(), "work_bytes"),
            (L.airice_icepath_host, _host_args(), "cap")):
        at = {name: k for k, name in enumerate(names)}
        # the poison: an argument refused after the null and stride checks, so a check that went
        # missing shows as a failed assertion, never as a kernel started on a wild address
        base = list(vals)
        base[at[poison]] -= 1
        assert fn(*base) == -1 and poison.split("_")[0] in err(), err()
        required = [name for name in names
                    if name not in ("model3", "status", "stream", "n", "ray_mask", "ld_rays",
                                    "work_bytes", "cap")]
        for name in required:  # each required pointer null in turn
            a = list(base)
            a[at[name]] = None
            assert fn(*a) == -1, name
            assert f"({name})" in err(), (name, err())
        a = list(base)  # a short stride, with both numbers
        a[at["ld_rays"]] = N - 1
        assert fn(*a) == -1 and "ld_rays" in err() and str(N - 1) in err(), err()
        a = list(base)  # n == 0 is AIRICE_OK whatever else is passed
        a[at["n"]] = 0
        assert fn(*a) == 0
        assert fn(*[0 if isinstance(v, int) else None for v in vals]) == 0
    # the launch alone: cap and work_bytes one short, offsets that are not the plan's, a
    # misaligned workspace
    names, vals, (z0, z1, off) = _launch_args()
    at = {name: k for k, name in enumerate(names)}
    for name in ("cap", "work_bytes"):
        a = list(vals)
        a[at[name]] -= 1
        assert L.airice_icepath_launch(*a) == -1 and name in err(), (name, err())
    wrong = off.copy()
    wrong[5] += 1
    a = list(vals)
    a[at["offsets"]] = _lib.ptr(wrong)
    a[at["work_bytes"]] -= 1
    assert L.airice_icepath_launch(*a) == -1 and "offsets[5]" in err(), err()
    a = list(vals)
    a[at["d_work"]] = ctypes.c_void_p(0x100008)
    a[at["work_bytes"]] -= 1
    assert L.airice_icepath_launch(*a) == -1 and "d_work" in err(), err()
    # the plan: offsets is required, the depths when there are pairs
    assert L.airice_icepath_plan(None, None, None, 0, 15, None, None) == -1 and "(offsets)" in err()
    assert L.airice_icepath_plan(None, _lib.ptr(z1), None, N, 15, _lib.ptr(off), None) == -1
    assert "(z0)" in err()
    assert [_lib.launch_count(k) for k in KERNELS] == before
