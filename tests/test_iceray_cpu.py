"""The in-ice ray solver (airice_iceray_launch / airice_iceray_host, include/IceRayTracing.hh)
without a GPU: header and exports, the launch's argument checks, one row per decision path, the
physics of every accepted ray by numerical integration (no oracle, no shared formula), the host
route bit for bit against the IceRayTracing:: drop-in, and the drop-in's caller under ASan + UBSan
as its own program."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import iceray_cases as cases
from tests.conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "cpp", "iceray_driver")
DRIVER_ASAN = os.path.join(ROOT, "tests", "cpp", "iceray_driver_asan")
N_PHYSICS = 2000
N_BITS = 5000


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


@pytest.fixture(scope="module")
def class_rows(solver):
    q = cases.class_queries()
    out, st = cases.host_rows(solver, q)
    for a in (q, out, st):
        a.setflags(write=False)
    return q, out, st


@pytest.fixture(scope="module")
def drawn_rows(solver):
    """5,000 drawn rows on the host route, computed once; the first 2,000 serve the physics."""
    q = cases.drawn(N_BITS, np.random.default_rng(2027))
    out, st = cases.host_rows(solver, q)
    for a in (q, out, st):
        a.setflags(write=False)
    return q, out, st


def _driver_rows(program, q, tmp_path):
    """The driver's IceRayTracing() values (n, 29) and its D / R / A lines for rows q."""
    path = os.path.join(tmp_path, "rows.bin")
    np.ascontiguousarray(q, dtype=np.float64).tofile(path)
    run = subprocess.run([program, path], capture_output=True, text=True, check=True)
    assert run.stderr == "", run.stderr
    got = {"I": {}, "D": {}, "R": {}, "A": {}}
    for line in run.stdout.splitlines():
        tag, row, *words = line.split()
        got[tag][int(row)] = np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)
    return got


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    for name in ("airice_iceray_launch", "airice_iceray_host"):
        assert f"int {name}(const double *model3" in header, name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert "#define AIRICE_ICERAY_FIELDS 32" in header
    assert _lib.launch_count("iceray_kernel") >= 0  # the counter and the timer exist
    assert _lib.kernel_time("iceray_kernel", reset=False) == (0.0, 0)
    with open(os.path.join(ROOT, "include", "IceRayTracing.hh")) as f:
        dropin = f.read()
    for name in ("SetA", "SetB", "SetC", "GetB", "GetC", "Getnz", "Refl_S", "Trans_S", "Refl_P",
                 "Trans_P", "GetZmax", "fDnfR", "fDnfR_L", "ftimeD", "fpathD", "fDa", "fRa", "fRaa",
                 "GetDirectRayPar", "GetReflectedRayPar", "GetRefractedRayPar", "IceRayTracing",
                 "IceRayTracingBatch"):
        assert f"{name}(" in dropin, name
    assert (_lib.ICERAY_FIELDS, _lib.ICERAY_LVALUE, _lib.ICERAY_STATUS) == (32, 19, 29)
    from airiceraytracing_amd import AirIceSolver
    assert callable(AirIceSolver.ice_rays_device) and callable(AirIceSolver.ice_rays_host)


def test_launch_argument_checks_need_no_device():
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a device call
    before = _lib.launch_count("iceray_kernel")
    assert L.airice_iceray_launch(None, None, None, None, 0, None, 0, None, None) == 0  # n == 0
    for i, name in ((1, "z0"), (2, "x1"), (3, "z1"), (5, "out")):
        a = [None, p, p, p, 8, p, 8, None, None]
        a[i] = None
        assert L.airice_iceray_launch(*a) == -1, name  # AIRICE_EINVAL
        assert f"({name})" in L.airice_last_error().decode(), (name, L.airice_last_error())
    assert L.airice_iceray_launch(None, p, p, p, 8, p, 7, None, None) == -1
    assert "ld" in L.airice_last_error().decode()
    # the host form checks the same before it allocates or launches
    assert L.airice_iceray_host(None, None, None, None, 0, None, 0, None) == 0
    assert L.airice_iceray_host(None, p, None, p, 8, p, 8, None) == -1
    assert "(x1)" in L.airice_last_error().decode()
    assert L.airice_iceray_host(None, p, p, p, 8, p, 7, None) == -1
    assert _lib.launch_count("iceray_kernel") == before


def test_class_rows_are_their_class(class_rows):
    q, out, st = class_rows
    for i, (row, status, why) in enumerate(cases.CLASS_ROWS):
        assert st[i] == status == int(out[i, cases.STATUS]), (row, st[i], why)
        for ray in range(4):  # the -1000 flag of a ray that does not exist, and zeroed leg times
            if not status & (1 << ray):
                assert out[i, cases.RANG + ray] == -1000.0, (row, ray)
                if ray:
                    assert out[i, 10 + 2 * ray] == 0.0 and out[i, 11 + 2 * ray] == 0.0
    assert len({s for _, s, _ in cases.CLASS_ROWS}) >= 7  # distinct classes
    # the first row: the known direct ray
    assert abs(out[0, cases.LVALUE] - 1.33384) < 1e-5 and out[0, cases.ITERS] == 8
    assert abs(out[0, cases.TIME] - 7.299694880677e-07) < 1e-12 * 7.3e-07 + 1.78e-6 / cases.C_LIGHT
    assert out[0, cases.EVALS] < 60
    # the second: D's residual is NaN, the refracted ray turns above the Rx
    assert abs(out[1, cases.LVALUE + 2] - 1.66369) < 1e-5
    assert abs(out[1, cases.ZMAX] - 99.05) < 0.01 and out[1, cases.ZMAX] < 100.0
    # equal depths: flagged, not trapped, and the flat residual ends the search at once
    assert not st[7] & cases.D and out[7, cases.EVALS] < 100
    # the flip (rows 1 and 8): angles are 180 - each other's, leg times swap, the rest is equal
    a, b = out[1], out[8]
    for ray in (1, 2):
        assert b[cases.LANG + ray] == 180 - a[cases.RANG + ray]
        assert b[cases.RANG + ray] == 180 - a[cases.LANG + ray]
        assert (b[10 + 2 * ray], b[11 + 2 * ray]) == (a[11 + 2 * ray], a[10 + 2 * ray])
        for col in (cases.TIME, cases.LVALUE, cases.PATH):
            assert b[col + ray] == a[col + ray]


def test_edge_and_nonfinite_inputs(solver):
    out, st = cases.host_rows(solver, np.array(cases.EDGE_ROWS))
    assert np.array_equal(st, out[:, cases.STATUS].astype(np.int64))
    assert (out[:, cases.EVALS] <= 9 * 100 * 10).all() and not (st & cases.NONFINITE).any()
    # z0 = 0 and z1 = 0 are each other's flip; x1 = 0 between two depths and x1 < 0: no ray;
    # all three zero is the empty ray, whose residuals are 0 at the first end
    assert st.tolist() == [3, 3, 0, 3, 0], st
    assert cases.same_bits(out[0, cases.TIME:cases.TIME + 2], out[1, cases.TIME:cases.TIME + 2])
    out, st = cases.host_rows(solver, cases.nonfinite_queries())
    assert (st == cases.NONFINITE).all() and (out[:, cases.STATUS] == 128).all()
    assert np.isnan(out[:, :29]).all() and (out[:, 30:] == 0).all()


def test_other_ice_model(solver):
    q = cases.class_queries()[:3]
    ref, _ = cases.host_rows(solver, q)
    same, _ = cases.host_rows(solver, q, model=(1.78, -0.43, 0.0132))
    assert cases.same_bits(ref, same)
    other, st = cases.host_rows(solver, q, model=(1.775, -0.45, 0.014))
    assert st[0] == cases.D | cases.R and not cases.same_bits(ref[0], other[0])
    n0 = 1.775 - 0.45 * math.exp(-0.014 * 180.0)
    assert other[0, cases.LANG] == math.asin(other[0, cases.LVALUE] / n0) * (180.0 / cases.PI_REF)


def test_physics_of_accepted_rays(class_rows, drawn_rows):
    """Every accepted ray of the class rows and of 2,000 drawn rows, integrated by mpmath.quad at
    30 digits over the ray's legs: reach = x1 within |checkzero| + 1e-9 x1, time within
    1.78e-6/c + 1e-12 t, geometric path within 1e-6 + 1e-12 s."""
    q = np.concatenate([class_rows[0], drawn_rows[0][:N_PHYSICS]])
    out = np.concatenate([class_rows[1], drawn_rows[1][:N_PHYSICS]])
    st = np.concatenate([class_rows[2], drawn_rows[2][:N_PHYSICS]])
    rows = np.array(cases.physics_errors(q, out, st))
    print(f"[iceray physics] {len(rows)} rays of {len(q)} rows: worst reach {rows[:, 2].max():.2e} m "
          f"(of its bound {np.max(rows[:, 2] / rows[:, 3]):.2f}), time {rows[:, 4].max():.2e} s "
          f"({np.max(rows[:, 4] / rows[:, 5]):.2e}), path {rows[:, 6].max():.2e} m "
          f"({np.max(rows[:, 6] / rows[:, 7]):.2e})")
    for ray in range(4):
        assert (rows[:, 1] == ray).sum() >= 10, ray  # every kind of ray is among them
    for err, bound, what in ((2, 3, "reach"), (4, 5, "time"), (6, 7, "path")):
        bad = rows[rows[:, err] > rows[:, bound]]
        assert len(bad) == 0, (what, bad[:5], q[bad[:5, 0].astype(int)])


def test_angles_and_time_order(class_rows, drawn_rows):
    q = np.concatenate([class_rows[0], drawn_rows[0]])
    out = np.concatenate([class_rows[1], drawn_rows[1]])
    st = np.concatenate([class_rows[2], drawn_rows[2]])
    deg = 180.0 / cases.PI_REF
    n_tx, n_rx = cases.nz(q[:, 0]), cases.nz(q[:, 2])
    flip = q[:, 0] > q[:, 2]
    for ray in range(4):
        ok = (st & (1 << ray)) != 0
        L = out[:, cases.LVALUE + ray]
        with np.errstate(invalid="ignore"):
            at_tx, at_rx = np.arcsin(L / n_tx) * deg, np.arcsin(L / n_rx) * deg
        # the solver works Tx-below-Rx: launch = asin(L/n) at the lower end, receive = asin at the
        # upper (180 - it for a ray that arrives from above), and reports 180 - each when flipped
        up = at_rx if ray == 0 else 180 - at_rx
        lang = np.where(flip, 180 - np.where(ray == 0, at_tx, 180 - at_tx), at_tx)
        rang = np.where(flip, 180 - at_rx, up)
        # numpy's asin and the C library's may differ in the last place
        assert np.allclose(out[ok, cases.LANG + ray], lang[ok], rtol=0, atol=1e-11), ray
        assert np.allclose(out[ok, cases.RANG + ray], rang[ok], rtol=0, atol=1e-11), ray
    both = (st & 3) == 3
    assert both.sum() > 1000 and (out[both, cases.TIME] < out[both, cases.TIME + 1]).all()
    for ray in (2, 3):
        m = ((st & 1) != 0) & ((st & (1 << ray)) != 0)
        assert (out[m, cases.TIME] < out[m, cases.TIME + ray]).all()
    inc = (st & 2) != 0
    assert np.allclose(out[inc, cases.INCIDENCE],
                       np.arcsin(out[inc, cases.LVALUE + 1] / cases.nz(1e-7)) * deg, atol=1e-11)


def test_host_route_is_the_drop_in_bit_for_bit(class_rows, drawn_rows, tmp_path):
    q = np.concatenate([class_rows[0], np.array(cases.EDGE_ROWS), cases.nonfinite_queries(),
                        drawn_rows[0]])
    n_head = len(q) - len(drawn_rows[0])
    from airiceraytracing_amd import AirIceSolver
    head, _ = cases.host_rows(AirIceSolver(), q[:n_head])
    out = np.concatenate([head, drawn_rows[1]])
    got = _driver_rows(DRIVER, q, str(tmp_path))
    assert len(got["I"]) == len(q)
    for i in range(len(q)):
        assert cases.same_bits(got["I"][i], out[i, :29]), (i, q[i])
    # the three *RayPar functions return what IceRayTracing assembles
    finite = np.isfinite(q).all(axis=1)
    for i in np.flatnonzero(finite)[:600]:
        d, r, o = got["D"][i], got["R"][i], out[i]
        assert cases.same_bits(d[[1, 2, 3, 5]], o[[0, 4, 19, 25]]), i
        assert cases.same_bits(r[[1, 2, 3, 7, 8]], o[[1, 5, 20, 18, 26]]), i
        assert (abs(d[4]) < 0.5) == bool(int(o[cases.STATUS]) & 1)
        if abs(r[4]) > 0.5 or abs(d[4]) > 0.5:
            a = got["A"][i]
            assert cases.same_bits(a[[1, 2, 3, 7, 16]], o[[2, 6, 21, 23, 27]]), i
        else:
            assert i not in got["A"]


def test_getzmax_is_the_root_of_the_reference_equation():
    from airiceraytracing_amd import _lib
    f = getattr(_lib.lib(), "_ZN13IceRayTracing7GetZmaxEdd")
    f.argtypes, f.restype = [ctypes.c_double, ctypes.c_double], ctypes.c_double
    import mpmath as mp
    for L in np.linspace(1.3501, 1.7799, 400):
        z = f(cases.A, float(L))
        with mp.workdps(30):  # the root of A + B exp(-C z) - L by its own search
            ref = mp.findroot(lambda x: cases.A + cases.B * mp.exp(-cases.C * x) - mp.mpf(float(L)),
                              (0, 5000), solver="illinois", tol=1e-26, maxsteps=400)
        assert abs(z - float(ref)) <= 1e-12 * float(ref), (L, z, ref)
    assert f(cases.A, 1.78) == -1000.0 and f(cases.A, 1.35) == -1000.0 and f(cases.A, 2.0) == -1000.0


def test_driver_under_sanitizers(class_rows, tmp_path):
    """tests/cpp/iceray_driver.cpp with the drop-in and the host route compiled in under ASan and
    UBSan (its own program, nothing preloaded): clean on the class rows and the tour, and the same
    bits as the library."""
    run = subprocess.run([DRIVER_ASAN], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lib = subprocess.run([DRIVER], capture_output=True, text=True, check=True)
    assert run.stdout == lib.stdout
    lines = [ln.split() for ln in run.stdout.splitlines()]
    rows = {int(ln[1]): ln[2:] for ln in lines if ln[0] == "I" and int(ln[1]) < 7}
    mine = {tuple(q): o for q, o in zip(map(tuple, class_rows[0]), class_rows[1])}
    shown = [(-180, 100, -100), (-180, 500, -100), (-1000, 2000, -200), (-200, 1000, -150),
             (-50, 300, -20), (-100, 50, -100), (-100, 500, -180)]
    for i, q in enumerate(shown):
        if tuple(map(float, q)) in mine:
            got = np.array([int(w, 16) for w in rows[i]], dtype=np.uint64).view(np.float64)
            assert cases.same_bits(got, mine[tuple(map(float, q))][:29]), q
    tour = {ln[1]: ln[2] for ln in lines if ln[0] == "T"}
    assert tour["Refl_S(1.2)"] == "3ff0000000000000" and tour["Trans_P(1.2)"] == "0" * 16
    assert tour["fDnfR(100)"] == tour["fDnfR_L(1.3)"]  # the same point of the same surface
    assert tour["fRaa(1.9)"] == "41cdcd6500000000"  # 1e9: no turning depth
    assert tour["Getnz(-100)'"] != tour["Getnz(-100)"]  # SetA / SetB / SetC took
