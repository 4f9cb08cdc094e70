"""The two-ray solutions (airice_icesol_launch / airice_icesol_host, the drop-in's
GetRayTracingSolutions / GetFocusingFactor and attenuation functions) without a GPU: header and
exports, the argument checks, the choice and ordering against a plain-Python restatement bit for
bit, the attenuation against mpmath.quad, the focusing factors against the formula, the host route
bit for bit against the drop-in, and the drop-in's caller under ASan + UBSan as its own program."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests import iceray_cases as rays
from tests import icesol_cases as cases
from tests.conftest import ROOT

DRIVER = os.path.join(ROOT, "tests", "cpp", "icesol_driver")
DRIVER_ASAN = os.path.join(ROOT, "tests", "cpp", "icesol_driver_asan")
N_CHOICE = 2000
N_ATT = 200


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


@pytest.fixture(scope="module")
def drawn_rows(solver):
    """2,000 drawn rows and their solver rows on the host route, computed once."""
    q = rays.drawn(N_CHOICE, np.random.default_rng(2907))
    ray_rows, _ = rays.host_rows(solver, q)
    for a in (q, ray_rows):
        a.setflags(write=False)
    return q, ray_rows


@pytest.fixture(scope="module")
def att_rows(solver, drawn_rows):
    """The class rows and the first 200 drawn rows with their solver rows: the attenuation and
    focusing checks."""
    q = np.concatenate([rays.class_queries(), drawn_rows[0][:N_ATT]])
    ray_rows = np.concatenate([rays.host_rows(solver, rays.class_queries())[0],
                               drawn_rows[1][:N_ATT]])
    for a in (q, ray_rows):
        a.setflags(write=False)
    return q, ray_rows


def test_header_declares_and_lib_exports():
    from airiceraytracing_amd import AirIceSolver, _lib
    with open(os.path.join(ROOT, "include", "airice.h")) as f:
        header = f.read()
    for name in ("airice_icesol_launch", "airice_icesol_host"):
        assert f"int {name}(const double *model3" in header, name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert "#define AIRICE_ICESOL_FIELDS 18" in header
    assert _lib.launch_count("icesol_kernel") >= 0  # the counter and the timer exist
    assert _lib.kernel_time("icesol_kernel", reset=False) == (0.0, 0)
    with open(os.path.join(ROOT, "include", "IceRayTracing.hh")) as f:
        dropin = f.read()
    for name in ("GetIceTemperature", "GetIceAttenuationLength", "AttenuationIntegrand",
                 "IntegrateOverLAttn", "GetTotalAttenuationDirect", "GetTotalAttenuationReflected",
                 "GetTotalAttenuationRefracted", "GetRayTracingSolutions", "GetFocusingFactor",
                 "GetRayTracingSolutionsBatch"):
        assert f"{name}(" in dropin, name
    assert (_lib.ICESOL_FIELDS, _lib.ICESOL_ATTENUATION, _lib.ICESOL_FOCUSING) == (18, 12, 16)
    assert (_lib.ICESOL_SLOT0, _lib.ICESOL_STRAIGHT, _lib.ICESOL_FOCUS1, _lib.ICESOL_NONFINITE) \
        == (1, 4, 16, 128)
    assert callable(AirIceSolver.ice_solutions_device) and callable(AirIceSolver.ice_solutions_host)


def test_argument_checks_need_no_device():
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below returns before a device call
    counts = [_lib.launch_count(k) for k in ("icesol_kernel", "iceray_kernel")]

    def launch(**kw):
        a = dict(model=None, z0=p, x1=p, z1=p, rays=p, ld_rays=8, lower=None, ld_lower=0, n=8,
                 a0=1.0, f=0.1, out=p, ld=8, status=None, stream=None)
        a.update(kw)
        return L.airice_icesol_launch(*a.values()), L.airice_last_error().decode()

    assert launch(n=0, z0=None, x1=None, z1=None, rays=None, out=None)[0] == 0  # n == 0
    for name in ("z0", "x1", "z1", "rays", "out"):
        rc, msg = launch(**{name: None})
        assert rc == -1 and f"({name})" in msg, (name, msg)  # AIRICE_EINVAL
    for name, kw in (("ld", dict(ld=7)), ("ld_rays", dict(ld_rays=7)),
                     ("ld_lower", dict(lower=p, ld_lower=7))):
        rc, msg = launch(**kw)
        assert rc == -1 and f"{name} (7)" in msg, (name, msg)
    for bad in (math.nan, math.inf, -math.inf):
        rc, msg = launch(a0=bad)
        assert rc == -1 and "a0" in msg, msg
    for bad in (math.nan, math.inf, 0.0, -0.1):
        rc, msg = launch(f=bad)
        assert rc == -1 and "frequency_ghz" in msg, (bad, msg)
    for bad in ((1.78, 0.43, 0.0132), (1.78, -0.43, -0.0132), (1.78, 0.0, 0.0132),
                (1.78, -0.43, 0.0), (1.78, math.nan, 0.0132)):
        m = np.array(bad, dtype=np.float64)
        rc, msg = launch(model=_lib.ptr(m))
        assert rc == -1 and "model3" in msg, (bad, msg)
    # the host form checks the same before it allocates or launches
    H = L.airice_icesol_host
    assert H(None, None, None, None, 0, 1.0, 0.1, 1, None, 0, None) == 0
    assert H(None, p, None, p, 8, 1.0, 0.1, 1, p, 8, None) == -1
    assert "(x1)" in L.airice_last_error().decode()
    assert H(None, p, p, p, 8, 1.0, 0.1, 1, p, 7, None) == -1
    assert H(None, p, p, p, 8, math.nan, 0.1, 1, p, 8, None) == -1
    assert H(None, p, p, p, 8, 1.0, -1.0, 1, p, 8, None) == -1
    assert "frequency_ghz" in L.airice_last_error().decode()
    assert [_lib.launch_count(k) for k in ("icesol_kernel", "iceray_kernel")] == counts


def test_choice_is_the_reference_statement_by_statement(solver, drawn_rows):
    """The class, edge and non-finite rows and 2,000 drawn rows on the host route: every column
    but the attenuation and the focusing equals the Python restatement bit for bit, and so do the
    status bits."""
    head = rays.head_rows()
    q = np.concatenate([head, drawn_rows[0]])
    ray_rows = np.concatenate([rays.host_rows(solver, head)[0], drawn_rows[1]])
    got, st = cases.host_solutions(solver, q)
    want, want_st, _ = cases.choose_rows(q, ray_rows)
    assert np.array_equal(st, want_st), np.flatnonzero(st != want_st)[:5]
    bad = [i for i in range(len(q)) if not cases.same_choice(got[i:i + 1], want[i:i + 1])]
    assert not bad, (bad[:5], q[bad[:5]], got[bad[:1]], want[bad[:1]])
    assert np.array_equal(st & 3, (got[:, cases.IGNORE] + 2 * got[:, cases.IGNORE + 1]))
    # the non-finite rows
    nf = slice(len(head) - len(rays.nonfinite_queries()), len(head))
    assert (st[nf] == cases.NONFINITE).all()
    assert np.isnan(got[nf][:, [0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 16, 17]]).all()
    assert (got[nf][:, [8, 9, 14, 15]] == 0).all()
    # the class rows' types before the order by time, and who is ignored
    types = {rays.D | rays.R: {1, 2}, rays.R | rays.RA0: {3, 2}, rays.D | rays.RA0: {1, 3},
             rays.RA0 | rays.RA1: {3, 4}}
    for i, (row, status, why) in enumerate(rays.CLASS_ROWS):
        t, ig = got[i, cases.TYPE:cases.TYPE + 2], got[i, cases.IGNORE:cases.IGNORE + 2]
        if status in types:
            assert set(t) == types[status] and ig.tolist() == [1, 1], (row, t, ig)
            assert got[i, cases.TIME] <= got[i, cases.TIME + 1], row
        elif status == rays.RA0:
            assert t[0] == 3 and ig.tolist() == [1, 0], (row, t, ig)
        elif status == rays.D:
            assert t[0] == 1 and ig.tolist() == [1, 0], (row, t, ig)
        else:
            assert status == 0 and ig.tolist() == [0, 0], (row, ig)
    # every kind of pair is among the drawn rows, and the swap by time happens
    kinds = {tuple(sorted(t)) for t, s in zip(got[:, cases.TYPE:cases.TYPE + 2], st) if s & 3 == 3}
    assert {(1, 2), (2, 3), (1, 3), (3, 4)} <= kinds, kinds
    assert (got[:, cases.TYPE] > got[:, cases.TYPE + 1]).sum() > 10


def test_straight_line_rule(solver):
    """Equal depths where the solver leaves no time and no path: the straight line, and the
    emitter on top of the receiver ignored except for slot 0."""
    q = np.array([(-100.0, 0.3, -100.0), (-100.0, 0.0, -100.0)])
    ray_rows, _ = rays.host_rows(solver, q)
    assert (ray_rows[:, rays.TIME] == 0).all() and (ray_rows[:, rays.PATH] == 0).all()
    got, st = cases.host_solutions(solver, q, focusing=True)
    want, want_st, _ = cases.choose_rows(q, ray_rows)
    assert cases.same_choice(got, want) and np.array_equal(st & 7, want_st)
    assert (st & cases.STRAIGHT).all()
    assert got[0, cases.PATH] == 0.3 and got[0, cases.LANG] == got[0, cases.RANG] == 90.0
    assert got[0, cases.TIME] == 0.3 / (rays.C_LIGHT / (rays.A + rays.B * math.exp(-rays.C * 100)))
    assert got[0, cases.IGNORE:cases.IGNORE + 2].tolist() == [1, 1]
    assert got[1, cases.IGNORE:cases.IGNORE + 2].tolist() == [1, 0] and got[1, cases.PATH] == 0.0


def _check_attenuation(label, rows):
    """rows: (what, got Att, I by mpmath, mpmath's error estimate).  The issue's bound
    |Att - (1 - I)| <= 1e-9 I + 1e-15; the quadrature's own error estimate must be far inside it."""
    worst, at = 0.0, None
    for what, att, I, err in rows:
        bound = cases.attenuation_bound(I)
        assert err <= 0.01 * bound, (what, I, err)
        ratio = abs(att - (1 - I)) / bound if not math.isnan(att) else math.inf
        if ratio > worst:
            worst, at = ratio, what
    print(f"[icesol attenuation] {label}: {len(rows)} rays, worst |Att - (1 - I)| is "
          f"{worst:.3e} of its bound 1e-9 I + 1e-15, at {at}")
    assert worst <= 1.0, (worst, at)


def test_attenuation_of_accepted_rays_against_mpmath(solver, att_rows):
    """Each accepted ray the host route chose on the class rows and 200 drawn rows, at 0.1, 0.5
    and 2.0 GHz: |Att - (1 - I_mp)| <= 1e-9 I_mp + 1e-15, I_mp by mpmath.quad at 30 digits in z
    with the reference's integrand form.  Measured: the worst is 8.0e-5 of the bound."""
    q, ray_rows = att_rows
    _, _, src = cases.choose_rows(q, ray_rows)
    rows, seen = [], set()
    for f in cases.FREQUENCIES:
        got, _ = cases.host_solutions(solver, q, frequency=f)
        for i, (z0, x1, z1) in enumerate(q):
            for k in range(2):
                ray = src[i][k]
                if ray is None:
                    assert got[i, cases.ATT + k] == 0.0
                    continue
                assert got[i, cases.TYPE + k] == ray + 1
                seen.add(ray)
                I, err = cases.attenuation_mp(ray + 1, f, ray_rows[i, rays.LVALUE + ray], z0, z1)
                rows.append(((q[i].tolist(), f, ray), got[i, cases.ATT + k], I, err))
    assert seen == {0, 1, 2, 3}
    _check_attenuation("accepted rays", rows)


def test_total_attenuation_on_deep_and_grazing_legs():
    """GetTotalAttenuationDirect / Reflected / Refracted on 60 synthetic rays to 3000 m depth, the
    three frequencies in turn: direct rays, refracted rays (each leg to the turning depth) and
    reflected rays grazing the surface with L = 1.35 (1 - 10^u), u in [-12, 0]; A0 = 1 and, on
    every fourth, A0 = 0.37.  Measured: the worst is 6.5e-5 of the bound."""
    rng = np.random.default_rng(3000)
    rows = []
    for i in range(60):
        f = cases.FREQUENCIES[i % 3]
        a0 = 0.37 if i % 4 == 3 else 1.0
        za, zb = rng.uniform(1.0, 3000.0, 2)
        kind = i // 20
        if kind == 0:
            ray_type, L = 1, rng.uniform(1e-3, float(rays.nz(min(za, zb)))) * 0.999999
        elif kind == 1:
            ray_type, L = 3, rng.uniform(1.3501, float(rays.nz(min(za, zb))) * 0.999999)
        else:
            ray_type, L = 2, 1.35 * (1 - 10 ** rng.uniform(-12, 0))
        I, err = cases.attenuation_mp(ray_type, f, L, -za, -zb)
        got = cases.total_attenuation(ray_type, a0, f, -za, -zb, L)
        # the bound is on Att = 1 - A0 I; the function returns A0 I
        rows.append(((ray_type, f, a0, L, za, zb), 1 - got / a0, I, err))
    _check_attenuation("synthetic legs to 3000 m", rows)


def test_integrate_over_lattn():
    assert cases.integrate_over_lattn(1.0, 0.3, 150.0, 150.0, 1.3) == 0.0
    assert cases.integrate_over_lattn(1.0, 0.3, 1e-6, 1e-6, 1.2) == 0.0
    # between the limits it is given, in either order; A0 scales it
    a = cases.integrate_over_lattn(1.0, 0.3, 150.0, 40.0, 1.3)
    assert a > 0 and abs(cases.integrate_over_lattn(1.0, 0.3, 40.0, 150.0, 1.3) - a) <= 1e-15 * a
    I, err = cases.leg_mp(0.3, 1.3, 150.0, 40.0)
    assert abs(a - I) <= cases.attenuation_bound(I) and err < 1e-12 * I
    assert abs(cases.integrate_over_lattn(2.5, 0.3, 150.0, 40.0, 1.3) - 2.5 * a) <= 4e-16 * 2.5 * a
    # where the reference's integrand is NaN: a limit above the depth where n = L, or L >= A
    assert math.isnan(cases.integrate_over_lattn(1.0, 0.3, 150.0, 40.0, 1.6))
    assert math.isnan(cases.integrate_over_lattn(1.0, 0.3, 150.0, 40.0, 1.78))
    # the attenuation length model
    f = cases._dropin("_ZN13IceRayTracing23GetIceAttenuationLengthEdd", 2)
    t = cases._dropin("_ZN13IceRayTracing17GetIceTemperatureEd", 1)
    for z, fr in ((-150.0, 0.3), (-2000.0, 2.0), (40.0, 1.0)):
        d = abs(z)
        temp = 1.83415e-09 * d ** 3 + (-1.59061e-08 * d ** 2) + 0.00267687 * d + (-51.0696)
        assert abs(t(z) - temp) <= 1e-13 * abs(temp)
        w0, w1, w2, w = math.log(0.0001), 0.0, math.log(3.16), math.log(fr)
        b0 = -6.74890 + temp * (0.026709 - temp * 0.000884)
        b1 = -6.22121 - temp * (0.070927 + temp * 0.001773)
        b2 = -4.09468 - temp * (0.002213 + temp * 0.000332)
        if fr < 1:
            a_, bb = (b1 * w0 - b0 * w1) / (w0 - w1), (b1 - b0) / (w1 - w0)
        else:
            a_, bb = (b2 * w1 - b1 * w2) / (w1 - w2), (b2 - b1) / (w2 - w1)
        want = 1.0 / math.exp(a_ + bb * w)
        assert abs(f(z, fr) - want) <= 1e-12 * want, (z, fr)


def test_focusing_is_the_formula_on_the_two_solutions(solver, att_rows):
    """The class rows and 200 drawn rows: the focusing factors of the host route equal the
    reference's formula applied in Python to the host solutions at z1 and at z1 - 0.01 up to the
    last-place effects of sin and sqrt (4 ulp), with the same NaN and infinity positions."""
    q = att_rows[0]
    got, st = cases.host_solutions(solver, q, focusing=True)
    at, at_st = cases.host_solutions(solver, q)
    lower, _ = cases.host_solutions(solver, q - np.array([0.0, 0.0, 0.01]))
    assert cases.same_choice(got, at) and np.array_equal(st & 7, at_st)
    assert rays.same_bits(got[:, cases.ATT:cases.ATT + 2], at[:, cases.ATT:cases.ATT + 2])
    assert (at[:, cases.FOCUS:] == 0).all() and not (at_st & 24).any()
    worst, set_bits = 0.0, 0
    for i, (z0, x1, z1) in enumerate(q):
        f, bits = cases.focusing(z0, z1, at[i], lower[i])
        assert st[i] & 24 == bits, (q[i], st[i], bits)
        set_bits += bin(bits).count("1")
        for k in range(2):
            d = cases.ulps(got[i, cases.FOCUS + k], f[k])
            assert d <= 4, (q[i], k, got[i, cases.FOCUS + k], f[k])
            worst = max(worst, d)
    print(f"[icesol focusing] {len(q)} rows, {set_bits} factors set, worst {worst:.2f} ulp")
    assert set_bits > len(q)


def test_focusing_at_equal_depths(solver):
    """zR == zT: a factor 0 left at 0 becomes 1 (the emitter on top of the receiver, where the
    lower receiver's angle equals the straight line's 90 degrees and the factor is
    sqrt(0 / ...) = 0); 30 cm apart the formula's value stays."""
    got, st = cases.host_solutions(solver, np.array([(-100.0, 0.0, -100.0), (-100.0, 0.3, -100.0)]),
                                   focusing=True)
    at, _ = cases.host_solutions(solver, np.array([(-100.0, 0.3, -100.0)]))
    lower, _ = cases.host_solutions(solver, np.array([(-100.0, 0.3, -100.01)]))
    assert got[0, cases.FOCUS] == 1.0
    f, bits = cases.focusing(-100.0, -100.0, at[0], lower[0])
    assert st[1] & 24 == bits == 24
    assert cases.ulps(got[1, cases.FOCUS], f[0]) <= 4 and cases.ulps(got[1, cases.FOCUS + 1], f[1]) <= 4


def _driver_rows(program, q, a0, f, tmp_path):
    path = os.path.join(tmp_path, "rows.bin")
    np.ascontiguousarray(q, dtype=np.float64).tofile(path)
    run = subprocess.run([program, path, repr(a0), repr(f)], capture_output=True, text=True,
                         check=True)
    assert run.stderr == "", run.stderr
    got = {"S": {}, "F": {}}
    for line in run.stdout.splitlines():
        tag, row, *words = line.split()
        got[tag][int(row)] = np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)
    return got


def test_host_route_is_the_drop_in_bit_for_bit(solver, drawn_rows, tmp_path):
    """GetRayTracingSolutions and GetFocusingFactor of the drop-in against airice_icesol_host with
    n = 1 on the calling thread: the head rows, two equal-depth rows and 500 drawn rows."""
    q = np.concatenate([rays.head_rows(), [(-100.0, 0.3, -100.0), (-100.0, 0.0, -100.0)],
                        drawn_rows[0][:500]])
    for a0, f in ((1.0, 0.1), (0.8, 2.0)):
        got = _driver_rows(DRIVER, q, a0, f, str(tmp_path))
        mine, st = cases.host_solutions(solver, q, frequency=f, a0=a0)
        assert len(got["S"]) == len(q)
        for i in range(len(q)):
            assert rays.same_bits(got["S"][i], mine[i, :14]), (i, q[i])
    # GetFocusingFactor runs at A0 = 1, f = 0.1 GHz; a factor whose condition is not met is what
    # the caller left there (0 and 7 in the driver), but for the closing zR == zT rule
    foc, st = cases.host_solutions(solver, q, focusing=True)
    for i in range(len(q)):
        for k, bit in ((0, cases.FOCUS0), (1, cases.FOCUS1)):
            if st[i] & bit:
                assert rays.same_bits(got["F"][i][[k, 2 + k]], foc[i, [16 + k, 16 + k]]), (i, q[i])
            elif st[i] & cases.NONFINITE:
                assert got["F"][i][2 + k] == 7.0
            else:
                assert got["F"][i][2 + k] == 7.0 and got["F"][i][k] == foc[i, 16 + k], (i, q[i])


def test_driver_under_sanitizers(solver):
    """tests/cpp/icesol_driver.cpp with the drop-in and the host route compiled in under ASan and
    UBSan (its own program, nothing preloaded): clean, and the same bits as the library."""
    run = subprocess.run([DRIVER_ASAN], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lib = subprocess.run([DRIVER], capture_output=True, text=True, check=True)
    assert run.stdout == lib.stdout
    lines = [ln.split() for ln in run.stdout.splitlines()]
    q = rays.class_queries()
    mine, _ = cases.host_solutions(solver, q)
    for i in range(len(q)):
        words = next(ln[2:] for ln in lines if ln[0] == "S" and int(ln[1]) == i)
        got = np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)
        assert rays.same_bits(got, mine[i, :14]), q[i]
    tour = {ln[1]: ln[2] for ln in lines if ln[0] == "T"}
    assert tour["IntegrateOverLAttn(150,150)"] == "0" * 16
    assert tour["IntegrateOverLAttn(150,40)"] == tour["Direct"]
    assert tour["Refracted(L>=A)"].startswith("7ff") or tour["Refracted(L>=A)"].startswith("fff")
