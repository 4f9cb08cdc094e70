"""The two-layer (double-exponential) firn on the host route (airice_rays_host_firn, airice_nz_firn
and the argument checks of every *_firn entry point): no kernel is launched here.

The reference of a layered ray is the composition of three one-layer oracle rays
(tests/firn_cases.py); 64 rays are also checked against 30-digit mpmath quadrature of the three
path integrals, which shares no closed form with the library or the oracle.
Bound: the project's parity rule (tests/parity.py: 1e-9 relative with the per-slot floors).
"""
import ctypes
import math

import numpy as np
import pytest

import oracle
from tests import firn_cases as fc
from tests import parity

N_RAYS = 2000
C_LIGHT = 299792458.0


@pytest.fixture(scope="module")
def solver():
    from airiceraytracing_amd import AirIceSolver
    return AirIceSolver()


@pytest.fixture(scope="module")
def firn():
    from airiceraytracing_amd import Firn
    return Firn.summit()


@pytest.fixture(scope="module")
def summit(solver):
    """The library medium with the Summit A_ice (B_ice / C_ice left at the defaults: ignored)."""
    return fc.lib_medium(solver.medium)


@pytest.fixture(scope="module")
def one_layer(solver):
    """(A, B[0], C[0]) as a one-layer medium."""
    return fc.lib_medium(solver.medium, B=fc.SUMMIT_B[0], C=fc.SUMMIT_C[0])


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def rays_firn(m, f, launch, txh, depth, in_ice=1, ice_m=fc.ICE_M):
    """airice_rays_host_firn with a per-ray depth (one call per distinct depth)."""
    from airiceraytracing_amd import _lib
    launch, txh = np.ascontiguousarray(launch), np.ascontiguousarray(txh)
    depth = np.broadcast_to(np.asarray(depth, dtype=np.float64), launch.shape)
    out = np.empty((18, launch.size))
    for d in np.unique(depth):
        sel = np.flatnonzero(depth == d)
        a, h = np.ascontiguousarray(launch[sel]), np.ascontiguousarray(txh[sel])
        o = np.empty((18, sel.size))
        _lib.check(_lib.lib().airice_rays_host_firn(ctypes.byref(m), ctypes.byref(f), _ptr(a),
                                                    _ptr(h), ice_m, float(d), in_ice, sel.size,
                                                    _ptr(o), sel.size), "airice_rays_host_firn")
        out[:, sel] = o
    return out


def rays_one_layer(m, launch, txh, depth, in_ice=1, ice_m=fc.ICE_M):
    from airiceraytracing_amd import _lib
    launch, txh = np.ascontiguousarray(launch), np.ascontiguousarray(txh)
    depth = np.broadcast_to(np.asarray(depth, dtype=np.float64), launch.shape)
    out = np.empty((18, launch.size))
    for d in np.unique(depth):
        sel = np.flatnonzero(depth == d)
        a, h = np.ascontiguousarray(launch[sel]), np.ascontiguousarray(txh[sel])
        o = np.empty((18, sel.size))
        _lib.check(_lib.lib().airice_rays_host(ctypes.byref(m), _ptr(a), _ptr(h), ice_m, float(d),
                                               in_ice, sel.size, _ptr(o), sel.size),
                   "airice_rays_host")
        out[:, sel] = o
    return out


@pytest.fixture(scope="module")
def drawn(summit, firn):
    launch, txh, depth = fc.draw(N_RAYS)
    return launch, txh, depth, rays_firn(summit, firn, launch, txh, depth)


def test_index(summit, firn):
    """airice_nz_firn is A + B[l] exp(-C[l] z) with the upper layer at z == boundary_m.  The
    library and this formula each round one exp and one product-sum: 2 ulp of n ~ 1.5."""
    from airiceraytracing_amd import _lib
    nz = _lib.lib().airice_nz_firn
    b = firn.boundary_m
    for z in (0.0, 1.0, 14.0, b, np.nextafter(b, np.inf), 15.0, 100.0, 2000.0):
        layer = 0 if z <= b else 1
        want = fc.SUMMIT_A + fc.SUMMIT_B[layer] * math.exp(-fc.SUMMIT_C[layer] * z)
        got = nz(ctypes.byref(summit), ctypes.byref(firn), z)
        assert abs(got - want) <= 2 * np.spacing(want), (z, got, want)
        assert nz(ctypes.byref(summit), ctypes.byref(firn), -z) == got  # |z|, as airice_nz_ice
    up = fc.SUMMIT_A + fc.SUMMIT_B[0] * math.exp(-fc.SUMMIT_C[0] * b)
    low = fc.SUMMIT_A + fc.SUMMIT_B[1] * math.exp(-fc.SUMMIT_C[1] * b)
    assert abs(up - low) > 1e-4  # the two layers differ at the boundary, so the layer matters
    assert abs(nz(ctypes.byref(summit), ctypes.byref(firn), b) - up) <= 2 * np.spacing(up)


def test_composition(drawn, one_layer, oracle_medium):
    launch, txh, depth, got = drawn
    # the ice leg is never NaN; a few grazing rays from just above the ice are NaN in their air
    # part (in the oracle too: compare_columns wants the NaN positions identical)
    assert not np.isnan(got[[4, 7, 10, 13, 17]]).any()
    assert np.isnan(got).any(axis=0).mean() < 0.02
    ref = fc.compose_rays(oracle_medium, launch, txh, depth)
    cols = list(fc.COMPOSED_COLUMNS)
    rep = parity.compare_columns(got[cols], ref[cols], parity.RAY_FLOORS[cols])
    print(f"[firn composition] {N_RAYS} rays, columns {cols}: max_rel={rep['max_rel']:.3e} "
          f"per column {['%.1e' % v for v in rep['max_rel_per_col']]}")
    assert rep["ok"], rep
    # what does not read the ice below the surface is the one-layer call's, bit for bit (its own
    # parity with the oracle is the business of the one-layer tests)
    upper = rays_one_layer(one_layer, launch, txh, depth)
    for c in fc.UPPER_COLUMNS:
        assert np.array_equal(got[c].view(np.uint64), upper[c].view(np.uint64)), c
    assert not np.array_equal(got[4], upper[4])  # and the ice leg is not


def test_quadrature(drawn, summit, firn):
    """64 of the rays against 30-digit quadrature of int L/sqrt(n^2-L^2), int n^2/sqrt(n^2-L^2) / c,
    int n/sqrt(n^2-L^2) over the depth and asin(L/n) at the antenna, L from column 12 (the
    incidence on the ice) and airice_nz_air."""
    import mpmath as mp
    from airiceraytracing_amd import _lib
    launch, txh, depth, got = drawn
    mp.mp.dps = 30
    n_air = _lib.lib().airice_nz_air(ctypes.byref(summit), fc.ICE_M)
    A, b = mp.mpf(fc.SUMMIT_A), mp.mpf(fc.SUMMIT_BOUNDARY)
    pi = mp.mpf(summit.pi)  # the variant's pi: the library's degrees are 180 / 3.1415927 radians

    def n_of(z):
        layer = 0 if z <= b else 1
        return A + mp.mpf(fc.SUMMIT_B[layer]) * mp.exp(-mp.mpf(fc.SUMMIT_C[layer]) * z)

    worst = np.zeros(4)
    for k in np.linspace(0, N_RAYS - 1, 64).astype(int):
        L = mp.mpf(n_air) * mp.sin(mp.mpf(got[12, k]) * pi / 180)
        d = mp.mpf(-depth[k])
        root = lambda z: mp.sqrt(n_of(z) ** 2 - L * L)
        want = [mp.quad(lambda z: L / root(z), [0, b, d]),
                mp.quad(lambda z: n_of(z) ** 2 / root(z), [0, b, d]),  # c * t
                mp.quad(lambda z: n_of(z) / root(z), [0, b, d]),
                mp.asin(L / n_of(d)) * 180 / pi]
        for j, c in enumerate((4, 7, 17, 13)):
            scale = max(abs(float(want[j])), parity.RAY_FLOORS[c])
            worst[j] = max(worst[j], abs(float(mp.mpf(got[c, k]) - want[j])) / scale)
    print(f"[firn quadrature] 64 rays, max rel of columns 4, 7, 17, 13: {worst}")
    assert (worst <= parity.RTOL).all(), worst


@pytest.mark.parametrize("depth,in_ice", [(-14.9, 1), (-5.0, 1), (-0.0, 1), (-100.0, 0),
                                          (-14.9000001, 0), (3.0, 0)])
def test_routing(summit, one_layer, firn, depth, in_ice):
    """At or above the boundary, or with in_ice = 0, all 18 columns are the one-layer call's."""
    launch, txh, _ = fc.draw(200, seed=7)
    if depth > 0:
        txh = txh + depth
    got = rays_firn(summit, firn, launch, txh, depth, in_ice)
    want = rays_one_layer(one_layer, launch, txh, depth, in_ice)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_equal_layers(solver, oracle_medium):
    """B[0] = B[1], C[0] = C[1]: the two legs add up to the one-layer ray within the bound."""
    from airiceraytracing_amd import Firn
    m = solver.medium
    f = Firn(14.9, (ctypes.c_double * 2)(m.B_ice, m.B_ice), (ctypes.c_double * 2)(m.C_ice, m.C_ice))
    launch, txh, depth = fc.draw(N_RAYS, seed=11)
    got = rays_firn(m, f, launch, txh, depth)
    want = rays_one_layer(m, launch, txh, depth)
    rep = parity.compare_columns(got, want, parity.RAY_FLOORS)
    print(f"[firn equal layers] max_rel={rep['max_rel']:.3e}")
    assert rep["ok"], rep


def _bad_firns():
    from airiceraytracing_amd import Firn

    def make(**kw):
        f = Firn.summit()
        for k, v in kw.items():
            if k == "boundary_m":
                f.boundary_m = v
            else:
                getattr(f, k[0])[int(k[1])] = v
        return f
    nan, inf = float("nan"), float("inf")
    return [("null", None), ("boundary 0", make(boundary_m=0.0)),
            ("boundary < 0", make(boundary_m=-14.9)), ("boundary nan", make(boundary_m=nan)),
            ("boundary inf", make(boundary_m=inf)), ("B0 nan", make(B0=nan)),
            ("B1 inf", make(B1=inf)), ("C0 0", make(C0=0.0)), ("C1 < 0", make(C1=-0.02)),
            ("C0 nan", make(C0=nan)), ("C1 inf", make(C1=inf))]


def test_arguments(summit):
    """Every invalid firn returns AIRICE_EINVAL from every *_firn entry point with a message, and
    nothing is written; so do the namesakes' own invalid arguments."""
    from airiceraytracing_amd import _lib, make_grid
    L = _lib.lib()
    g = make_grid(-10000.0, fc.ICE_M * 100.0, 2000.0, 90.1, 180.0, 0.7)
    n = g.n_rays
    a, h = np.full(4, 120.0), np.full(4, 5000.0)
    m = ctypes.byref(summit)
    fake = ctypes.c_void_p(4096)  # a device pointer that is never dereferenced: the check is first
    fakes = (ctypes.c_void_p * 1)(4096)
    lds = (ctypes.c_size_t * 1)(n)
    for name, f in _bad_firns():
        fp = None if f is None else ctypes.byref(f)
        out = np.full((18, 4), 7.0)
        tab = np.full((11, n), 7.0, dtype=np.float32)
        calls = {
            "rays_host": L.airice_rays_host_firn(m, fp, _ptr(a), _ptr(h), fc.ICE_M, -100.0, 1, 4,
                                                 _ptr(out), 4),
            "rays_launch": L.airice_rays_launch_firn(m, fp, fake, fake, fc.ICE_M, -100.0, 1, 4,
                                                     fake, 4, None),
            "table_host": L.airice_table_host_firn(m, fp, ctypes.byref(g), 0, g.table_rows,
                                                   _ptr(tab), None, n),
            "table_launch": L.airice_table_launch_firn(m, fp, ctypes.byref(g), 0, g.table_rows,
                                                       fake, None, n, None),
            "table_multi": L.airice_table_launch_multi_firn(m, fp, ctypes.byref(g), 1, fakes, lds,
                                                            None),
        }
        for call, rc in calls.items():
            assert rc == -1, (name, call, rc)
        assert b"firn" in L.airice_last_error(), (name, L.airice_last_error())
        assert (out == 7.0).all() and (tab == 7.0).all(), name
    # the namesakes' checks still hold with a valid firn
    f = ctypes.byref(_lib.Firn.summit())
    out = np.full((18, 4), 7.0)
    assert L.airice_rays_host_firn(None, f, _ptr(a), _ptr(h), fc.ICE_M, -100.0, 1, 4, _ptr(out),
                                   4) == -1
    assert L.airice_rays_host_firn(m, f, None, _ptr(h), fc.ICE_M, -100.0, 1, 4, _ptr(out), 4) == -1
    assert L.airice_rays_host_firn(m, f, _ptr(a), _ptr(h), fc.ICE_M, -100.0, 1, 4, _ptr(out),
                                   3) == -1
    assert L.airice_rays_launch_firn(m, f, None, fake, fc.ICE_M, -100.0, 1, 4, fake, 4, None) == -1
    assert L.airice_table_launch_firn(m, f, ctypes.byref(g), 40, 20, fake, None, n, None) == -1
    assert L.airice_table_launch_firn(m, f, ctypes.byref(g), 0, 1, None, None, n, None) == -1
    assert (out == 7.0).all()


def test_sanitizer_program():
    """The firn's host code (the check, the lower leg's constants, the layered host ray route)
    under ASan + UBSan as a program of its own (tests/cpp/firn_driver.cpp)."""
    import os
    import subprocess
    from tests.conftest import ROOT
    exe = os.path.join(ROOT, "tests", "cpp", "firn_driver_asan")
    assert os.path.exists(exe), "built by `make -C airiceraytracing_amd/csrc firn_driver_asan`"
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "firn_driver ok" in run.stdout and "runtime error" not in run.stderr
