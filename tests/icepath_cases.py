"""Geometries and independent checks for the in-ice ray-path samplers (airice_icepath_*, the
IceRayTracing::GetFull*RayPath drop-in): the shape rows, the host route ray by ray, a Python
restatement of the reference's running depth chain, and the physics check -- the horizontal
distance from the Tx along the ray to a sample by mpmath quadrature (iceray_cases.integrate_ray),
which shares no formula with the sampler beyond n(z) and Snell's invariant L."""
import ctypes

import numpy as np

from tests import iceray_cases as rc

H = 0.5
KINDS = 4

# x1 = 60, z1 = -50: the direct ray has 2, 256, 256 and 257 samples (z0 = -177 carries the duplicate
# closing sample), then equal depths; each followed by its flip.
_SHAPES = ((-50.3, 60.0, -50.0), (-177.0, 60.0, -50.0), (-177.25, 60.0, -50.0),
           (-177.5, 60.0, -50.0), (-50.0, 60.0, -50.0))
DIRECT_COUNTS = (2, 256, 256, 257, 2)
# R's first leg emits a sample at exactly 0
SURFACE_ROW = (-180.0, 100.0, -100.0)
# a refracted ray whose first leg holds a single sample: the host route puts its turning depth at
# 99.707 m, 0.29 m above the Rx (test_icepath_cpu checks it)
SINGLE_LEG1_ROW = (-180.0, 480.0, -100.0)


def shape_rows():
    rows = []
    for z0, x1, z1 in _SHAPES:
        rows.append((z0, x1, z1))
        rows.append((z1, x1, z0))
    rows.append(SURFACE_ROW)
    rows.append(SINGLE_LEG1_ROW)
    return np.array(rows, dtype=np.float64)


def head_rows():
    """Shape rows, then the solver's class, edge and non-finite rows: the head of every batch."""
    return np.concatenate([shape_rows(), rc.head_rows()])


def batch(n, rng):
    head = head_rows()
    if n <= len(head):
        return head[:n].copy()
    return np.concatenate([head, rc.drawn(n - len(head), rng)])


# ---- the host route ------------------------------------------------------------------------------
def one_host(kind, z0, x1, z1, L, zmax=0.0, model=None, cap=None):
    """airice_icepath_one_host: (x, z) of ray `kind` (0..3) on the calling thread."""
    from airiceraytracing_amd import _lib
    L_ = _lib.lib()
    m = None if model is None else np.ascontiguousarray(model, dtype=np.float64)
    cnt = ctypes.c_int64(0)
    if cap is None:  # ask for the count first
        L_.airice_icepath_one_host(_lib.ptr(m), 1 << kind, z0, x1, z1, L, zmax, None, None, 0,
                                   ctypes.byref(cnt))
        cap = cnt.value
    x, z = np.full(cap, np.nan), np.full(cap, np.nan)
    _lib.check(L_.airice_icepath_one_host(_lib.ptr(m), 1 << kind, z0, x1, z1, L, zmax, _lib.ptr(x),
                                          _lib.ptr(z), cap, ctypes.byref(cnt)),
               "airice_icepath_one_host")
    return x[:cnt.value], z[:cnt.value]


def host_paths(q, out, st, mask=15):
    """The host route over the solver's rows: {(row, ray): (x, z)} for every accepted ray in mask."""
    paths = {}
    for i, (z0, x1, z1) in enumerate(q):
        if st[i] & rc.NONFINITE:
            continue
        for ray in range(KINDS):
            if st[i] & mask & (1 << ray):
                zmax = out[i, rc.ZMAX + ray - 2] if ray >= 2 else 0.0
                paths[(i, ray)] = one_host(ray, z0, x1, z1, out[i, rc.LVALUE + ray], zmax)
    return paths


# ---- the reference's running depth chain (IceRayTracing.cc:1288-1350, 1394-1520, 1571-1702) ------
def reference_depths(ray, z0, z1, zmax):
    """The z the reference pushes for ray (0 D, 1 R, 2-3 Ra), its loops restated statement by
    statement (zn = zn - h as a running chain; no sample dropped), flip applied.  Returns
    (z, the number of samples of leg 1)."""
    if z0 > z1:
        z0, z1 = z1, z0
    z = []
    zn = z1
    if ray > 0:
        top = 0.0 if ray == 1 else -zmax
        while True:  # leg 1: a sample is pushed when zn <= 0, the loop ends when zn passes the top
            if zn <= 0:
                z.append(zn)
            zn = zn + H
            if zn > top:
                break
        zn = -1e-7 if ray == 1 else -zmax
    n1 = len(z)
    while True:  # the downward leg
        z.append(zn)
        zn = zn - H
        if zn < z0:
            zn = z0
            break
    z.append(zn)
    return np.array(z), n1


def ulp_distance(a, b):
    """|a - b| in units in the last place of the larger magnitude (0 where equal)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# ---- physics --------------------------------------------------------------------------------------
def reach_to(ray, L, z0, z1, zmax, k, n1, z):
    """The horizontal distance from the Tx (the lower depth, after the flip) along ray to sample k
    at depth z, by quadrature over the leg structure: a sample of the downward leg is reached from
    z0 directly, a sample of leg 1 over the top of the ray."""
    lo = min(z0, z1)
    if ray == 0 or k >= n1:
        legs = [(lo, z)]
    else:
        top = -1e-7 if ray == 1 else -zmax
        legs = [(lo, top), (z, top)]
    return rc.integrate_ray(L, legs)[0]


def physics_samples(q, out, st, paths, rng, max_rays=40, max_samples=200):
    """(row, ray, k, |x - integral|, bound) on first, last, the leg joints and 2 drawn samples per
    ray, at most max_samples in all of at most max_rays accepted rays; the bound is
    1e-9 max(1 m, x1)."""
    keys = sorted(paths)
    if len(keys) > max_rays:
        # every kind of ray among them: round-robin over the kinds
        by = {r: [k for k in keys if k[1] == r] for r in range(KINDS)}
        keys = []
        while len(keys) < max_rays:
            for r in range(KINDS):
                if by[r] and len(keys) < max_rays:
                    keys.append(by[r].pop(0))
    rows = []
    for i, ray in keys:
        z0, x1, z1 = q[i]
        x, z = paths[(i, ray)]
        L = out[i, rc.LVALUE + ray]
        zmax = out[i, rc.ZMAX + ray - 2] if ray >= 2 else 0.0
        n = len(z)
        n1 = reference_depths(ray, z0, z1, zmax)[1]
        ks = {0, n - 1, n - 2, max(n1 - 1, 0), min(n1, n - 1)}
        ks |= set(int(k) for k in rng.integers(0, n, 2))
        for k in sorted(ks):
            if len(rows) >= max_samples:
                return rows
            xk = x[k] if z0 <= z1 else x1 - x[k]  # undo the flip: distance from the lower end
            ref = reach_to(ray, L, z0, z1, zmax, k, n1, z[k])
            rows.append((i, ray, k, abs(xk - ref), 1e-9 * max(1.0, abs(x1))))
    return rows
