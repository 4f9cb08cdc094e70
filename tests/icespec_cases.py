"""Pairs, frequency lists and the comparison rule for the attenuation spectrum
(airice_icesol_spectrum_launch / _host, the drop-in's GetAttenuationSpectrum): shared by
tests/test_gpu_icespec.py and tests/test_icespec_cpu.py."""
import ctypes
import functools

import numpy as np

from tests import iceray_cases as rays
from tests import icesol_cases as sol

F8 = (0.05, 0.1, 0.5, 0.999999, 1.0, 2.0, 3.16, 5.0)  # straddles the 1 GHz branch, holds 1.0
BAD4 = (np.nan, 0.0, -0.3, 0.3)                       # a NaN, a 0, a negative and one good value
N_PAIRS = 64


def pairs():
    """The 23 head rows (every ray class, the edge rows, 9 non-finite rows) and 41 drawn rows."""
    head = rays.head_rows()
    return np.concatenate([head, rays.drawn(N_PAIRS - len(head), np.random.default_rng(12))])


def log_spaced(n, lo=0.05, hi=5.0):
    return np.exp(np.linspace(np.log(lo), np.log(hi), n))


def frequency_lists():
    """Every list of the checks, by name: F = 1 (each of the eight in turn), 3, 8, 65 (one past a
    wave), 257 (one past a block's lanes) and the four with three bad bins."""
    lists = {f"F1[{f!r}]": (f,) for f in F8}
    lists["F3"] = sol.FREQUENCIES
    lists["F8"] = F8
    lists["F65"] = tuple(log_spaced(65))
    lists["F257"] = tuple(log_spaced(257))
    lists["bad4"] = BAD4
    return lists


def good(frequency):
    return bool(np.isfinite(frequency) and frequency > 0)


def mismatches(att, single, tol=1e-12):
    """Entries where a spectrum column and the single-frequency route disagree: where one is
    exactly 0.0 or NaN the other must be too, otherwise |d| <= tol max(1, |1 - Att_single|)."""
    att, single = np.asarray(att), np.asarray(single)
    special = (single == 0.0) | np.isnan(single) | (att == 0.0) | np.isnan(att)
    same_special = ((single == 0.0) == (att == 0.0)) & (np.isnan(single) == np.isnan(att))
    with np.errstate(invalid="ignore"):
        close = np.abs(att - single) <= tol * np.maximum(1.0, np.abs(1.0 - single))
    return np.argwhere(~np.where(special, same_special, close))


@functools.lru_cache(maxsize=None)
def attenuation_mp(ray_type, frequency, L, z0, z1):
    """icesol_cases.attenuation_mp, computed once per ray and frequency for all the tests."""
    return sol.attenuation_mp(ray_type, frequency, L, z0, z1)


def mp_failures(q, ray_rows, types, att, frequencies):
    """The class rows against mpmath: for each slot that holds a ray (types (n, 2): the icesol
    type columns; att (n, 2, F)) and each frequency, |Att - (1 - I_mp)| against
    icesol_cases.attenuation_bound(I_mp).  Returns (failures, rays checked, worst ratio)."""
    bad, n, worst = [], 0, 0.0
    for i, (z0, x1, z1) in enumerate(q):
        for s in range(2):
            ray = int(types[i, s]) - 1
            if ray_rows[i, rays.RANG + ray] == sol.NO_RAY:
                if not (att[i, s] == 0.0).all():
                    bad.append((i, s, "no ray", att[i, s].tolist()))
                continue
            for k, f in enumerate(frequencies):
                I, err = attenuation_mp(ray + 1, float(f), float(ray_rows[i, rays.LVALUE + ray]),
                                        float(z0), float(z1))
                bound = sol.attenuation_bound(I)
                assert err <= 0.01 * bound, (i, s, f, I, err)
                ratio = abs(att[i, s, k] - (1 - I)) / bound
                ratio = np.inf if np.isnan(ratio) else ratio
                worst, n = max(worst, ratio), n + 1
                if ratio > 1.0:
                    bad.append((i, s, f, att[i, s, k], 1 - I, bound))
    return bad, n, worst


def dropin_spectrum(z0, x1, z1, frequencies, a0=1.0):
    """IceRayTracing::GetAttenuationSpectrum through its C++ name: (rc, AttRay0, AttRay1)."""
    from airiceraytracing_amd import _lib
    f = getattr(_lib.lib(), "_ZN13IceRayTracing22GetAttenuationSpectrumEddddPKdmPdS2_")
    D, P = ctypes.c_double, ctypes.c_void_p
    f.argtypes, f.restype = [D, D, D, D, P, ctypes.c_size_t, P, P], ctypes.c_int
    fr = np.ascontiguousarray(frequencies, dtype=np.float64)
    a = np.full((2, max(fr.size, 1)), -777.25)
    rc = f(z1, x1, z0, a0, _lib.ptr(fr), fr.size, _lib.ptr(a[0]), _lib.ptr(a[1]))
    return rc, a[0, :fr.size], a[1, :fr.size]


def set_model(model):
    """IceRayTracing::SetA / SetB / SetC (they take references)."""
    from airiceraytracing_amd import _lib
    for name, v in zip("ABC", model):
        f = getattr(_lib.lib(), f"_ZN13IceRayTracing4Set{name}ERd")
        f.argtypes, f.restype = [ctypes.POINTER(ctypes.c_double)], None
        f(ctypes.byref(ctypes.c_double(v)))
