"""Independent checks for the two-ray solutions (airice_icesol_launch / _host, the drop-in's
GetRayTracingSolutions / GetFocusingFactor): a plain-Python restatement of the reference's choice
and ordering (IceRayTracing.cc:2943-3200) that only copies values of a 29-value solver row, the
attenuation of a ray's legs by mpmath.quad in z with the reference's own integrand form, and the
focusing formula (.cc:3239-3291) applied to two solutions."""
import ctypes
import math

import numpy as np

from tests import iceray_cases as rays

FIELDS = 18
TIME, PATH, LANG, RANG, IGNORE, INCIDENCE, ATT, TYPE, FOCUS = 0, 2, 4, 6, 8, 10, 12, 14, 16
SLOT0, SLOT1, STRAIGHT, FOCUS0, FOCUS1, NONFINITE = 1, 2, 4, 8, 16, 128
CHOICE_COLUMNS = [c for c in range(FIELDS) if c not in (ATT, ATT + 1, FOCUS, FOCUS + 1)]
FREQUENCIES = (0.1, 0.5, 2.0)
NO_RAY = -1000.0


def choose(row, z0, x1, z1):
    """GetRayTracingSolutions on RTresults = row[0..28] for TxDepth z0, Distance x1, RxDepth z1,
    statement by statement; the attenuations are carried as the ray each came from.  Returns
    (the 18 columns with NaN in 12-13 and 16-17, status bits 0-2, the ray (0 D, 1 R, 2 Ra0, 3 Ra1)
    whose attenuation each slot holds, or None where AttRay is the initial 0)."""
    time4, path4 = row[4:8], row[25:29]
    rang4, lang4 = row[8:12], row[0:4]
    att4 = [k if rang4[k] != NO_RAY else None for k in range(4)]  # .cc:2976-2987

    T, P, R, La, At, Ty = [0, 0], [0, 0], [0, 0], [0, 0], [None, None], [0, 0]

    def put(slot, ray):
        T[slot], P[slot], R[slot], La[slot] = time4[ray], path4[ray], rang4[ray], lang4[ray]
        Ty[slot], At[slot] = ray + 1, att4[ray]

    put(0, 0)  # .cc:2989-3005
    put(1, 1)
    inc = [100.0, row[18]]
    if rang4[1] == NO_RAY:
        inc = [100.0, 100.0]
    if rang4[0] != NO_RAY:
        put(0, 0)
    if rang4[1] != NO_RAY:
        put(1, 1)
    if rang4[2] != NO_RAY and rang4[0] != NO_RAY:
        put(0, 0)
        put(1, 2)
    if rang4[2] != NO_RAY and rang4[1] != NO_RAY:
        put(1, 1)
        put(0, 2)
    if rang4[3] != NO_RAY and rang4[0] != NO_RAY:
        put(0, 0)
        put(1, 3)
    if rang4[3] != NO_RAY and rang4[1] != NO_RAY:
        put(1, 1)
        put(0, 3)
    if rang4[3] != NO_RAY and rang4[2] != NO_RAY:
        put(1, 3)
        put(0, 2)
    if R[1] == NO_RAY and R[0] == NO_RAY and rang4[2] != NO_RAY:
        put(0, 2)
    if R[1] == NO_RAY and R[0] == NO_RAY and rang4[3] != NO_RAY:
        put(1, 3)
    ignore = [1, 1]
    if R[0] == NO_RAY:
        ignore[0] = 0
    if R[1] == NO_RAY:
        ignore[1] = 0
    if T[0] > T[1] and R[0] != NO_RAY and R[1] != NO_RAY:
        for v in (La, R, T, Ty, P, At):
            v[0], v[1] = v[1], v[0]
    straight = bool(z1 == z0 and T[0] == 0 and P[0] == 0)
    if straight:
        if x1 == 0:
            ignore = [0, 0]
        P[0] = x1
        T[0] = x1 / (rays.C_LIGHT / (rays.A + rays.B * math.exp(-rays.C * abs(z0))))
        La[0] = R[0] = 90.0
        ignore[0] = 1
    out = np.full(FIELDS, np.nan)
    for k in range(2):
        out[TIME + k], out[PATH + k], out[LANG + k], out[RANG + k] = T[k], P[k], La[k], R[k]
        out[IGNORE + k], out[INCIDENCE + k], out[TYPE + k] = ignore[k], inc[k], Ty[k]
    status = (SLOT0 if ignore[0] else 0) | (SLOT1 if ignore[1] else 0) | (STRAIGHT if straight else 0)
    return out, status, At


def choose_rows(q, ray_rows):
    """choose() over rows: (values (n, 18), status (n), attenuation sources (n x 2)); a row the
    solver flagged non-finite is NaN with IgnoreCh and types 0 and status 128."""
    out = np.full((len(q), FIELDS), np.nan)
    st = np.zeros(len(q), dtype=np.int64)
    src = []
    for i, (z0, x1, z1) in enumerate(q):
        if not ray_rows[i, rays.STATUS] < 128:
            out[i, [IGNORE, IGNORE + 1, TYPE, TYPE + 1]] = 0.0
            st[i] = NONFINITE
            src.append([None, None])
            continue
        out[i], st[i], s = choose([float(v) for v in ray_rows[i, :29]], z0, x1, z1)
        src.append(s)
    return out, st, src


def same_choice(got, want):
    """The choice columns of (n, 18) arrays, bit for bit."""
    return rays.same_bits(np.asarray(got)[:, CHOICE_COLUMNS], np.asarray(want)[:, CHOICE_COLUMNS])


# ---- attenuation, independent of the solver -----------------------------------------------------
def leg_mp(frequency, L, za, zb, turning=False):
    """|integral over [za, zb] (depths, positive) of sqrt(1 + tan(asin(L/n))^2) / L_att(z, f) dz|
    by mpmath.quad at 30 digits, in z, no substitution: the reference's integrand form
    (.cc:174) over its attenuation model (.cc:137-163).  turning: zb is ln(B/(L-A))/C evaluated in
    mpmath from L.  Returns (value, mpmath's own error estimate)."""
    import mpmath as mp
    with mp.workdps(30):
        Lm, Am, Bm, Cm = mp.mpf(float(L)), mp.mpf(rays.A), mp.mpf(rays.B), mp.mpf(rays.C)
        za = mp.mpf(float(za))
        zb = mp.log(Bm / (Lm - Am)) / Cm if turning else mp.mpf(float(zb))
        w = mp.log(mp.mpf(float(frequency)))
        w0, w1, w2 = mp.log(mp.mpf("0.0001")), mp.mpf(0), mp.log(mp.mpf("3.16"))
        low = frequency < 1.0

        t3, t2, t1, t0 = (mp.mpf(v) for v in ("1.83415e-09", "-1.59061e-08", "0.00267687", "-51.0696"))
        b00, b01, b02 = mp.mpf("-6.74890"), mp.mpf("0.026709"), mp.mpf("0.000884")
        b10, b11, b12 = mp.mpf("-6.22121"), mp.mpf("0.070927"), mp.mpf("0.001773")
        b20, b21, b22 = mp.mpf("-4.09468"), mp.mpf("0.002213"), mp.mpf("0.000332")

        def integrand(z):
            d = abs(z)
            t = t3 * d ** 3 + (t2 * d ** 2) + t1 * d + t0
            b0 = b00 + t * (b01 - t * b02)
            b1 = b10 - t * (b11 + t * b12)
            b2 = b20 - t * (b21 + t * b22)
            if low:
                a, bb = (b1 * w0 - b0 * w1) / (w0 - w1), (b1 - b0) / (w1 - w0)
            else:
                a, bb = (b2 * w1 - b1 * w2) / (w1 - w2), (b2 - b1) / (w2 - w1)
            n = Am + Bm * mp.exp(-Cm * d)
            return mp.exp(a + bb * w) * mp.sqrt(1 + mp.tan(mp.asin(Lm / n)) ** 2)

        lo, hi = min(za, zb), max(za, zb)
        if lo == hi:
            return 0.0, 0.0
        # the shallow end is where n - L is smallest (zero for a turning leg): tanh-sinh takes the
        # end itself, the break points keep the levels of the near-singular stretch apart
        pts = [lo, lo + (hi - lo) * mp.mpf("1e-4"), lo + (hi - lo) / 10, hi]
        v, err = mp.quad(integrand, pts, error=True)
        return float(abs(v)), float(err)


def ray_legs(ray_type, z0, z1):
    """(za, zb, turning) of the legs of a ray of type 1 D, 2 R, 3 / 4 refracted."""
    z0, z1 = abs(z0), abs(z1)
    if ray_type == 1:
        return [(z0, z1, False)]
    if ray_type == 2:
        return [(z0, 1e-6, False), (z1, 1e-6, False)]
    return [(z0, None, True), (z1, None, True)]


def attenuation_mp(ray_type, frequency, L, z0, z1):
    """I of a ray (A0 = 1) over its legs, and the summed error estimate of the quadratures."""
    total = err = 0.0
    for za, zb, turning in ray_legs(ray_type, z0, z1):
        v, e = leg_mp(frequency, L, za, zb, turning)
        total += v
        err += e
    return total, err


def attenuation_bound(I):
    """The issue's bound on |Att - (1 - I)|."""
    return 1e-9 * I + 1e-15


# ---- the drop-in's scalar functions through their C++ names --------------------------------------
def _dropin(symbol, n_args, restype=ctypes.c_double):
    from airiceraytracing_amd import _lib
    f = getattr(_lib.lib(), symbol)
    f.argtypes, f.restype = [ctypes.c_double] * n_args, restype
    return f


def total_attenuation(ray_type, a0, frequency, z0, z1, L):
    """IceRayTracing::GetTotalAttenuationDirect / Reflected / Refracted (zmax unused: passed 0)."""
    if ray_type == 1:
        return _dropin("_ZN13IceRayTracing25GetTotalAttenuationDirectEddddd", 5)(a0, frequency, z0, z1, L)
    if ray_type == 2:
        return _dropin("_ZN13IceRayTracing28GetTotalAttenuationReflectedEddddd", 5)(
            a0, frequency, z0, z1, L)
    return _dropin("_ZN13IceRayTracing28GetTotalAttenuationRefractedEdddddd", 6)(
        a0, frequency, z0, z1, 0.0, L)


def integrate_over_lattn(a0, frequency, z0, z1, L):
    return _dropin("_ZN13IceRayTracing18IntegrateOverLAttnEddddd", 5)(a0, frequency, z0, z1, L)


# ---- focusing -----------------------------------------------------------------------------------
def focusing(z0, z1, at, lower):
    """GetFocusingFactor's closing arithmetic (.cc:3239-3291) on the (18) solutions of the
    receiver at z1 and of the one at z1 - 0.01, with a factor whose condition is not met 0.0:
    ((f0, f1), the status bits 3-4)."""
    pi = rays.PI_REF
    n_tx = rays.A + rays.B * math.exp(-rays.C * abs(z0))
    n_rx = rays.A + rays.B * math.exp(-rays.C * abs(z1))
    f, bits = [0.0, 0.0], 0
    for k in range(2):
        if at[RANG + k] != NO_RAY and lower[RANG + k] != NO_RAY:
            rec, lau = at[RANG + k] * (pi / 180), at[LANG + k] * (pi / 180)
            lau_b = lower[LANG + k] * (pi / 180)
            with np.errstate(all="ignore"):
                step = np.float64((z1 - 0.01) - z1) / np.float64(lau_b - lau)
                f[k] = float(np.sqrt((np.float64(at[PATH + k]) / (np.sin(rec) * np.abs(step)))
                                     * (n_tx / n_rx)))
            bits |= FOCUS0 << k
    if z1 == z0 and f[0] == 0:
        f[0] = 1.0
    return f, bits


def ulps(a, b):
    """Distance of two doubles in units in the last place of b (inf when only one is NaN)."""
    if math.isnan(a) or math.isnan(b):
        return 0.0 if math.isnan(a) and math.isnan(b) else math.inf
    if a == b:
        return 0.0
    return abs(a - b) / float(np.spacing(abs(b)))


def host_solutions(solver, q, frequency=0.1, a0=1.0, focusing=False, model=None):
    """The host route (airice_icesol_host, n = 1, on the calling thread) row by row:
    (values (n, 18), status (n)); it launches nothing."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    out = np.empty((len(q), FIELDS))
    st = np.empty(len(q), dtype=np.int64)
    with scalar_mode(_lib.SCALAR_HOST), _lib.launched("icesol_kernel") as k, \
            _lib.launched("iceray_kernel") as r:
        for i, (z0, x1, z1) in enumerate(q):
            o, s = solver.ice_solutions_host(z0, x1, z1, a0=a0, frequency=frequency,
                                             focusing=focusing, model=model)
            out[i], st[i] = o[:, 0], s[0]
    assert k.count == 0 and r.count == 0
    return out, st
