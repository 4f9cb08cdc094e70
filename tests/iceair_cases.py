"""Shared cases and independent checks for the ice-to-air direct ray (airice_iceair_launch / _host,
the drop-in's GetDirectRayPar_Air and fDa_Air) and for the first-arrival tracer
(airice_icefirst_launch / _host, DirectRayTracer): the head rows, the draw, the host routes row by
row, the physics check -- the ice leg integrated numerically with mpmath, the air leg in closed
form, sharing nothing with the solver beyond n(z) and Snell's invariant L -- and the reference's
first-arrival rule restated in numpy over the in-ice solver's rows."""
import os
import subprocess
import tempfile

import numpy as np

from tests import iceray_cases as rays
from tests.conftest import ROOT

FIELDS = 10
RANG, LANG, TIME, LVALUE, CHECKZERO, STATUS, EVALS, ITERS, PHYS_TIME, PATH = range(10)
ACCEPTED, NONFINITE = 1, 128
C_LIGHT = rays.C_LIGHT
OTHER_MODEL = (1.775, -0.5, 0.02)

FIRST_FIELDS = 8
F_LANG, F_RANG, F_PATH, F_TIMEC, F_TIME, F_TYPE, F_X1, F_STATUS = range(8)

DRIVER = os.path.join(ROOT, "tests", "cpp", "iceair_driver")
DRIVER_ASAN = os.path.join(ROOT, "tests", "cpp", "iceair_driver_asan")

# (z0, x1, h): a steep exit, a grazing exit, a deep Tx, then h and x1 at the ends of the draw
FINITE_HEAD = ((-100.0, 10.0, 500.0), (-10.0, 2500.0, 5.0), (-1000.0, 300.0, 1.0),
               (-200.0, 100.0, 0.1), (-200.0, 100.0, 3000.0), (-200.0, 1.0, 50.0),
               (-200.0, 3000.0, 50.0))


def nonfinite_rows():
    rows = []
    for k in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            q = list(FINITE_HEAD[0])
            q[k] = bad
            rows.append(q)
    return np.array(rows, dtype=np.float64)


def head_rows():
    return np.concatenate([np.array(FINITE_HEAD), nonfinite_rows()])


def drawn(n, rng):
    """n rows of the issue's draw: z0 uniform in [-1000, -1], h log-uniform in [0.1, 3000], x1
    log-uniform in [1, 3000]."""
    z0 = -1000.0 + 999.0 * rng.random(n)
    h = 0.1 * np.exp(np.log(3000.0 / 0.1) * rng.random(n))
    x1 = np.exp(np.log(3000.0) * rng.random(n))
    return np.stack([z0, x1, h], axis=1)


def batch(n, rng):
    head = head_rows()
    if n <= len(head):
        return head[:n].copy()
    return np.concatenate([head, drawn(n - len(head), rng)])


def host_rows(solver, q, model=None):
    """The host route (airice_iceair_host, n = 1, on the calling thread) row by row:
    (values (n, 10), status (n)); nothing may launch."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    out = np.empty((len(q), FIELDS))
    st = np.empty(len(q), dtype=np.int64)
    with scalar_mode(_lib.SCALAR_HOST), _lib.launched("iceair_kernel") as k:
        for i, (z0, x1, h) in enumerate(q):
            o, s = solver.ice_to_air_host(z0, x1, h, model=model)
            out[i], st[i] = o[:, 0], s[0]
    assert k.count == 0
    return out, st


# ---- physics, independent of the solver ---------------------------------------------------------
def physics_errors(q, out, st):
    """For every accepted row (default model): (row, reach error, its bound |checkzero| + 1e-9 x1,
    error of column 8, its bound 1.78e-6/c + 1e-12 t, error of column 9, its bound
    1e-6 + 1e-12 s, |sin(column 0) - L|, error of column 2 - column 8 against
    h (L - 1) / (c sqrt(1 - L^2)) over |column 8|): the bounds as the issue states them, the last
    two to be held to 1e-12.  The air leg is closed form at 30 digits: at a grazing exit
    1 - L^2 cancels in doubles."""
    import mpmath as mp
    rows = []
    for i, (z0, x1, h) in enumerate(q):
        if not st[i] & ACCEPTED:
            continue
        L = out[i, LVALUE]
        reach, time, path = rays.integrate_ray(L, [(z0, -1e-7)])
        with mp.workdps(30):
            Lm, hm = mp.mpf(float(L)), mp.mpf(float(h))
            root = mp.sqrt(1 - Lm * Lm)
            reach_air = float(hm * Lm / root)
            path_air = float(hm / root)
            time_air = float(hm / (mp.mpf(C_LIGHT) * root))
            gap = float(hm * (Lm - 1) / (mp.mpf(C_LIGHT) * root))
        t, s = out[i, PHYS_TIME], out[i, PATH]
        rows.append((i, abs(reach + reach_air - x1), abs(out[i, CHECKZERO]) + 1e-9 * abs(x1),
                     abs(time + time_air - t), 1.78e-6 / C_LIGHT + 1e-12 * abs(t),
                     abs(path + path_air - s), 1e-6 + 1e-12 * abs(s),
                     abs(np.sin(out[i, RANG] * rays.PI_REF / 180.0) - L),
                     abs((out[i, TIME] - t) - gap) / abs(t)))
    return rows


def physics_failures(rows):
    """The rows of physics_errors outside a bound, each with the check's name."""
    bad = []
    for r in rows:
        i, reach, reach_b, t, t_b, s, s_b, snell, gap = r
        for name, err, bound in (("reach", reach, reach_b), ("time", t, t_b), ("path", s, s_b),
                                 ("snell", snell, 1e-12), ("col2-col8", gap, 1e-12)):
            if not err <= bound:
                bad.append((i, name, err, bound))
    return bad


# ---- the drop-in through the caller program -----------------------------------------------------
def run_driver(mode, rows, program=DRIVER):
    """tests/cpp/iceair_driver <mode> on rows (n, 3 or 6): {tag: (n, words) uint64}."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(rows.tobytes())
        f.flush()
        run = subprocess.run([program, mode, f.name], capture_output=True, text=True, check=True)
    assert run.stderr == "", run.stderr
    got = {}
    for ln in run.stdout.splitlines():
        w = ln.split()
        got.setdefault(w[0], {})[int(w[1])] = [int(x, 16) for x in w[2:]]
    return {tag: bits(np.array([v[i] for i in range(len(rows))], dtype=np.uint64).view(np.float64))
            for tag, v in got.items()}


def bits(a):
    """The values' bit patterns, every NaN as numpy's."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.nan, a).view(np.uint64)


# ---- first arrivals -----------------------------------------------------------------------------
def first_rule(ray_rows, x1):
    """IceRayTracing.cc:2537-2598 as written, over rows (n, 32) of the in-ice solver: candidates
    D, Ra0, Ra1 whose receive angle is not -1000, the first with the strictly smallest time*c
    starting from min = 1e9 (MinValueBin starts at 0); no candidate: -1000; a row flagged
    non-finite: NaN, type 0.  Returns (n, 8)."""
    n = len(ray_rows)
    out = np.empty((n, FIRST_FIELDS))
    for i in range(n):
        g = ray_rows[i]
        status = int(g[rays.STATUS])
        out[i, F_X1], out[i, F_STATUS] = x1[i], status
        if status & rays.NONFINITE:
            out[i, :5], out[i, F_TYPE] = np.nan, 0.0
            continue
        values = []
        for ray in (0, 2, 3):
            if g[rays.RANG + ray] != -1000:
                values.append((g[rays.LANG + ray], g[rays.RANG + ray], g[rays.PATH + ray],
                               g[rays.TIME + ray] * C_LIGHT, g[rays.TIME + ray], ray + 1.0))
        if not values:
            out[i, :5], out[i, F_TYPE] = -1000.0, 0.0
            continue
        min_bin, least = 0, 1e9
        for k, v in enumerate(values):
            if v[3] < least:
                least, min_bin = v[3], k
        out[i, :6] = values[min_bin]
    return out


# deep pairs whose only accepted ray is the reflected one (the draw of iceray_cases has none)
R_ONLY_ROWS = ((-2904.4587553112347, 25.36752433711197, -2806.4070665101),
               (-2879.356449156405, 499.44426652552784, -2921.630601862438))


def first_head_points():
    """iceray_cases.head_rows() and the reflected-only rows as points along the x axis (dy = 0:
    x1 = |x1| exactly), then a non-finite coordinate in each of the six slots: (tx, rx), (3, n)."""
    q = np.concatenate([rays.head_rows(), np.array(R_ONLY_ROWS)])
    tx = np.stack([np.zeros(len(q)), np.zeros(len(q)), q[:, 0]])
    rx = np.stack([q[:, 1], np.zeros(len(q)), q[:, 2]])
    extra_tx, extra_rx = [], []
    for k in range(6):
        for bad in (np.nan, np.inf):
            p = [3.0, 4.0, -180.0, 63.0, 84.0, -100.0]
            p[k] = bad
            extra_tx.append(p[:3])
            extra_rx.append(p[3:])
    tx = np.concatenate([tx, np.array(extra_tx).T], axis=1)
    rx = np.concatenate([rx, np.array(extra_rx).T], axis=1)
    return np.ascontiguousarray(tx), np.ascontiguousarray(rx)


def first_points(q, rng):
    """Emitters and antennas (3, n) each whose (zT, horizontal distance, zR) are q's
    (z0, x1, z1) up to the rounding of the distance: a random origin and azimuth per pair."""
    n = len(q)
    phi = 2 * np.pi * rng.random(n)
    tx = np.stack([200.0 * rng.random(n) - 100.0, 200.0 * rng.random(n) - 100.0, q[:, 0]])
    rx = np.stack([tx[0] + q[:, 1] * np.cos(phi), tx[1] + q[:, 1] * np.sin(phi), q[:, 2]])
    return np.ascontiguousarray(tx), np.ascontiguousarray(rx)


def first_triples(tx, rx):
    """(z0, x1, z1) as DirectRayTracer forms them, x1 = np.sqrt(dx*dx + dy*dy)."""
    dx, dy = tx[0] - rx[0], tx[1] - rx[1]
    with np.errstate(invalid="ignore", over="ignore"):
        x1 = np.sqrt(dx * dx + dy * dy)
    return np.stack([tx[2], x1, rx[2]], axis=1)


def first_host_rows(solver, tx, rx, model=None):
    """The host route (airice_icefirst_host, one pair, on the calling thread) pair by pair:
    (values (n, 8), status (n)); nothing may launch."""
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd.solver import scalar_mode
    n = tx.shape[1]
    out = np.empty((n, FIRST_FIELDS))
    st = np.empty(n, dtype=np.int64)
    kernels = ("icefirst_geom_kernel", "iceray_kernel", "icefirst_select_kernel")
    before = [_lib.launch_count(k) for k in kernels]
    with scalar_mode(_lib.SCALAR_HOST):
        for i in range(n):
            o, s = solver.ice_first_arrivals_host(tx[:, i:i + 1], rx[:, i:i + 1], model=model)
            out[i], st[i] = o[:, 0], s[0]
    assert [_lib.launch_count(k) for k in kernels] == before
    return out, st
