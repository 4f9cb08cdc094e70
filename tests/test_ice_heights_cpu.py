"""The minimizers at ice heights other than 3000 m, on the host route (no GPU), and the query
generators tests/test_gpu_ice_heights.py shares.

Every other minimizer test has the ice surface at 3000 m: in the bottom layer of the GDAS
atmosphere, 217 m under its first layer bound.  Here the ice lies at sea level, at the South Pole's
2835 m, on the first layer bound and one ulp above it, in layers 1 and 2, on the second bound and
at 15 km, so bottom_layer() takes every value and the set of middle air segments changes.  The one
query calls (airice_solve_host / airice_trace_ice_to_air_host with n = 1) run the host route, the
same __host__ __device__ source as the kernels, against the oracle under the unchanged parity rule.

The 1e-9 rule on the geometric path in air is pinned for Tx >= ice + 250 m only (DESIGN.md §3,
"Tx within a few metres of the ice"); the generators clamp Tx there, and the near-ice tests at the
end of this module give that one column its measured absolute bound instead.

Not reachable from here: the CoREAS entry (airice_hdtip_launch) and the table lookup's minimizer
fallback have no host entry in the Python layer (their one-query host routes sit behind the C++
drop-ins, which tests/test_gpu_compat.py drives on a GPU machine); the GPU module runs both.
"""
import numpy as np
import pytest

import oracle
from tests import parity


def _medium_heights():
    """The layer bounds (m) and h_top of the loaded medium: atmlay_cm[1 .. max_layers - 1] / 100,
    the quotient both the library and the oracle form."""
    from airiceraytracing_amd import _lib
    m = _lib.load_medium()
    return tuple(m.atmlay_cm[i] / 100 for i in range(1, int(m.max_layers))), float(m.h_top)


BOUNDS, H_TOP = _medium_heights()
B1, B2, B3 = BOUNDS
ICE_HEIGHTS = (0.0, 2835.0, B1, float(np.nextafter(B1, np.inf)), 4000.0, B2, 9000.0, 15000.0)
ICE_IDS = ("0", "2835", "b1", "b1+ulp", "4000", "b2", "9000", "15000")
ICE_PARAMS = [pytest.param(h, id=i) for h, i in zip(ICE_HEIGHTS, ICE_IDS)]
VARIANTS = ("multiray", "pywrapper")

# the slot holding the geometric path in air of each entry point's output: Air2IceRayTracing's
# dummy[14] (MultiRay) / dummy[13] (pythonwrapper), GetHorizontalDistanceToIntersectionPoint's
# geometricalPathLengthInAir (dummy[14] * 100) and Py_TraceIceToAir's a[3]
GEO_AIR_SLOT = {"multiray": 14, "pywrapper": 13, "hdtip": 3, "trace": 3}

# Tx this far above the (effective) ice and further: where the 1e-9 rule on the geometric path in
# air is pinned
TX_CLEARANCE = 250.0


def ice_height_queries(ice: float, n: int, seed: int):
    """(txh, dist, depth), n queries in metres over ice at ``ice``: the fixed rows first (Tx on the
    layer bounds and one ulp under them, at h_top, above the atmosphere, 250 / 300 / 1000 m over
    the ice; D = 0, 1e-3, 10, 49999; the antenna on the surface, and, where the first bound is
    within 240 m over the ice, an antenna in the air exactly on it and 30 m past it: the effective
    ice on and across the bound), then a cfg3-like body with every fifth antenna in the air."""
    rng = np.random.default_rng(seed)
    rows = []

    def some_d():
        return rng.uniform(0.0, 5e4)

    def some_dep():
        return -rng.uniform(0.0, 300.0)

    for b in BOUNDS:
        if b > ice + TX_CLEARANCE:
            rows.append((b, some_d(), some_dep()))
            rows.append((float(np.nextafter(b, 0.0)), some_d(), some_dep()))
    rows.append((H_TOP, some_d(), some_dep()))
    rows.append((1.001e5, some_d(), some_dep()))
    rows.append((5e5, some_d(), some_dep()))
    for dh in (250.0, 300.0, 1000.0):  # low over the ice: distances up to 5x the height
        rows.append((ice + dh, dh * rng.uniform(0.05, 5.0), some_dep()))
    for d in (0.0, 1e-3, 10.0, 49999.0):
        rows.append((rng.uniform(ice + TX_CLEARANCE, 1e5), d, some_dep()))
    rows.append((rng.uniform(ice + TX_CLEARANCE, 1e5), some_d(), 0.0))
    rows.append((rng.uniform(ice + TX_CLEARANCE, 3e4), 10.0, 0.0))
    if 0.0 <= B1 - ice < 240.0:
        for dep in (B1 - ice, B1 - ice + 30.0):
            rows.append((rng.uniform(ice + 600.0, 3e4), rng.uniform(0.0, 2e4), dep))
            rows.append((B2, rng.uniform(0.0, 2e4), dep))
    fx = np.array(rows)
    m = n - fx.shape[0]
    assert m > 0, (n, fx.shape)
    txh = rng.uniform(ice + TX_CLEARANCE, 1e5, m)
    dist = rng.uniform(0.0, 5e4, m)
    depth = -rng.uniform(0.0, 300.0, m)
    up = rng.uniform(0.0, 240.0, m)
    air = np.arange(m) % 5 == 4
    depth[air] = up[air]
    txh = np.concatenate([fx[:, 0], txh])
    dist = np.concatenate([fx[:, 1], dist])
    depth = np.concatenate([fx[:, 2], depth])
    txh = np.maximum(txh, ice + np.maximum(depth, 0.0) + TX_CLEARANCE)
    return txh, dist, depth


MIXED_ICE = ICE_HEIGHTS + (3000.0,)


def mixed_ice_trace_queries(n: int, seed: int):
    """(depth, ice, txh, dist) for trace_ice_to_air_*: the ice drawn per query from ICE_HEIGHTS and
    3000 m, Tx = ice + U(1, 17000), depth -U(1, 300), D ~ U(0, 3e4).  No ice of the list lies in
    the bottom layer with a Tx 17 km over it in the top one, so every 16th query takes
    Tx = ice + U(21000, 40000) instead: with them the batch holds all four layer-span classes of
    query_bucket()."""
    rng = np.random.default_rng(seed)
    ice = rng.choice(np.array(MIXED_ICE), n)
    up = rng.uniform(1.0, 17000.0, n)
    high = rng.uniform(21000.0, 40000.0, n)
    txh = ice + np.where(np.arange(n) % 16 == 15, high, up)
    depth = -rng.uniform(1.0, 300.0, n)
    dist = rng.uniform(0.0, 3e4, n)
    return depth, ice, txh, dist


def layer_of(m, z):
    """The air layer [atmlay[l], atmlay[l + 1]) that holds height z, from the oracle medium's
    bounds; -1 when none does (the scans of .cc:1798-1825)."""
    z = np.asarray(z, dtype=np.float64)
    lay = np.full(z.shape, -1)
    for l in range(int(m.max_layers)):
        lay[(z >= m.atmlay[l] / 100) & (z < m.atmlay[l + 1] / 100)] = l
    return lay


def span_classes(m, txh, ice_eff):
    """query_bucket()'s layer-span class: top_layer(Tx) - bottom_layer(ice), clamped to 0..3."""
    return np.clip(layer_of(m, txh) - layer_of(m, ice_eff), 0, 3)


def oracle_solve(variant, om, om_py, txh, dist, depth, ice, nthreads=0):
    """Air2IceRayTracing of the variant on the oracle: (out (fields, n), status, floors)."""
    if variant == "pywrapper":
        rows = [oracle.py_air2ice(om_py, a, b, ice, c, oracle.straight_angle_of(om_py, a, b, ice, c))
                for a, b, c in zip(txh, dist, depth)]
        return (np.stack([r[0] for r in rows], 1), np.array([r[1] for r in rows]),
                parity.PYSOLVE_FLOORS)
    ref, rst = oracle.solve_batch(om, txh, dist, depth, ice, nthreads=nthreads)
    return ref, rst.astype(np.int64), parity.SOLVE_FLOORS


def make_solver(variant):
    from airiceraytracing_amd import AirIceSolver, VARIANT_MULTIRAY, VARIANT_PYWRAPPER
    return AirIceSolver(variant=VARIANT_PYWRAPPER if variant == "pywrapper" else VARIANT_MULTIRAY)


def host_solve_one_by_one(s, txh, dist, depth, ice):
    """airice_solve_host with n = 1 per query: the host route."""
    outs, sts = [], []
    for i in range(txh.size):
        o, st = s.solve_host(txh[i:i + 1], dist[i:i + 1], depth[i:i + 1], ice)
        outs.append(o[:, 0])
        sts.append(int(st[0]))
    return np.stack(outs, 1), np.array(sts)


def host_trace_one_by_one(s, depth, ice, txh, dist):
    return np.stack([s.trace_ice_to_air_host(depth[i:i + 1], ice[i:i + 1], txh[i:i + 1],
                                             dist[i:i + 1])[0] for i in range(depth.size)])


@pytest.fixture(scope="module")
def host_mode():
    from airiceraytracing_amd import _lib
    assert _lib.lib().airice_scalar_mode(-1) == _lib.SCALAR_HOST  # the default


def test_ice_heights_come_from_the_medium(oracle_medium):
    """The list holds what the issue names, and both libraries form the same bounds."""
    assert [round(h, 5) for h in ICE_HEIGHTS] == [0.0, 2835.0, 3217.48275, 3217.48275, 4000.0,
                                                  8363.53902, 9000.0, 15000.0]
    assert ICE_HEIGHTS[3] > ICE_HEIGHTS[2] and H_TOP == 23141.0295
    assert tuple(oracle_medium.atmlay[i] / 100 for i in range(1, 4)) == BOUNDS
    assert [int(layer_of(oracle_medium, h)) for h in ICE_HEIGHTS] == [0, 0, 1, 1, 1, 2, 2, 2]


@pytest.mark.parametrize("ice", ICE_PARAMS)
def test_generator_rows(oracle_medium, ice):
    """ice_height_queries holds its fixed rows and keeps the Tx clearance."""
    txh, dist, depth = ice_height_queries(ice, 400, seed=1)
    assert txh.size == dist.size == depth.size == 400
    eff = ice + np.maximum(depth, 0.0)
    assert (txh >= eff + TX_CLEARANCE).all()
    for b in BOUNDS:
        assert ((txh == b).any() and (txh == np.nextafter(b, 0.0)).any()) == (b > ice + 250.0)
    for t in (H_TOP, 1.001e5, 5e5) if ice + 250.0 < H_TOP else (1.001e5, 5e5):
        assert (txh == t).any()
    for d in (0.0, 1e-3, 10.0, 49999.0):
        assert (dist == d).any()
    assert (depth == 0.0).any() and 0.15 < (depth > 0).mean() < 0.25
    if 0.0 <= B1 - ice < 240.0:
        assert (eff == B1).any() and (eff == ice + (B1 - ice + 30.0)).any()
    # the effective ice of the antennas in the air reaches the next layer where a bound is close
    assert set(np.unique(layer_of(oracle_medium, eff))) >= {int(layer_of(oracle_medium, ice))}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ice", ICE_PARAMS)
def test_host_solves_vs_oracle(host_mode, oracle_medium, oracle_medium_py, ice, variant):
    """400 one-query host solves per ice height against the oracle: status equal on the pinned
    rows, every column within 1e-9 (SOLVE_FLOORS / PYSOLVE_FLOORS), pinned share over 0.95."""
    s = make_solver(variant)
    txh, dist, depth = ice_height_queries(ice, 400, seed=100 + ICE_HEIGHTS.index(ice))
    got, gst = host_solve_one_by_one(s, txh, dist, depth, ice)
    ref, rst, floors = oracle_solve(variant, oracle_medium, oracle_medium_py, txh, dist, depth, ice)
    mask = (rst & oracle.SOLVE_UNPINNED) == 0
    rep = parity.compare_columns(got, ref, floors, mask=mask)
    print(f"[host {variant} ice={ice!r}] n={txh.size} pinned={mask.mean():.4f} "
          f"max_rel={rep['max_rel']:.3e}")
    assert mask.mean() > 0.95
    assert np.array_equal(gst[mask], rst[mask])
    assert rep["ok"], rep


def test_host_trace_mixed_ice_vs_oracle(host_mode, oracle_medium_py):
    """Py_TraceIceToAir one query at a time on the host, the ice height drawn per query: solved
    masks equal, TRACE_FLOORS at 1e-9."""
    s = make_solver("pywrapper")
    depth, ice, txh, dist = mixed_ice_trace_queries(600, seed=41)
    got = host_trace_one_by_one(s, depth, ice, txh, dist)
    ref = oracle.py_trace_batch(oracle_medium_py, depth, ice, txh, dist)
    assert set(span_classes(oracle_medium_py, txh, ice).tolist()) == {0, 1, 2, 3}
    assert np.array_equal(got[:, 0] != -1000, ref[:, 0] != -1000)
    rep = parity.compare_columns(got.T, ref.T, parity.TRACE_FLOORS)
    print(f"[host trace mixed ice] n={depth.size} solved={(ref[:, 0] != -1000).mean():.4f} "
          f"max_rel={rep['max_rel']:.3e}")
    assert rep["ok"], rep


# ---------------------------------------------------------------------------------------------
# Tx within a few metres of the ice
# ---------------------------------------------------------------------------------------------
NEAR_ICE_HEIGHTS = (0.0, 3000.0, 9000.0)
NEAR_OFFSETS = (0.5, 1.0, 10.0, 50.0)
NEAR_N = 256

# max |oracle - exact| (m) of the geometric path in air over near_ice_queries() at NEAR_ICE_HEIGHTS
# (3 x 256 queries, the pinned rows), per variant, the exact value being the 50-digit evaluation of
# the reference's formula at the oracle's own launch angle (geo_air_exact below).  Measured on the
# CPU with mpmath 1.3.0: 6.6305e-7 m (MultiRay) and 1.7735e-6 m (pythonwrapper), both at ice
# 9000 m, written here rounded up to two digits; test_oracle_geo_air_error_is_the_recorded_one
# measures it again.  The bound on |product - oracle| is 4 x that: one for each side's rounding,
# doubled for the multi-layer sums ("Tx within a few metres of the ice").
GEO_AIR_ORACLE_ERR_M = {"multiray": 6.7e-7, "pywrapper": 1.8e-6}
GEO_AIR_NEAR_ICE_ATOL_M = {v: 4 * e for v, e in GEO_AIR_ORACLE_ERR_M.items()}
# the entry points that report the same number: the CoREAS entry is MultiRay's solve in cm, the
# trace the pythonwrapper's
GEO_AIR_NEAR_ICE_ATOL_M["hdtip_cm"] = 100 * GEO_AIR_NEAR_ICE_ATOL_M["multiray"]
GEO_AIR_NEAR_ICE_ATOL_M["trace"] = GEO_AIR_NEAR_ICE_ATOL_M["pywrapper"]


def near_ice_queries(ice: float, n: int, seed: int):
    """(txh, dist, depth): Tx 0.5, 1, 10 and 50 m over the effective ice in turn, D ~ U(0, 5000),
    depth -U(0, 300) with every fifth antenna +U(0, 240) in the air."""
    rng = np.random.default_rng(seed)
    dist = rng.uniform(0.0, 5000.0, n)
    depth = -rng.uniform(0.0, 300.0, n)
    up = rng.uniform(0.0, 240.0, n)
    air = np.arange(n) % 5 == 4
    depth[air] = up[air]
    txh = ice + np.maximum(depth, 0.0) + np.array(NEAR_OFFSETS)[np.arange(n) % len(NEAR_OFFSETS)]
    return txh, dist, depth


def assert_every_offset_pinned(mask):
    """Near-horizontal rays (D up to 5 km from 0.5 m up) often end on the reference's undefined
    bracket set-up, which the oracle flags; the comparison must still hold rows of every Tx
    offset: at least a quarter of each (a condition on the oracle's own mask, 0.58 and more of
    each offset here)."""
    k = np.arange(mask.size) % len(NEAR_OFFSETS)
    for j in range(len(NEAR_OFFSETS)):
        assert mask[k == j].mean() >= 0.25, (NEAR_OFFSETS[j], mask[k == j].mean())


def geo_air_exact(m, txh: float, ice_eff: float, launch_deg: float) -> float:
    """The geometric path in air of GetAirPropagationPar at one launch angle, in 50-digit
    arithmetic on the medium's double constants: L = n(Tx) sin(180 - launch), then per layer
    fpathD(start) - fpathD(stop) with each end's own layer constants, the layer starts 1e-5 m under
    the bounds as the reference has them.  Rounded to double at the end."""
    import mpmath as mp
    with mp.workdps(50):
        A = mp.mpf(m.A_air)
        bounds = [m.atmlay[i] / 100 for i in range(1, int(m.max_layers))]

        def consts(z):  # GetB_air / GetC_air: the last layer's constants from its lower bound up
            l = min(int(np.searchsorted(bounds, z, side="right")), int(m.max_layers) - 1)
            return mp.mpf(m.B_air[l]), -mp.mpf(m.C_air[l])

        def n_at(z):
            B, C = consts(z)
            return A + B * mp.exp(C * mp.mpf(z))

        def fpath(z, L):
            B, C = consts(z)
            x = mp.mpf(z)
            e = mp.exp(C * x)
            y = A + B * e
            sA = mp.sqrt(A * A - L * L)
            sy = mp.sqrt(y * y - L * L)  # y sqrt(Q) of the reference's form
            return (mp.log(sy + y) - A * mp.log(sA * sy + A * y - L * L) / sA + A * C * x / sA) / C

        top, bot = int(layer_of(m, txh)), int(layer_of(m, ice_eff))
        L = n_at(txh) * mp.sin((180 - mp.mpf(launch_deg)) * (mp.mpf(m.pi) / 180))
        total = mp.mpf(0)
        for il in range(top, bot - 1, -1):
            start = txh if il == top else m.atmlay[il + 1] / 100 - 0.00001
            stop = ice_eff if il == bot else m.atmlay[il] / 100
            total += fpath(start, L) - fpath(stop, L)
        return float(total)


def geo_air_errors(m, txh, ice_eff, launch_deg, geo, rows):
    """|geo - exact| on ``rows`` (indices), each against the exact path at its own launch angle."""
    return np.array([abs(geo[i] - geo_air_exact(m, txh[i], ice_eff[i], launch_deg[i]))
                     for i in rows])


def compare_except_geo_air(got, ref, floors, slot, mask, atol):
    """The unchanged rule on every column but ``slot``; that one within ``atol`` absolutely."""
    keep = np.arange(got.shape[0]) != slot
    rep = parity.compare_columns(got[keep], ref[keep], floors[keep], mask=mask)
    d = np.abs(got[slot][mask] - ref[slot][mask])
    both_nan = np.isnan(got[slot][mask]) & np.isnan(ref[slot][mask])
    rep["geo_air_max_abs"] = float(np.nanmax(np.where(both_nan, 0.0, d))) if d.size else 0.0
    rep["geo_air_ok"] = bool(np.all(both_nan | (d <= atol)))
    return rep


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ice", NEAR_ICE_HEIGHTS)
def test_host_near_ice_vs_oracle(host_mode, oracle_medium, oracle_medium_py, ice, variant):
    """Tx 0.5 .. 50 m over the ice on the host route: every column but the geometric path in air
    under the unchanged rule, that column within its measured absolute bound."""
    s = make_solver(variant)
    txh, dist, depth = near_ice_queries(ice, NEAR_N, seed=300 + int(ice))
    got, gst = host_solve_one_by_one(s, txh, dist, depth, ice)
    ref, rst, floors = oracle_solve(variant, oracle_medium, oracle_medium_py, txh, dist, depth, ice)
    mask = (rst & oracle.SOLVE_UNPINNED) == 0
    rep = compare_except_geo_air(got, ref, floors, GEO_AIR_SLOT[variant], mask,
                                 GEO_AIR_NEAR_ICE_ATOL_M[variant])
    print(f"[host near ice {variant} ice={ice}] pinned={mask.mean():.4f} "
          f"max_rel={rep['max_rel']:.3e} geo_air_max_abs={rep['geo_air_max_abs']:.3e}")
    assert_every_offset_pinned(mask)
    assert np.array_equal(gst[mask], rst[mask])
    assert rep["ok"], rep
    assert rep["geo_air_ok"], rep


def test_host_near_ice_trace_vs_oracle(host_mode, oracle_medium_py):
    s = make_solver("pywrapper")
    parts = [near_ice_queries(ice, NEAR_N, seed=300 + int(ice)) + (np.full(NEAR_N, ice),)
             for ice in NEAR_ICE_HEIGHTS]
    txh, dist, depth, ice = (np.concatenate([p[k] for p in parts]) for k in range(4))
    got = host_trace_one_by_one(s, depth, ice, txh, dist)
    ref = oracle.py_trace_batch(oracle_medium_py, depth, ice, txh, dist)
    solved = ref[:, 0] != -1000
    assert np.array_equal(got[:, 0] != -1000, solved)
    rep = compare_except_geo_air(got.T, ref.T, parity.TRACE_FLOORS, GEO_AIR_SLOT["trace"], solved,
                                 GEO_AIR_NEAR_ICE_ATOL_M["trace"])
    print(f"[host near ice trace] solved={solved.mean():.4f} max_rel={rep['max_rel']:.3e} "
          f"geo_air_max_abs={rep['geo_air_max_abs']:.3e}")
    assert np.array_equal(got[~solved], ref[~solved])
    assert rep["ok"], rep
    assert rep["geo_air_ok"], rep


def near_ice_oracle_errors(variant, om, om_py):
    """(max |oracle - exact|, the per-height (txh, dist, depth, ice, pinned rows) sets)."""
    m = om_py if variant == "pywrapper" else om
    worst, sets = 0.0, []
    for ice in NEAR_ICE_HEIGHTS:
        txh, dist, depth = near_ice_queries(ice, NEAR_N, seed=300 + int(ice))
        ref, rst, _ = oracle_solve(variant, om, om_py, txh, dist, depth, ice)
        slot = GEO_AIR_SLOT[variant]
        rows = np.flatnonzero(((rst & oracle.SOLVE_UNPINNED) == 0) & np.isfinite(ref[slot]))
        eff = ice + np.maximum(depth, 0.0)
        err = geo_air_errors(m, txh, eff, ref[10], ref[slot], rows)
        worst = max(worst, float(err.max()))
        sets.append((txh, dist, depth, ice, rows))
    return worst, sets


@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_geo_air_error_is_the_recorded_one(oracle_medium, oracle_medium_py, variant):
    """GEO_AIR_ORACLE_ERR_M is what the oracle's geometric path in air is off by near the ice, and
    the host route is off by no more than twice that."""
    pytest.importorskip("mpmath")
    worst, sets = near_ice_oracle_errors(variant, oracle_medium, oracle_medium_py)
    m = oracle_medium_py if variant == "pywrapper" else oracle_medium
    s = make_solver(variant)
    slot = GEO_AIR_SLOT[variant]
    host_worst = 0.0
    for txh, dist, depth, ice, rows in sets:
        got, _ = host_solve_one_by_one(s, txh[rows], dist[rows], depth[rows], ice)
        eff = ice + np.maximum(depth[rows], 0.0)
        err = geo_air_errors(m, txh[rows], eff, got[10], got[slot], np.arange(rows.size))
        host_worst = max(host_worst, float(err.max()))
    print(f"[near ice {variant}] oracle max |geo_air - exact| = {worst:.4e} m, host route "
          f"{host_worst:.4e} m")
    assert worst <= GEO_AIR_ORACLE_ERR_M[variant]
    assert host_worst <= 2 * GEO_AIR_ORACLE_ERR_M[variant]
