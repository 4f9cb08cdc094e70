"""Shared by tests/test_firn_cpu.py and tests/test_gpu_firn.py: the Summit two-layer firn, the ray
draw, and the reference of a layered ray composed from three one-layer oracle rays.

The ray parameter L = n sin(theta) is fixed by the air part and conserved in the ice, so with
up = (A, B[0], C[0]), low = (A, B[1], C[1]) and the boundary at depth b the ice leg of a ray to an
antenna at depth < -b is

    up(depth = -b) + [low(depth) - low(depth = -b)]        columns 4, 7, 10, 17
    low(depth)[13]                                         the receive angle

every air column and the surface Fresnel coefficients being those of up.  Columns 2, 5, 8 are the
sums of their air and ice parts.
"""
from __future__ import annotations

import copy

import numpy as np

import oracle

SUMMIT_A = 1.775
SUMMIT_BOUNDARY = 14.9
SUMMIT_B = (-0.5019, -0.448023)
SUMMIT_C = (0.03247, 0.02469)
ICE_M = 3216.0
DEPTHS = (-14.9000001, -15.0, -20.0, -100.0, -200.0)
# composed from the oracle / bit-identical to the one-layer call with (A, B[0], C[0])
COMPOSED_COLUMNS = (2, 4, 5, 7, 8, 10, 13, 17)
UPPER_COLUMNS = (1, 3, 6, 9, 11, 12, 14, 15, 16)
# table column -> dummy[] slot (MultiRayAirIceRefraction.cc:2101-2111)
TABLE_SLOTS = (1, 2, 7, 6, 11, 3, 14, 15, 16, 17, 13)


def oracle_layer(om, layer: int, A=SUMMIT_A, B=SUMMIT_B, C=SUMMIT_C):
    """A copy of the oracle medium with the ice model of one firn layer."""
    m = copy.copy(om)
    m.A_ice, m.B_ice, m.C_ice = A, B[layer], C[layer]
    return m


def lib_medium(solver_medium, A=SUMMIT_A, B=None, C=None):
    """A copy of the library medium with A_ice (and, for the one-layer calls, B_ice / C_ice) set."""
    from airiceraytracing_amd import _lib
    m = _lib.Medium.from_buffer_copy(bytes(solver_medium))
    m.A_ice = A
    if B is not None:
        m.B_ice, m.C_ice = B, C
    return m


def draw(n: int, seed: int = 20240611):
    """n rays: launch angle U(90.1, 180) deg, Tx 1 m to 90 km above the ice (log-uniform, so the
    lowest air layer and Tx heights near the surface are drawn as often as the top), the five
    depths in turn."""
    rng = np.random.default_rng(seed)
    launch = rng.uniform(90.1, 180.0, n)
    txh = ICE_M + 10.0 ** rng.uniform(0.0, np.log10(9.0e4), n)
    depth = np.array(DEPTHS)[np.arange(n) % len(DEPTHS)]
    return launch, txh, depth


def compose(up, low, low_b):
    """(18, n) layered reference from the three one-layer results (each (18, n))."""
    out = np.array(up, dtype=np.float64, copy=True)
    for c in (4, 7, 10, 17):
        out[c] = up[c] + (low[c] - low_b[c])
    out[2] = up[3] + out[4]
    out[5] = up[6] + out[7]
    out[8] = up[9] + out[10]
    out[13] = low[13]
    return out


def compose_rays(om, launch, txh, depth, ice_m=ICE_M, b=SUMMIT_BOUNDARY):
    """The layered reference of single rays (per-ray depth, all below the boundary)."""
    m_up, m_low = oracle_layer(om, 0), oracle_layer(om, 1)
    n = len(launch)
    up, low, low_b = (np.empty((18, n)) for _ in range(3))
    for k in range(n):
        up[:, k] = oracle.ray_solution(m_up, launch[k], txh[k], ice_m, -b)
        low[:, k] = oracle.ray_solution(m_low, launch[k], txh[k], ice_m, depth[k])
        low_b[:, k] = oracle.ray_solution(m_low, launch[k], txh[k], ice_m, -b)
    return compose(up, low, low_b)


def compose_table(om, depth_cm, ice_cm, height_step, start_angle, stop_angle, angle_step,
                  b=SUMMIT_BOUNDARY):
    """(11 x n float32 table, 18 x n doubles) of a whole grid for an antenna below the boundary."""
    m_up, m_low = oracle_layer(om, 0), oracle_layer(om, 1)
    grid = lambda d: oracle.grid_init(d, ice_cm, height_step, start_angle, stop_angle, angle_step)
    g_b, g_d = grid(-b * 100.0), grid(depth_cm)
    rows = int(g_d.table_rows)
    assert int(g_b.table_rows) == rows and g_b.angle_steps == g_d.angle_steps
    _, up = oracle.table_rows(m_up, g_b, 0, rows, full=True)
    _, low = oracle.table_rows(m_low, g_d, 0, rows, full=True)
    _, low_b = oracle.table_rows(m_low, g_b, 0, rows, full=True)
    full = compose(up, low, low_b)
    table = np.stack([full[s] for s in TABLE_SLOTS]).astype(np.float32)
    return table, full
