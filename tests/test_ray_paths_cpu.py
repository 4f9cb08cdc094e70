"""Batched ray paths on the CPU: the host plan of airice_ray_paths_plan (CSR sample offsets of a
batch of rays) against the oracle's per-ray SingleRayAirIceRefraction loops, and the argument
checks airice_ray_paths_launch makes before any device call."""
import copy
import ctypes
import re

import numpy as np
import pytest

import oracle
from tests.test_single_ray_cpu import CASES

# Tx heights above ice 3000 m around one 256-sample tile of ray_paths_kernel, and the two shortest
# paths: txh - ice in {0.5, 1, 254, 255, 256, 257}.  A path of integer txh - ice = d has d + 1 air
# samples, one more where it crosses the layer boundary at 3217.48 m (the upper layer's last
# sample is clamped to the boundary and the lower layer starts 1e-5 m below it), and one ice
# sample at depth 0: d + 3 here, so 254..257 give 258..261.  d = 251, 252, 253 are added so that
# the counts 255, 256 and 257 themselves occur.
TILE_EDGE_TX = [3000.5, 3001.0, 3254.0, 3255.0, 3256.0, 3257.0, 3251.0, 3252.0, 3253.0]


def _batches():
    """The eight CASES grouped by their (depth, ice), then the tile-boundary batch."""
    groups = {}
    for depth, launch, txh, ice in CASES:
        groups.setdefault((float(depth), float(ice)), []).append((float(launch), float(txh)))
    out = [(d, i, [t for _, t in rays]) for (d, i), rays in groups.items()]
    out.append((0.0, 3000.0, TILE_EDGE_TX))
    return out


def _plan(m, depth, ice, txh):
    from airiceraytracing_amd import _lib
    h = np.ascontiguousarray(txh, dtype=np.float64)
    offsets = np.full(h.size + 1, -7, dtype=np.int64)
    work = ctypes.c_size_t(0)
    rc = _lib.lib().airice_ray_paths_plan(ctypes.byref(m), depth, ice, _lib.ptr(h), h.size,
                                          _lib.ptr(offsets), ctypes.byref(work))
    return rc, offsets, work.value


@pytest.mark.parametrize("depth,ice,txh", _batches())
def test_plan_offsets_are_running_oracle_counts(oracle_medium, depth, ice, txh):
    from airiceraytracing_amd import _lib
    rc, offsets, work = _plan(_lib.load_medium(), depth, ice, txh)
    assert rc == 0, _lib.lib().airice_last_error()
    counts = []
    for t in txh:
        # the count does not depend on the launch angle
        r, _, _ = oracle.single_ray(oracle_medium, depth, 135.0, t, ice)
        counts.append(r.n_air + r.n_ice)
    assert offsets[0] == 0
    assert offsets.tolist() == [0] + np.cumsum(counts).tolist()
    assert work > 0


def test_tile_edge_counts_straddle_a_tile(oracle_medium):
    """The batch above really has rays one short of a tile, of exactly one tile and one past it."""
    from airiceraytracing_amd import _lib
    rc, offsets, _ = _plan(_lib.load_medium(), 0.0, 3000.0, TILE_EDGE_TX)
    assert rc == 0
    assert np.diff(offsets).tolist() == [3, 3, 258, 259, 260, 261, 255, 256, 257]


def test_solver_plan_matches_capi():
    from airiceraytracing_amd import AirIceSolver, _lib
    s = AirIceSolver()
    rc, offsets, work = _plan(s.medium, 0.0, 3000.0, TILE_EDGE_TX)
    assert rc == 0
    assert np.array_equal(s.ray_paths_plan(TILE_EDGE_TX, 3000.0, 0.0), offsets)
    assert s.ray_paths_work_bytes(TILE_EDGE_TX, 3000.0, 0.0) == work


def test_empty_batch():
    from airiceraytracing_amd import _lib
    m = _lib.load_medium()
    rc, offsets, work = _plan(m, 200.0, 3000.0, np.empty(0))
    assert rc == 0 and offsets.tolist() == [0] and work == 0
    # the launch and the host entry of an empty batch are AIRICE_OK and touch nothing
    L = _lib.lib()
    assert L.airice_ray_paths_launch(ctypes.byref(m), 200.0, 3000.0, None, None, 0,
                                     _lib.ptr(offsets), None, 0, None, 0, None, None, 0,
                                     None) == 0
    assert L.airice_ray_paths_host(ctypes.byref(m), 200.0, 3000.0, None, None, 0,
                                   _lib.ptr(offsets), None, 0, None, None, 0) == 0


def test_rejected_ray_is_named():
    """A Tx height the single-ray plan rejects fails the batch and the message names the ray.
    Every layer of the GDAS medium is shorter than the 2^31-sample limit, so the medium's last
    layer bound is raised (an atmosphere tabulated to 1e12 m) and a Tx at 3e9 m then makes its
    layer 3e9 samples long."""
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    m = copy.copy(_lib.load_medium())
    m.atmlay_cm[4] = 1e14
    info = _lib.SingleRayInfo()
    bad = 3e9
    assert L.airice_single_ray_plan(ctypes.byref(m), 200.0, 135.0, 5000.0, 3000.0,
                                    ctypes.byref(info)) == 0
    assert L.airice_single_ray_plan(ctypes.byref(m), 200.0, 135.0, bad, 3000.0,
                                    ctypes.byref(info)) == -1
    single_msg = L.airice_last_error().decode()
    rc, _, _ = _plan(m, 200.0, 3000.0, [5000.0, 8000.0, bad, 9000.0])
    assert rc == -1
    msg = L.airice_last_error().decode()
    assert re.search(r"\bray 2\b", msg), msg
    assert single_msg in msg
    # the same batch without that ray plans
    rc, offsets, _ = _plan(m, 200.0, 3000.0, [5000.0, 8000.0, 9000.0])
    assert rc == 0 and offsets[0] == 0 and np.all(np.diff(offsets) > 0)


def test_launch_checks_capacity_and_workspace_before_any_device_call():
    """cap one short of offsets[n], or a workspace one byte short, is AIRICE_EINVAL; nothing is
    dereferenced or launched (the device pointers here are not real), so this runs without a GPU."""
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    m = _lib.load_medium()
    txh = np.array(TILE_EDGE_TX)
    rc, offsets, work = _plan(m, 0.0, 3000.0, txh)
    assert rc == 0
    total = int(offsets[-1])
    fake = [ctypes.c_void_p(0x10000 * (k + 1)) for k in range(5)]
    d_launch, d_work, d_sum, d_x, d_z = fake
    before = {k: _lib.launch_count(k) for k in ("ray_consts_kernel", "ray_paths_kernel")}

    def launch(offs, work_bytes, cap, x=d_x, z=d_z):
        return L.airice_ray_paths_launch(ctypes.byref(m), 0.0, 3000.0, d_launch, _lib.ptr(txh),
                                         txh.size, _lib.ptr(offs), d_work, work_bytes, d_sum,
                                         txh.size, x, z, cap, None)

    assert launch(offsets, work, total - 1) == -1
    assert b"capacity" in L.airice_last_error()
    assert launch(offsets, work - 1, total) == -1
    assert b"workspace" in L.airice_last_error()
    # x without z, and offsets that are not this batch's plan
    assert launch(offsets, work, total, z=None) == -1
    wrong = offsets.copy()
    wrong[3] += 1
    assert launch(wrong, work, total) == -1
    assert b"offsets[3]" in L.airice_last_error()
    for k, v in before.items():
        assert _lib.launch_count(k) == v
