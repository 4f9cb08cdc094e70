"""Batched ray-path sampling (airice_ray_paths_launch) against the loop of airice_single_ray_launch
calls it replaces, on one GPU.

Workload A: 10,000 rays at ice 3000 m, antenna depth 200 m, Tx heights uniform in 3010-20000 m.
Workload B: the shower of DrawShowerRays.C:440-519 (ice 2800 m, antenna 180 m deep, a 30 degree
            shower axis sampled every 10 m from 500 m above the ice, points kept while they are
            >= 10 m above the ice), launch angles from the minimizer (paths_between's route).

Per workload: the two batch kernels timed with the library's hipEvent kernel timing over --reps
launches after --warmup, the wall time of the whole batch call (host plan, upload, two launches,
synchronise) and the wall time of the per-ray loop on one stream (2 launches per ray, synchronised
once at the end).  Prints one JSON document.

    python tools/ray_paths_bench.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shower_geometry(ice=2800.0, top=500.0, angle_deg=30.0, step=10.0, points=100):
    """(Tx height, horizontal distance to the antenna) of the shower points: the vertical line
    of points rotated by the shower angle about its middle, the antenna 100 m past the impact
    point of the axis."""
    th = np.radians(angle_deg)
    mid = top / 2 + ice
    y = ice + top - step * np.arange(points)
    rx = -(y - mid) * np.sin(th)
    ry = (y - mid) * np.cos(th) + mid
    rx = rx - rx[0]
    hdist = (ry[0] - ice) * np.tan(th) + 100.0
    keep = ry >= ice + 10.0
    return ry[keep], (hdist - rx)[keep]


def bench(solver, name, launch, txh, ice, depth, reps, warmup):
    import torch
    from airiceraytracing_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n = txh.size
    offsets = solver.ray_paths_plan(txh, ice, depth)
    total = int(offsets[-1])
    t_launch = torch.from_numpy(launch).to(dev)
    summary = torch.empty((6, n), dtype=torch.float64, device=dev)
    x = torch.empty(total, dtype=torch.float64, device=dev)
    z = torch.empty(total, dtype=torch.float64, device=dev)
    work = torch.empty(solver.ray_paths_work_bytes(txh, ice, depth), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()

    def batch():
        solver.ray_paths_device(t_launch, txh, ice, depth, offsets, summary, x, z, work=work,
                                stream=st)
        torch.cuda.synchronize()

    for _ in range(warmup):
        batch()
    _lib.kernel_timing(True)
    _lib.kernel_time("ray_consts_kernel")
    _lib.kernel_time("ray_paths_kernel")
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        batch()
        wall.append(time.perf_counter() - t0)
    consts_ms, nc = _lib.kernel_time("ray_consts_kernel")
    paths_ms, npk = _lib.kernel_time("ray_paths_kernel")
    _lib.kernel_timing(False)
    assert nc == npk == reps, (nc, npk)
    bx, bz, bs = x.clone(), z.clone(), summary.clone()

    # the loop: one airice_single_ray_launch per ray into the same arrays
    single = torch.empty((n, _lib.SINGLE_RAY_WORK), dtype=torch.float64, device=dev)
    x.zero_()
    z.zero_()
    m = ctypes.byref(solver.medium)
    sh = ctypes.c_void_p(st.cuda_stream)
    xp, zp, sp = x.data_ptr(), z.data_ptr(), single.data_ptr()

    def loop():
        for i in range(n):
            o = int(offsets[i])
            rc = L.airice_single_ray_launch(m, depth, launch[i], txh[i], ice,
                                            ctypes.c_void_p(sp + 8 * _lib.SINGLE_RAY_WORK * i),
                                            ctypes.c_void_p(xp + 8 * o),
                                            ctypes.c_void_p(zp + 8 * o),
                                            int(offsets[i + 1]) - o, sh)
            assert rc == 0, L.airice_last_error()
        torch.cuda.synchronize()

    for _ in range(min(warmup, 1)):
        loop()
    lwall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        loop()
        lwall.append(time.perf_counter() - t0)
    same = bool(torch.equal(bx.view(torch.int64), x.view(torch.int64)) and
                torch.equal(bz.view(torch.int64), z.view(torch.int64)) and
                torch.equal(bs.t().contiguous().view(torch.int64),
                            single[:, :6].contiguous().view(torch.int64)))
    kern_s = (consts_ms + paths_ms) / reps * 1e-3
    bw, lw = float(np.median(wall)), float(np.median(lwall))
    return {
        "workload": name, "rays": int(n), "samples": total, "reps": reps,
        "ray_consts_kernel_us": consts_ms / reps * 1e3,
        "ray_paths_kernel_us": paths_ms / reps * 1e3,
        "samples_per_s_paths_kernel": total / (paths_ms / reps * 1e-3),
        "samples_per_s_both_kernels": total / kern_s,
        "batch_call_wall_ms_median": bw * 1e3, "batch_call_wall_ms_min": min(wall) * 1e3,
        "samples_per_s_batch_call": total / bw,
        "loop_wall_ms_median": lw * 1e3, "loop_wall_ms_min": min(lwall) * 1e3,
        "samples_per_s_loop": total / lw,
        "loop_launches": 2 * int(n), "batch_launches": 2,
        "ratio_loop_over_batch_call": lw / bw,
        "ratio_loop_over_batch_kernels": lw / kern_s,
        "loop_bits_equal_batch": same,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    from airiceraytracing_amd import AirIceSolver
    s = AirIceSolver()
    rng = np.random.default_rng(8)
    res = []
    txh = rng.uniform(3010.0, 20000.0, 10000)
    launch = rng.uniform(95.0, 179.0, txh.size)
    res.append(bench(s, "A: 10000 rays, Tx 3010-20000 m, ice 3000 m, depth 200 m", launch, txh,
                     3000.0, 200.0, a.reps, a.warmup))
    txh, dist = shower_geometry()
    sol, status = s.solve_host(txh, dist, np.full(txh.shape, -180.0), 2800.0, variant=0)
    res.append(bench(s, "B: DrawShowerRays geometry (%d of 100 points >= 10 m above the ice)"
                     % txh.size, np.ascontiguousarray(sol[10]), np.ascontiguousarray(txh), 2800.0,
                     180.0, a.reps, a.warmup))
    doc = json.dumps({"ray_paths_bench": res}, indent=1)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
