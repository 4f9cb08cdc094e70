#!/usr/bin/env python3
"""The in-ice interpolation tables, measured: build time by kernel, lookups per second against
the direct solve they replace, and the interpolation error of the reference's method.  Writes
profiles/icetab_bench.json and prints it as one JSON line.

    python tools/icetab_bench.py [--warmup 2] [--steps 7] [--out profiles/icetab_bench.json]

Build: MakeTable's own 401 x 201 grid around (150 m, -100 m) for 1, 4 and 16 antennas between 100
and 115 m deep, the four kernels timed by the library's event pairs (airice_kernel_timing).
Lookup: 1e6 and 1e7 queries against 1 and 16 antennas, uniform over the grid and Gaussian
(sigma = 1 m) around the shower point, each launch bracketed by a device event pair on the launch
stream, every shape warmed up first, median and spread reported.  Bytes per query are the nominal
ones: 20 B of inputs (x, z, antenna), 105 B of outputs (13 values, status) and four 128-byte
records; `tb_per_s` prices the rate at them, `of_air_lookup` is that against the 3.25 TB/s the
air-side lookup reaches.
Direct: iceray_kernel twice and icesol_kernel once at the same points (the thing the table
replaces).  Error: interpolated value against direct solution at 1e5 uniform off-node points, per
parameter, over the points where both hold a value -- the reference method's own property,
reported and never asserted."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIT, DEPTH = 150.0, -100.0
AIR_LOOKUP_TB_S = 3.25
IO_BYTES, TABLE_BYTES = 20 + 105, 4 * 128
BUILD_KERNELS = ("icetab_points_kernel", "iceray_kernel", "icesol_kernel", "icetab_pack_kernel")
PARAMS = ("time0", "path0", "launch0", "receive0", "attenuation0", "focusing0", "time1", "path1",
          "launch1", "receive1", "attenuation1", "focusing1", "incidence")


def timed(step, stream, warmup, steps):
    import torch
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        step()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def rx_depths(n_ant):
    return [-100.0 - a for a in range(n_ant)]


def bench_build(solver, n_ant, warmup, steps):
    import torch
    from airiceraytracing_amd import _lib
    stream = torch.cuda.current_stream()
    for _ in range(warmup):
        solver.ice_tables(HIT, DEPTH, rx_depths(n_ant), stream=stream)
    torch.cuda.synchronize()
    _lib.kernel_timing(True)
    for k in BUILD_KERNELS:
        _lib.kernel_time(k, reset=True)
    for _ in range(steps):
        tables = solver.ice_tables(HIT, DEPTH, rx_depths(n_ant), stream=stream)
    torch.cuda.synchronize()
    res = {"antennas": n_ant, "positions": n_ant * 401 * 201, "kernels_ms": {}}
    for k in BUILD_KERNELS:
        ms, launches = _lib.kernel_time(k, reset=True)
        assert launches == steps, (k, launches)
        res["kernels_ms"][k] = ms / steps
    _lib.kernel_timing(False)
    res["ms"] = sum(res["kernels_ms"].values())
    res["positions_per_s"] = res["positions"] / (res["ms"] * 1e-3)
    return res, tables


def draw(rng, n, n_ant, shape):
    if shape == "uniform":
        x = rng.uniform(HIT - 20.0, HIT + 20.0, n)
        z = rng.uniform(DEPTH - 10.0, DEPTH + 10.0, n)
    else:
        x = rng.normal(HIT, 1.0, n)
        z = rng.normal(DEPTH, 1.0, n)
    return rng.integers(0, n_ant, n).astype(np.int32), x, z


def bench_lookup(solver, tables, n_ant, n, shape, rng, warmup, steps):
    import torch
    from airiceraytracing_amd import _lib
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    ant, x, z = draw(rng, n, n_ant, shape)
    d_ant, d_x, d_z = [torch.from_numpy(a).to(dev) for a in (ant, x, z)]
    out = torch.empty((13, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    res = {"antennas": n_ant, "queries": n, "distribution": shape}
    look = timed(lambda: tables.lookup(d_x, d_z, ant=d_ant, out=out, status=st, stream=stream),
                 stream, warmup, steps)
    look["lookups_per_s"] = n / (look["ms_median"] * 1e-3)
    look["io_bytes_per_query"], look["table_bytes_per_query"] = IO_BYTES, TABLE_BYTES
    look["tb_per_s"] = look["lookups_per_s"] * (IO_BYTES + TABLE_BYTES) / 1e12
    look["io_tb_per_s"] = look["lookups_per_s"] * IO_BYTES / 1e12
    look["of_air_lookup"] = look["tb_per_s"] / AIR_LOOKUP_TB_S
    status = st.cpu().numpy()
    look["in_cell"] = float((status & _lib.ICETAB_CELL != 0).mean())
    look["idw"] = float((status & _lib.ICETAB_IDW != 0).mean())
    res["lookup"] = look
    # the direct solve at the same points: (zT, xT, zR), the receiver 1 cm lower, the solutions
    zr = torch.from_numpy(np.asarray(rx_depths(n_ant))[ant]).to(dev)
    zr_low = zr - 0.01
    rays = torch.empty((_lib.ICERAY_FIELDS, n), dtype=torch.float64, device=dev)
    lower = torch.empty((_lib.ICERAY_FIELDS, n), dtype=torch.float64, device=dev)
    sol = torch.empty((_lib.ICESOL_FIELDS, n), dtype=torch.float64, device=dev)

    def direct():
        solver.ice_rays_device(d_z, d_x, zr, rays, stream=stream)
        solver.ice_rays_device(d_z, d_x, zr_low, lower, stream=stream)
        solver.ice_solutions_device(d_z, d_x, zr, rays, sol, st, rays_lower=lower, stream=stream)

    res["direct"] = timed(direct, stream, 1, min(steps, 3))
    res["direct"]["solves_per_s"] = n / (res["direct"]["ms_median"] * 1e-3)
    res["table_gain"] = res["direct"]["ms_median"] / look["ms_median"]
    return res


def interpolation_error(solver, tables, rng, n):
    import torch
    from airiceraytracing_amd import _lib
    from airiceraytracing_amd import solver as sv
    dev = torch.device("cuda:0")
    # off the nodes: a cell drawn uniformly, the point 10 % to 90 % of the way across it
    x = HIT - 20.0 + 0.1 * (rng.integers(0, 400, n) + rng.uniform(0.1, 0.9, n))
    z = DEPTH - 10.0 + 0.1 * (rng.integers(0, 200, n) + rng.uniform(0.1, 0.9, n))
    d_x, d_z = torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev)
    got = tables.lookup(d_x, d_z).cpu().numpy()
    zr = torch.full((n,), rx_depths(1)[0], dtype=torch.float64, device=dev)
    rays = torch.empty((_lib.ICERAY_FIELDS, n), dtype=torch.float64, device=dev)
    lower = torch.empty((_lib.ICERAY_FIELDS, n), dtype=torch.float64, device=dev)
    sol = torch.empty((_lib.ICESOL_FIELDS, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    solver.ice_rays_device(d_z, d_x, zr, rays)
    solver.ice_rays_device(d_z, d_x, zr - 0.01, lower)
    solver.ice_solutions_device(d_z, d_x, zr, rays, sol, st, rays_lower=lower)
    torch.cuda.synchronize()
    want = sv.icetab_pack_host(sol.cpu().numpy(), st.cpu().numpy())[:, :13].T
    res = {"points": n, "parameters": {}}
    for c, name in enumerate(PARAMS):
        both = (got[c] != -1000) & (want[c] != -1000) & np.isfinite(got[c]) & np.isfinite(want[c])
        err = np.abs(got[c][both] - want[c][both])
        rel = err / np.maximum(np.abs(want[c][both]), 1e-300)
        res["parameters"][name] = {
            "points": int(both.sum()),
            "abs_median": float(np.median(err)) if both.any() else None,
            "abs_max": float(err.max()) if both.any() else None,
            "rel_median": float(np.median(rel)) if both.any() else None,
            "rel_max": float(rel.max()) if both.any() else None}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=2727)
    ap.add_argument("--queries", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icetab_bench.json"))
    args = ap.parse_args()

    from airiceraytracing_amd import AirIceSolver
    solver = AirIceSolver()
    rng = np.random.default_rng(args.seed)
    res = {"bench": "icetab", "grid": "401 x 201, 0.1 m", "shower": [HIT, DEPTH],
           "steps": args.steps, "warmup": args.warmup, "air_lookup_tb_per_s": AIR_LOOKUP_TB_S,
           "build": [], "lookup": []}
    tables = {}
    for n_ant in (1, 4, 16):
        b, tables[n_ant] = bench_build(solver, n_ant, args.warmup, args.steps)
        res["build"].append(b)
    for n_ant in (1, 16):
        for n in args.queries:
            for shape in ("uniform", "gaussian"):
                res["lookup"].append(bench_lookup(solver, tables[n_ant], n_ant, n, shape, rng,
                                                  args.warmup, args.steps))
    res["interpolation_error"] = interpolation_error(solver, tables[1], rng, 100_000)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
