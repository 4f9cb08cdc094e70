#!/usr/bin/env python3
"""Throughput of the in-ice ray solver (iceray_kernel): pairs per second and residual
evaluations per second over the draw of tests/iceray_cases.py, one JSON line.

    python tools/iceray_bench.py [--pairs 1000000] [--warmup 3] [--steps 10] [--host-threads 16]

Timing: inputs and outputs resident on the device, the launches of one step bracketed by a device
event pair on the launch stream (the kernel time, not the enqueue), every shape warmed up before
the timed window, the median step and the spread of the steps reported.  --host-threads N also
runs tests/cpp/iceray_driver --bench on N CPU threads over the first --host-pairs rows: the same
solver source compiled for the host, so the ratio is the speed-up of the device route."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# FP64 vector rate of one MI355X used for the fraction below: 256 CUs x 4 SIMDs x 16 lanes x
# 2.4 GHz FMA issue = 39.3e12 lane-operations per second (78.6 TFLOP/s counting an FMA as two).
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9
# FP64 VALU instructions of the residual function compiled alone for gfx950 (501 in its assembly,
# all three residuals' paths together: four logs, an exp, four square roots, the quotients).  One
# evaluation runs fewer, so the fraction below is an upper bound.
OPS_PER_EVAL = 500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2028)
    ap.add_argument("--host-threads", type=int, default=0)
    ap.add_argument("--host-pairs", type=int, default=200_000)
    args = ap.parse_args()

    import torch
    from airiceraytracing_amd import AirIceSolver, _lib
    from tests import iceray_cases as cases

    q = cases.drawn(args.pairs, np.random.default_rng(args.seed))
    dev = torch.device("cuda:0")
    solver = AirIceSolver()
    cols = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(3)]
    out = torch.empty((_lib.ICERAY_FIELDS, args.pairs), dtype=torch.float64, device=dev)
    st = torch.empty(args.pairs, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream()

    def step():
        solver.ice_rays_device(*cols, out, st, stream=stream)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        step()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    evals = float(out[_lib.ICERAY_EVALS].sum().item())
    status = st.cpu().numpy()
    med = statistics.median(ms)
    res = {
        "bench": "iceray", "pairs": args.pairs, "steps": args.steps, "warmup": args.warmup,
        "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
        "pairs_per_s": args.pairs / (med * 1e-3),
        "evals_per_pair": evals / args.pairs,
        "evals_per_s": evals / (med * 1e-3),
        "fp64_valu_fraction": evals * OPS_PER_EVAL / (med * 1e-3) / PEAK_LANE_OPS,
        "status_counts": {str(k): int(v) for k, v in
                          zip(*np.unique(status, return_counts=True))},
    }
    if args.host_threads > 0:
        n = min(args.host_pairs, args.pairs)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "rows.bin")
            np.ascontiguousarray(q[:n]).tofile(path)
            run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "iceray_driver"), "--bench",
                                  path, str(args.host_threads)], capture_output=True, text=True,
                                 check=True)
        host = json.loads(run.stdout)
        res["host_threads"] = args.host_threads
        res["host_pairs_per_s"] = host["pairs_per_s"]
        res["device_over_host"] = res["pairs_per_s"] / host["pairs_per_s"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
