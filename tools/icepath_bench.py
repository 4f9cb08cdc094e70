#!/usr/bin/env python3
"""The in-ice ray-path sampler, measured: samples per second of icepath_kernel and the time of
icepath_consts_kernel.  Writes profiles/icepath_bench.json and prints it as one JSON line.

    python tools/icepath_bench.py [--pairs 10000] [--warmup 3] [--steps 10] [--threads 16]
                                  [--out profiles/icepath_bench.json]

Batch: 1e4 pairs drawn by tests/iceray_cases.drawn, solved once by iceray_kernel (not timed); the
plan is made with the solver's status bytes, so only accepted rays own slots.  Each of the timed
launches of airice_icepath_launch has its two kernels bracketed by the library's device event
pairs (airice_kernel_timing); medians over the timed launches after the warm-ups.
Beside the rate, two baselines, neither a pass mark: the loop of airice_icepath_one_host over the
same rays on `threads` CPU threads (tests/cpp/icepath_driver --bench: what a user of the drop-in
has without the batch) and ray_paths_kernel's 1.1e11 samples/s on the air side.
The bound the kernel is held against: 16 B stored per sample against the 6.3 TB/s the project
takes as achievable HBM bandwidth (3.9e11 samples/s)."""
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

HBM_TB_S = 6.3
BYTES_PER_SAMPLE = 16
RAY_PATHS_SAMPLES_S = 1.1e11
KERNELS = ("icepath_consts_kernel", "icepath_kernel")
DRIVER = os.path.join(ROOT, "tests", "cpp", "icepath_driver")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icepath_bench.json"))
    args = ap.parse_args()

    import torch
    from airiceraytracing_amd import AirIceSolver, _lib
    from tests import iceray_cases as rc

    dev = torch.device("cuda:0")
    solver = AirIceSolver()
    q = rc.drawn(args.pairs, np.random.default_rng(2035))
    n = len(q)
    cols = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(3)]
    rays = torch.empty((_lib.ICERAY_FIELDS, n), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    solver.ice_rays_device(cols[0], cols[1], cols[2], rays, status)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    z0h, z1h = np.ascontiguousarray(q[:, 0]), np.ascontiguousarray(q[:, 2])
    off = solver.ice_ray_paths_plan(z0h, z1h, st)
    total = int(off[-1])
    x = torch.empty(total, dtype=torch.float64, device=dev)
    z = torch.empty(total, dtype=torch.float64, device=dev)
    count = torch.zeros(4 * n, dtype=torch.int64, device=dev)
    work = torch.empty(solver.ice_ray_paths_work_bytes(z0h, z1h, st), dtype=torch.uint8,
                       device=dev)
    stream = torch.cuda.current_stream()

    def step():
        solver.ice_ray_paths_device(cols[0], cols[1], cols[2], rays, off, count, x, z,
                                    z0_host=z0h, z1_host=z1h, status=st, work=work, stream=stream)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = {k: [] for k in KERNELS}
    _lib.kernel_timing(True)
    try:
        for _ in range(args.steps):
            for k in KERNELS:
                _lib.kernel_time(k, reset=True)
            step()
            torch.cuda.synchronize()
            for k in KERNELS:
                t, launches = _lib.kernel_time(k, reset=True)
                assert launches == 1, (k, launches)
                ms[k].append(t)
    finally:
        _lib.kernel_timing(False)
    samples = int(count.cpu().numpy().sum())
    path_ms = statistics.median(ms["icepath_kernel"])
    rate = samples / (path_ms * 1e-3)
    result = {
        "bench": "icepath",
        "pairs": n,
        "rays": int((count.cpu().numpy() > 0).sum()),
        "samples": samples,
        "slots": total,
        "warmup": args.warmup,
        "steps": args.steps,
        "icepath_kernel": {"ms_median": path_ms, "ms_min": min(ms["icepath_kernel"]),
                           "ms_max": max(ms["icepath_kernel"]), "samples_per_s": rate,
                           "stored_tb_per_s": rate * BYTES_PER_SAMPLE / 1e12},
        "icepath_consts_kernel": {"ms_median": statistics.median(ms["icepath_consts_kernel"]),
                                  "ms_min": min(ms["icepath_consts_kernel"]),
                                  "ms_max": max(ms["icepath_consts_kernel"])},
        "bound": {"bytes_per_sample": BYTES_PER_SAMPLE, "hbm_tb_per_s": HBM_TB_S,
                  "samples_per_s": HBM_TB_S * 1e12 / BYTES_PER_SAMPLE,
                  "fraction_reached": rate * BYTES_PER_SAMPLE / (HBM_TB_S * 1e12)},
        "baselines": {"ray_paths_kernel_samples_per_s": RAY_PATHS_SAMPLES_S,
                      "of_ray_paths_kernel": rate / RAY_PATHS_SAMPLES_S},
    }
    if os.path.exists(DRIVER):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "rows.bin")
            np.ascontiguousarray(q, dtype=np.float64).tofile(path)
            run = subprocess.run([DRIVER, "--bench", path, str(args.threads)],
                                 capture_output=True, text=True, check=True)
        host = json.loads(run.stdout)
        result["baselines"]["one_host_loop"] = host
        result["baselines"]["over_one_host_loop"] = rate / host["samples_per_s"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
