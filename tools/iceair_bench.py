#!/usr/bin/env python3
"""Throughput of the ice-to-air direct ray (iceair_kernel) and of the first-arrival tracer (the
geometry, iceray_kernel and select launches), written to profiles/iceair_bench.json.

    python tools/iceair_bench.py [--triples 1000000] [--emitters 1000] [--antennas 1000]
                                 [--warmup 3] [--steps 10] [--host-threads 16] [--out PATH]

Ice-to-air: --triples rows of the draw of tests/iceair_cases.py, inputs and outputs resident on
the device, each timed launch bracketed by a device event pair on the launch stream, every shape
warmed up first; the median and the range of the steps, triples per second, mean residual
evaluations per triple and evaluations per second.  --host-threads N runs
tests/cpp/iceair_driver --bench on N CPU threads over the first --host-triples rows: the same
source compiled for the host.
First arrivals: --emitters x --antennas in cross mode (the emitters of a shower, the antennas of a
station, drawn around each other), the same way for the whole call, and -- with the library's
kernel timers on -- the three kernels' times separately, so that what the geometry and select
launches add to iceray_kernel is visible."""
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

FIRST_KERNELS = ("icefirst_geom_kernel", "iceray_kernel", "icefirst_select_kernel")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triples", type=int, default=1_000_000)
    ap.add_argument("--emitters", type=int, default=1000)
    ap.add_argument("--antennas", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2029)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-triples", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iceair_bench.json"))
    args = ap.parse_args()

    import torch
    from airiceraytracing_amd import AirIceSolver, _lib
    from tests import iceair_cases as cases

    dev = torch.device("cuda:0")
    solver = AirIceSolver()
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(args.seed)

    # ---- ice to air
    n = args.triples
    q = cases.drawn(n, rng)
    cols = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(3)]
    out = torch.empty((_lib.ICEAIR_FIELDS, n), dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    air = timed(lambda: solver.ice_to_air_device(*cols, out, st, stream=stream), stream,
                args.warmup, args.steps)
    evals = float(out[_lib.ICEAIR_EVALS].sum().item())
    sec = air["ms_median"] * 1e-3
    air.update({
        "triples": n, "triples_per_s": n / sec, "evals_per_triple": evals / n,
        "evals_per_s": evals / sec,
        "iterations_per_triple": float(out[_lib.ICEAIR_ITERS].mean().item()),
        "at_the_iteration_limit": int((out[_lib.ICEAIR_ITERS] == 100).sum().item()),
        "accepted": int((st == _lib.ICEAIR_ACCEPTED).sum().item()),
    })
    if args.host_threads > 0:
        m = min(args.host_triples, n)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "rows.bin")
            np.ascontiguousarray(q[:m]).tofile(path)
            run = subprocess.run([os.path.join(ROOT, "tests", "cpp", "iceair_driver"), "--bench",
                                  path, str(args.host_threads)], capture_output=True, text=True,
                                 check=True)
        host = json.loads(run.stdout)
        air["host_threads"] = args.host_threads
        air["host_triples"] = m
        air["host_triples_per_s"] = host["triples_per_s"]
        air["device_over_host"] = air["triples_per_s"] / host["triples_per_s"]
    del cols, out, st

    # ---- first arrivals, cross mode: a shower's emitters x a station's antennas
    n_tx, n_rx = args.emitters, args.antennas
    pairs = n_tx * n_rx
    tx = np.stack([20 * rng.random(n_tx) - 10, 20 * rng.random(n_tx) - 10,
                   -1000 + 999 * rng.random(n_tx)])
    rx = np.stack([3000 * rng.random(n_rx) - 1500, 3000 * rng.random(n_rx) - 1500,
                   -200 + 199 * rng.random(n_rx)])
    t, r = torch.from_numpy(tx).to(dev), torch.from_numpy(rx).to(dev)
    out = torch.empty((_lib.ICEFIRST_FIELDS, pairs), dtype=torch.float64, device=dev)
    st = torch.empty(pairs, dtype=torch.uint8, device=dev)
    work = torch.empty(solver.ice_first_arrivals_work_bytes(pairs), dtype=torch.uint8, device=dev)

    def step():
        solver.ice_first_arrivals_device(t, r, out, work=work, pairing="cross", status=st,
                                         stream=stream)

    first = timed(step, stream, args.warmup, args.steps)
    for k in FIRST_KERNELS:
        _lib.kernel_time(k)  # reset
    _lib.kernel_timing(True)
    try:
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
    finally:
        _lib.kernel_timing(False)
    kernels = {}
    for k in FIRST_KERNELS:
        ms, launches = _lib.kernel_time(k)
        kernels[k] = {"ms_mean": ms / max(launches, 1), "launches": launches}
    types, counts = np.unique(out[_lib.ICEFIRST_RAY_TYPE].cpu().numpy(), return_counts=True)
    first.update({
        "emitters": n_tx, "antennas": n_rx, "pairs": pairs,
        "pairs_per_s": pairs / (first["ms_median"] * 1e-3),
        "work_bytes": int(work.numel()), "kernels": kernels,
        "ray_type_counts": {str(int(a)): int(b) for a, b in zip(types, counts)},
    })

    res = {"bench": "iceair", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "ice_to_air": air, "first_arrivals": first}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
