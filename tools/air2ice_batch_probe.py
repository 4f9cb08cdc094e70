"""Probe (GPU box): the batched Brent point-to-point solve (airice_air2ice_launch, one
air2ice_kernel launch) beside the per-call loop it replaces.

  * 10^6 queries (Tx ~ U(3100, 99000) m, D ~ U(0, 40000) m, ice 3000 m, depth ~ U(1, 300) m) in one
    launch: the kernel's time from event pairs on its stream, 3 warm-up rounds, then 7 timed ones,
    reported as median [min, max];
  * airice_rtf_eval(AIRICE_RTF_AIR2ICE) on AIRICE_SCALAR_HOST, one thread, 20,000 calls of the
    first of those queries through ctypes with preallocated buffers: the per-call rate.

A caller with 16 CPUs could run that loop on 16 threads, so the batch is worth having only above
16 x the single-thread rate; the probe says whether it is, and exits 1 when it is not.

    python tools/air2ice_batch_probe.py [--out profiles/air2ice_batch_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, WARMUP, ROUNDS, CALLS, THREADS = 1_000_000, 3, 7, 20_000, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "air2ice_batch_probe.json"))
    args = ap.parse_args()
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib
    from airiceraytracing_amd.solver import scalar_mode
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    s = AirIceSolver()
    rng = np.random.default_rng(10**6)
    q = np.stack([rng.uniform(3100, 99000, N), rng.uniform(0, 40000, N), np.full(N, 3000.0),
                  rng.uniform(1, 300, N)], axis=1)
    cols = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(4)]
    out = torch.empty((_lib.RTF_AIR2ICE_FIELDS, N), dtype=torch.float64, device=dev)
    status = torch.empty(N, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream()
    ms = []
    for r in range(WARMUP + ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        s.air2ice_device(*cols, out, status, stream=st)
        b.record(st)
        b.synchronize()
        if r >= WARMUP:
            ms.append(a.elapsed_time(b))
        print(f"round {r}: {a.elapsed_time(b):.3f} ms", flush=True)
    stat = status.cpu().numpy()
    classes = {str(k): int(v) for k, v in zip(*np.unique(stat, return_counts=True))}

    # the parent's route: one query per call on the calling thread
    L = _lib.lib()
    m = ctypes.byref(s.medium)
    qa = np.ascontiguousarray(q[:CALLS])
    o = np.zeros(_lib.RTF_AIR2ICE_FIELDS)
    po = _lib.ptr(o)
    base = qa.ctypes.data
    with scalar_mode(_lib.SCALAR_HOST):
        for i in range(200):
            L.airice_rtf_eval(m, _lib.RTF_AIR2ICE, ctypes.c_void_p(base + 32 * i), 4, po, 16)
        t0 = time.perf_counter()
        for i in range(CALLS):
            L.airice_rtf_eval(m, _lib.RTF_AIR2ICE, ctypes.c_void_p(base + 32 * i), 4, po, 16)
        per_call_us = (time.perf_counter() - t0) / CALLS * 1e6
    cases_ok = bool(np.array_equal(
        o.view(np.int64)[[12, 14, 15]],
        out[:, CALLS - 1].cpu().numpy().view(np.int64)[[12, 14, 15]]))

    med = float(np.median(ms))
    batch_rate = N / (med * 1e-3)        # queries per second
    loop_rate = 1e6 / per_call_us        # one thread
    result = {
        "queries": N, "range": "Tx U(3100,99000) m, D U(0,40000) m, ice 3000 m, depth U(1,300) m",
        "device": torch.cuda.get_device_name(0),
        "air2ice_kernel_ms": {"median": med, "min": min(ms), "max": max(ms), "all": ms,
                              "warmup_rounds": WARMUP, "timed_rounds": ROUNDS},
        "batch_queries_per_s": batch_rate,
        "batch_ns_per_query": med * 1e6 / N,
        "status_counts": classes,
        "per_call_loop": {"route": "airice_rtf_eval(AIRICE_RTF_AIR2ICE), AIRICE_SCALAR_HOST, "
                                   "one thread, ctypes", "calls": CALLS,
                          "us_per_call": per_call_us, "queries_per_s": loop_rate,
                          "last_call_status_probes_layers_equal_the_batch": cases_ok},
        "threads_assumed": THREADS,
        "batch_over_one_thread": batch_rate / loop_rate,
        "batch_over_16_threads": batch_rate / (THREADS * loop_rate),
        "beats_16_threads": bool(batch_rate > THREADS * loop_rate),
    }
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0 if result["beats_16_threads"] else 1


if __name__ == "__main__":
    sys.exit(main())
