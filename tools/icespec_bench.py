#!/usr/bin/env python3
"""Time of the attenuation spectrum (icesol_spectrum_kernel): ONE launch over F log-spaced
frequencies beside the only route the parent commit has, F consecutive icesol_kernel launches over
the same solver rows.  The draw of tests/iceray_cases.py, one JSON line.

    python tools/icespec_bench.py [--pairs 100000] [--bins 64 256] [--warmup 3] [--steps 10]

Timing: inputs, the solver's rows, the frequencies and the outputs resident on the device, each
step bracketed by a device event pair on the launch stream (the device time of the step, not the
enqueue), every shape warmed up before the timed window, the median and the spread reported.
stored_bytes_per_s counts the 16 n F bytes the spectrum stores against the 6.3 TB/s the project
takes as the memory bound; exps_walked_per_s counts 24 exps per bin for each leg that is not empty
(legs_per_pair of the 4: an empty leg is skipped)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12


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
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--bins", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=2029)
    ap.add_argument("--a0", type=float, default=1.0)
    args = ap.parse_args()

    import torch
    from airiceraytracing_amd import AirIceSolver, _lib
    from tests import iceray_cases as cases

    n = args.pairs
    q = cases.drawn(n, np.random.default_rng(args.seed))
    dev = torch.device("cuda:0")
    solver = AirIceSolver()
    z0, x1, z1 = [torch.from_numpy(np.ascontiguousarray(q[:, k])).to(dev) for k in range(3)]
    rays = torch.empty((_lib.ICERAY_FIELDS, n), dtype=torch.float64, device=dev)
    sol = torch.empty((_lib.ICESOL_FIELDS, n), dtype=torch.float64, device=dev)
    out = torch.empty((_lib.ICESOL_FIELDS, n), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream()
    solver.ice_rays_device(z0, x1, z1, rays, stream=stream)
    solver.ice_solutions_device(z0, x1, z1, rays, sol, a0=args.a0, stream=stream)
    torch.cuda.synchronize()

    res = {"bench": "icespec", "pairs": n, "steps": args.steps, "warmup": args.warmup,
           "a0": args.a0, "band_ghz": [0.05, 1.0], "hbm_bytes_per_s": HBM_BYTES_PER_S}
    has = sol[_lib.ICESOL_ATTENUATION:_lib.ICESOL_ATTENUATION + 2].cpu().numpy() != 0
    types = sol[_lib.ICESOL_RAY_TYPE:_lib.ICESOL_RAY_TYPE + 2].cpu().numpy()
    res["legs_per_pair"] = float(np.where(has, np.where(types == 1, 1, 2), 0).sum() / n)
    for f in args.bins:
        freq_host = np.exp(np.linspace(np.log(0.05), np.log(1.0), f))
        freq = torch.from_numpy(freq_host).to(dev)
        att = torch.empty((n, 2, f), dtype=torch.float64, device=dev)

        def one_launch():
            solver.ice_attenuation_spectrum_device(z0, z1, rays, sol, freq, att, a0=args.a0,
                                                   stream=stream)

        def f_launches():
            for v in freq_host:
                solver.ice_solutions_device(z0, x1, z1, rays, out, a0=args.a0, frequency=float(v),
                                            stream=stream)

        with _lib.launched("icesol_spectrum_kernel") as k:
            one = timed(one_launch, stream, args.warmup, args.steps)
        assert k.count == args.warmup + args.steps
        with _lib.launched("icesol_kernel") as k:
            many = timed(f_launches, stream, args.warmup, args.steps)
        assert k.count == f * (args.warmup + args.steps)
        # the last bin of both routes, as a sanity figure beside the times
        last = att[:, :, f - 1].cpu().numpy()
        ref = out[_lib.ICESOL_ATTENUATION:_lib.ICESOL_ATTENUATION + 2].cpu().numpy().T
        with np.errstate(invalid="ignore"):
            d = np.abs(last - ref) / np.maximum(1.0, np.abs(1 - ref))
        s = one["ms_median"] * 1e-3
        one.update(pair_bins_per_s=n * f / s,
                   exps_walked_per_s=24 * res["legs_per_pair"] * n * f / s,
                   stored_bytes_per_s=16 * n * f / s,
                   of_hbm_store_bound=16 * n * f / s / HBM_BYTES_PER_S)
        many.update(pair_bins_per_s=n * f / (many["ms_median"] * 1e-3))
        res[f"F{f}"] = {"icesol_spectrum_kernel_one_launch": one,
                        "icesol_kernel_F_launches": many,
                        "speedup": many["ms_median"] / one["ms_median"],
                        "last_bin_max_rel_difference": float(np.nanmax(d))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
