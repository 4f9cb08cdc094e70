"""Probe (GPU box): A antennas x N sources looked up (a) with A table_lookup_device launches back to
back, the only way before airice_table_lookup_launch_multi, and (b) with one multi launch of the
same queries, on one stream.  Packed cfg2-grid tables (20 m x 0.5 deg), cfg3-distributed sources as
in bench.py's lookup item; every antenna has its own depth (its own table) and its own distances.
Shapes: 16 antennas x 20,000 sources and 4 antennas x 1,000,000 sources, each with the sources in
random order and sorted by height (the distance rows permuted alike).

Per shape and order: the wall clock per batch (host clock around `reps` batches that end in a
device synchronise; (a) and (b) alternate, `rounds` times, so the spread of each is seen on the same
box at the same time) and the kernels' own time (airice_kernel_timing, in a pass of its own).  The
outputs of (a) and (b) are compared bit for bit first.

    python tools/lookup_multi_probe.py [--out profiles/NAME.json] [--rounds 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ICE_CM = 300000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    from airiceraytracing_amd import AirIceSolver, _lib
    from tests.parity import cfg3_queries
    assert torch.cuda.is_available(), "the probe needs a GPU"
    dev = torch.device("cuda:0")
    s = AirIceSolver()
    st = torch.cuda.current_stream()
    result = {"grid": "cfg2 (20 m x 0.5 deg, 92..180 deg), packed tables", "shapes": []}
    for n_ant, n_src, reps in ((16, 20000, 1000), (4, 1000000, 200)):
        depths = [-20000.0 + 500.0 * a for a in range(n_ant)]  # -200 m ... : all distinct
        at = s.antenna_tables(depths, ICE_CM, 20.0, 92.0, 180.0, 0.5, stream=st)
        assert len(at.tables) == n_ant
        txh, _, _ = cfg3_queries(n_src, seed=4242)
        dst = np.stack([cfg3_queries(n_src, seed=4243 + a)[1] for a in range(n_ant)])
        n = n_ant * n_src
        out_a = torch.empty((9, n), dtype=torch.float64, device=dev)
        out_b = torch.empty((9, n), dtype=torch.float64, device=dev)
        ok_a, ok_b, fl_a, fl_b = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(4))
        dep = [torch.full((n_src,), d, dtype=torch.float64, device=dev) for d in depths]
        work = torch.empty(int(_lib.lib().airice_table_lookup_multi_work_bytes(n_ant, n_ant)),
                           dtype=torch.uint8, device=dev)
        for order in ("random", "sorted"):
            o = np.argsort(txh, kind="stable") if order == "sorted" else np.arange(n_src)
            src = torch.from_numpy(txh[o] * 100).to(dev)
            dcm = torch.from_numpy(np.ascontiguousarray(dst[:, o]) * 100).to(dev)

            def single():
                for a in range(n_ant):
                    s.table_lookup_device(at.tables[a], src, dcm[a], dep[a], ICE_CM,
                                          out_a[:, a * n_src:], ok_a[a * n_src:],
                                          fl_a[a * n_src:], ld=n, stream=st)

            def multi():
                s.table_lookup_multi_device(at.tables, at.antenna_table, depths, src, dcm, ICE_CM,
                                            out_b, ok_b, fl_b, work=work, stream=st)

            for f in (single, multi, single, multi):  # warm-up of both
                f()
            torch.cuda.synchronize()
            same = (torch.equal(out_a.view(torch.int64), out_b.view(torch.int64)) and
                    torch.equal(ok_a, ok_b) and torch.equal(fl_a, fl_b))
            assert same, "the multi launch differs from the single-antenna launches"

            def wall(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    f()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / reps * 1e6

            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(wall(single))
                tb.append(wall(multi))
            # the kernels alone, in a pass of its own (the event pairs slow the host)
            _lib.kernel_time("lookup_kernel")
            _lib.kernel_time("lookup_multi_kernel")
            _lib.kernel_timing(True)
            for _ in range(10):
                single()
            for _ in range(10):
                multi()
            torch.cuda.synchronize()
            _lib.kernel_timing(False)
            ka, na = _lib.kernel_time("lookup_kernel")
            kb, nb = _lib.kernel_time("lookup_multi_kernel")
            row = {"n_ant": n_ant, "n_src": n_src, "order": order, "reps": reps,
                   "rounds": args.rounds, "outputs_identical": bool(same),
                   "single_launches_wall_us": {"median": float(np.median(ta)), "min": min(ta),
                                               "max": max(ta), "all": ta},
                   "multi_launch_wall_us": {"median": float(np.median(tb)), "min": min(tb),
                                            "max": max(tb), "all": tb},
                   "single_kernels_us_per_batch": ka / 10 * 1e3 if na else None,
                   "multi_kernel_us_per_batch": kb / 10 * 1e3 if nb else None,
                   "kernel_launches_timed": [int(na), int(nb)]}
            result["shapes"].append(row)
            print(f"{n_ant} x {n_src} {order}: single {np.median(ta):.1f} us "
                  f"[{min(ta):.1f}, {max(ta):.1f}]  multi {np.median(tb):.1f} us "
                  f"[{min(tb):.1f}, {max(tb):.1f}]  kernels {row['single_kernels_us_per_batch']:.1f}"
                  f" / {row['multi_kernel_us_per_batch']:.1f} us", flush=True)
        del at
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
