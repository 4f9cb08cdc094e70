"""Time the table build in a two-layer firn against the one-layer build of the same grid and depth.

    python tools/firn_bench.py [--parent-lib PATH] [--asm airice_table.s] [--out profiles/firn_bench.json]

Grids: BASELINE cfg2 (4,851 x 177) and the reference's default grid (10 m x 0.1 deg), antenna at
-100 m, ice at 3000 m.  Per grid three builds are timed, cold (air-record cache off: the whole ray)
and warm (the air record is there: the ice leg only):

    parent      the one-layer build of --parent-lib (a libairice.so built from the parent commit);
                left out without it
    one_layer   this library's one-layer build (the same kernels, tools/isa_diff.py)
    layered     airice_table_launch_firn, Summit firn, A_ice = 1.775

Method: the table and every launch argument stay resident, each build is one launch bracketed by
a device event pair on the stream, the variants alternate inside every round, warm-up rounds are
dropped, the figure is the median over the rounds (min and max are kept).  A run without a GPU
fails.  --asm adds the layered kernels' registers, scratch and LDS from a device-assembly dump
(`make -C airiceraytracing_amd/csrc asm`).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRIDS = {
    "cfg2": (-10000.0, 300000.0, 20.0, 92.0, 180.0, 0.5),
    "reference_default": (-10000.0, 300000.0, 10.0, 90.1, 180.0, 0.1),
}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--asm", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grids", default=",".join(GRIDS))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("firn_bench: no GPU (a timing needs one)", file=sys.stderr)
        return 2
    from airiceraytracing_amd import AirIceSolver, Firn, _lib, make_grid

    L = _lib.lib()
    solver = AirIceSolver()
    plain = solver.medium
    summit = _lib.Medium.from_buffer_copy(bytes(plain))
    summit.A_ice = Firn.SUMMIT_A_ICE
    firn = Firn.summit()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("airice_table_launch", "airice_air_cache_limits"):
            getattr(parent, name).restype = ctypes.c_int
        parent.airice_table_launch.argtypes = L.airice_table_launch.argtypes
        parent.airice_air_cache_limits.argtypes = L.airice_air_cache_limits.argtypes
    libs = [L] + ([parent] if parent is not None else [])
    stream = torch.cuda.current_stream()
    sh = ctypes.c_void_p(stream.cuda_stream)

    def limits(entry, total):
        for lib in libs:
            _lib.check(lib.airice_air_cache_limits(entry, total), "airice_air_cache_limits")

    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "warmup_rounds": args.warmup, "depth_m": -100.0, "grids": {}}
    for gname in args.grids.split(","):
        g = make_grid(*GRIDS[gname])
        n = g.n_rays
        table = torch.empty((11, n), dtype=torch.float32, device="cuda:0")
        tp = ctypes.c_void_p(table.data_ptr())

        def one_layer(lib):
            return lambda: _lib.check(lib.airice_table_launch(
                ctypes.byref(plain), ctypes.byref(g), 0, g.table_rows, tp, None, n, sh), "table")

        def layered():
            _lib.check(L.airice_table_launch_firn(
                ctypes.byref(summit), ctypes.byref(firn), ctypes.byref(g), 0, g.table_rows, tp,
                None, n, sh), "table firn")

        variants = {"one_layer": one_layer(L), "layered": layered}
        if parent is not None:
            variants = {"parent": one_layer(parent), **variants}
        entry = {"rows": int(g.table_rows), "angle_steps": int(g.angle_steps), "rays": int(n)}
        for phase in ("cold", "warm"):
            if phase == "cold":
                limits(0, 0)
            else:
                limits(320 << 20, 640 << 20)
                for fn in variants.values():  # key, fill, first warm build
                    for _ in range(3):
                        fn()
            times = {k: [] for k in variants}
            for r in range(args.warmup + args.rounds):
                for k, fn in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(stream)
                    fn()
                    b.record(stream)
                    b.synchronize()
                    if r >= args.warmup:
                        times[k].append(a.elapsed_time(b) * 1e3)
            stats = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
                     for k, v in times.items()}
            base = "parent" if parent is not None else "one_layer"
            stats["layered_over_" + base] = (stats["layered"]["median_us"] /
                                             stats[base]["median_us"])
            entry[phase] = stats
            print(f"[{gname} {phase}] " + "  ".join(
                f"{k}={v['median_us']:.1f}us" if isinstance(v, dict) else f"{k}={v:.3f}"
                for k, v in stats.items()), flush=True)
        limits(320 << 20, 640 << 20)
        result["grids"][gname] = entry
        del table
        limits(0, 0)  # drop this grid's records before the next grid's
        limits(320 << 20, 640 << 20)
    if args.asm:
        from tools import isa_diff
        result["kernels"] = {k: v for k, v in isa_diff.resources(args.asm).items() if "firn" in k}
    text = json.dumps(result, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
