"""Times the HEALPix -> lat-lon remap (ops.healpix_to_latlon, dlwp_healpix_to_latlon_f32) against the torch composition of the
same table on the same tensors, `(x[:, index.long()] * weight).sum(-1)`, at the plane count of an evaluation batch
(16 samples x 15 lead times x 8 variables) on three meshes.

Per shape one JSON line:
  ms_hip / ms_torch   median over --reps of HIP-event brackets around --inner back-to-back calls, divided by --inner; the two
                      are alternated bracket by bracket in one process, after --warmup brackets of each
  bytes               what the algorithm has to move: planes (12 n^2 + cells) 4 + cells 32
  hbm_peak_frac       bytes / ms_hip against the HBM peak (8.0 TB/s); inputs of these sizes fit the 256 MiB Infinity Cache at
                      nside 8 and 32, so a fraction above what HBM sustains says the planes came from cache
  max_abs_diff        largest difference of the two results (the torch sum adds the four products in another order)

Usage: python tools/bench_healpix_remap.py [--planes 1920] [--reps 15] [--inner 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
SHAPES = [(8, 32, 64), (32, 180, 360), (64, 180, 360)]     # (nside, H, W)


def bracket(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    return e0, e1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planes", type=int, default=16 * 15 * 8)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_healpix_remap: no GPU; a timing taken anywhere else says nothing")

    from dlwp_benchmark_amd import healpix as H
    from dlwp_benchmark_amd import ops

    dev = torch.device("cuda:0")
    lines = []
    for nside, h, w in SHAPES:
        lats, lons = H.reference_grid(h, w)
        table = H.device_latlon_table(nside, lats, lons, dev)
        index64 = table.index.long()
        gen = torch.Generator(device=dev).manual_seed(nside)
        x = torch.randn(args.planes, 12, nside, nside, device=dev, generator=gen)
        flat = x.view(args.planes, -1)
        y = torch.empty(args.planes, h, w, device=dev)
        hip = lambda: ops.healpix_to_latlon(x, lats, lons, out=y)
        tor = lambda: (flat[:, index64] * table.weight).sum(-1)
        diff = float((hip().view(args.planes, -1) - tor()).abs().max())
        for _ in range(args.warmup):
            bracket(hip, args.inner)
            bracket(tor, args.inner)
        torch.cuda.synchronize()
        ev = {"hip": [], "torch": []}
        for _ in range(args.reps):
            ev["hip"].append(bracket(hip, args.inner))
            ev["torch"].append(bracket(tor, args.inner))
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) / args.inner for a, b in v] for k, v in ev.items()}
        cells = h * w
        nbytes = args.planes * (12 * nside * nside + cells) * 4 + cells * 32
        ms_hip, ms_torch = statistics.median(ms["hip"]), statistics.median(ms["torch"])
        line = {"op": "healpix_to_latlon", "nside": nside, "grid": [h, w], "planes": args.planes, "ms_hip": round(ms_hip, 5),
                "ms_hip_min_max": [round(min(ms["hip"]), 5), round(max(ms["hip"]), 5)], "ms_torch": round(ms_torch, 5),
                "ms_torch_min_max": [round(min(ms["torch"]), 5), round(max(ms["torch"]), 5)],
                "speedup": round(ms_torch / ms_hip, 2), "bytes": nbytes, "gbytes_per_s_hip": round(nbytes / ms_hip / 1e6, 1),
                "hbm_peak_frac": round(nbytes / (ms_hip * 1e-3) / HBM_PEAK, 4), "max_abs_diff": diff,
                "reps": args.reps, "inner": args.inner}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del x, flat, y
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
