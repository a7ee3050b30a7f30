"""Times the fused spherical power spectrum sums (ops.sph_power_sums, csrc/sph_power.hip) against the two ways the same four
sums could be had without it, on the device:
  (a) "three_sht"   ops.sht of out, target and out - target (three launches, three coefficient tensors written and read back)
                    and a torch reduction of the coefficients to the four [K, C, lmax] sums in float64
  (b) "sht_torch"   the same with training.sht_torch (torch.fft + einsum on the same fp32 tables) for the transforms
at the evaluation shapes: 32 x 64, B 32, K 20, C 3 on "equiangular-centred" with lmax 32, and 128 x 256, B 8, K 20, C 13 on
"legendre-gauss" with lmax 128.

Per shape one JSON line:
  ms_fused / ms_three_sht / ms_sht_torch   median over --reps of HIP-event brackets around --inner back-to-back calls, divided by
                      --inner; the three are alternated bracket by bracket in one process, after --warmup brackets of each
  *_min_max           the spread of those brackets
  bytes_fused         out and target read once per m tile, the fp64 partials written and read, the sums written
  bytes_three_sht     out and target read, the difference written, three fields read, three coefficient tensors written and read
  rel_*               the largest difference of the candidate's sums from the fused ones, relative to the peak of each quantity

Usage: python tools/bench_sph_spectrum.py [--reps 15] [--inner 10] [--warmup 3] [--out profiles/sph_spectrum_mi355x.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("equiangular-centred", 32, 64, 32, 32, 20, 3), ("legendre-gauss", 128, 256, 128, 8, 20, 13)]


def bracket(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    return e0, e1


def reduce_coefficients(co, ct, cd, nlon):
    """the four sums [4, K, C, lmax] in float64 from complex64 coefficients [B, K, C, lmax, mmax]"""
    mmax = co.shape[-1]
    f = torch.full((mmax,), 2.0, dtype=torch.float64, device=co.device)
    f[0] = 1.0
    keep = torch.ones(mmax, dtype=torch.float32, device=co.device)       # the imaginary parts of the self-conjugate columns
    keep[0] = 0.0
    if nlon // 2 < mmax:
        f[nlon // 2] = 1.0
        keep[nlon // 2] = 0.0
    parts = []
    for c in (co, ct, cd):
        r = torch.view_as_real(c)
        parts.append((r[..., 0].double(), (r[..., 1] * keep).double()))
    (xr, xi), (yr, yi), (dr, di) = parts
    red = lambda t: (t * f).sum(-1).sum(0)
    return torch.stack([red(xr * xr + xi * xi), red(yr * yr + yi * yi), red(dr * dr + di * di), red(xr * yr + xi * yi)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sph_spectrum: no GPU; a timing taken anywhere else says nothing")

    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd import sphere as S
    from dlwp_benchmark_amd import training as T

    dev = torch.device("cuda:0")
    lines = []
    with torch.no_grad():
        for grid, nlat, nlon, lmax, b, k, c in SHAPES:
            mmax = min(lmax, nlon // 2 + 1)
            tab = S.device_tables(grid, nlat, nlon, lmax, mmax, dev)
            gen = torch.Generator(device=dev).manual_seed(nlat)
            out = torch.randn(b, k, c, nlat, nlon, device=dev, generator=gen)
            tar = out + 0.3 * torch.randn(b, k, c, nlat, nlon, device=dev, generator=gen)
            ws_bytes = ops.sph_power_workspace_bytes(out.shape, lmax, mmax)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            cands = {
                "fused": lambda: ops.sph_power_sums(out, tar, grid, lmax, mmax, workspace=ws),
                "three_sht": lambda: reduce_coefficients(ops.sht(out, grid, lmax, mmax), ops.sht(tar, grid, lmax, mmax),
                                                         ops.sht(out - tar, grid, lmax, mmax), nlon),
                "sht_torch": lambda: reduce_coefficients(T.sht_torch(out, tab), T.sht_torch(tar, tab), T.sht_torch(out - tar, tab),
                                                         nlon),
            }
            ref = cands["fused"]()
            peak = ref.abs().amax(-1, keepdim=True)
            peak[3] = torch.sqrt(peak[0] * peak[1])
            rel = {name: float(((fn() - ref).abs() / peak).max()) for name, fn in cands.items() if name != "fused"}
            for _ in range(args.warmup):
                for fn in cands.values():
                    bracket(fn, args.inner)
            torch.cuda.synchronize()
            ev = {name: [] for name in cands}
            for _ in range(args.reps):
                for name, fn in cands.items():
                    ev[name].append(bracket(fn, args.inner))
            torch.cuda.synchronize()
            ms = {name: [a.elapsed_time(e) / args.inner for a, e in v] for name, v in ev.items()}
            med = {name: statistics.median(v) for name, v in ms.items()}
            units = b * k * c
            field, spec, sums = units * nlat * nlon * 4, units * lmax * mmax * 8, 4 * k * c * lmax * 8
            mtiles = ws_bytes // (units * 4 * lmax * 8)
            line = {"op": "sph_power_sums", "grid": grid, "nlat": nlat, "nlon": nlon, "lmax": lmax, "mmax": mmax, "batch": b,
                    "steps": k, "channels": c, "m_tiles": mtiles}
            for name in cands:
                line[f"ms_{name}"] = round(med[name], 5)
                line[f"ms_{name}_min_max"] = [round(min(ms[name]), 5), round(max(ms[name]), 5)]
            line.update({"fused_over_three_sht": round(med["fused"] / med["three_sht"], 3),
                         "fused_over_sht_torch": round(med["fused"] / med["sht_torch"], 3),
                         "bytes_fused": 2 * field * mtiles + 2 * ws_bytes + sums, "bytes_three_sht": 6 * field + 6 * spec + sums,
                         "workspace_bytes": ws_bytes, "rel_three_sht": rel["three_sht"], "rel_sht_torch": rel["sht_torch"],
                         "reps": args.reps, "inner": args.inner})
            print(json.dumps(line), flush=True)
            lines.append(line)
            del out, tar, ws
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
