"""Times SpectralConv2d and FNO2DModule rollouts across channel widths (B = 32, 64 x 64 grid).

Width 32 runs the specialised 32-channel kernels (csrc/fno_kernels.hip), every other width the width-generic path
(csrc/spectral_any.hip).  For each row: ms per call / per rollout step, and the fraction of the HBM bound -- the bytes
the row must move, from the shapes alone, at the measured copy rate of 6.29 TB/s:

  SpectralConv2d   x + y + the complex weights (one read of each)
  FNO step         every tensor the generic launch sequence reads or writes once per step: lifting (x_t, the lifting
                   hidden twice, h), per layer (h twice, the spectral output twice, h out, spectral + skip weights),
                   projection (h, the projection hidden twice, the output and the residual).  The fused 32-channel
                   step moves far less than this; its row is there to compare times, not fractions.

Usage: python tools/bench_fno_width.py [--widths 16,32,64,128,256] [--ops spectral,fno] [--steps 10] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_BYTES_PER_S = 6.29e12
B, H, W = 32, 64, 64


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def spectral_row(c, reps, dev):
    from dlwp_benchmark_amd.models import SpectralConv2d

    m1 = m2 = 12
    mod = SpectralConv2d(c, c, m1, m2).to(dev).eval()
    x = torch.randn(B, c, H, W, device=dev)
    with torch.no_grad():
        ms = _time(lambda: mod(x), reps)
    nbytes = 2 * B * c * H * W * 4 + 2 * c * c * m1 * m2 * 8
    return dict(op="SpectralConv2d", channels=c, batch=B, grid=[H, W], modes=[m1, m2], ms=ms, bytes=nbytes,
                hbm_fraction=nbytes / COPY_BYTES_PER_S / (ms * 1e-3))


def fno_row(hidden, steps, reps, dev):
    from dlwp_benchmark_amd.models import FNO2DModule
    from dlwp_benchmark_amd.weights import fill_state_dict

    lift = proj = 256
    layers, modes = 4, [12, 12]
    m = FNO2DModule(n_modes=modes, constant_channels=0, prescribed_channels=0, prognostic_channels=1,
                    hidden_channels=hidden, lifting_channels=lift, projection_channels=proj, n_layers=layers,
                    context_size=1)
    fill_state_dict(m, std_fn=lambda n, s: (0.85 / s[0] ** 0.5) if "convs.weight" in n else None, gain=0.85)
    m = m.to(dev).eval()
    prog = torch.randn(B, steps + 1, 1, H, W, device=dev)
    ms = _time(lambda: m(prognostic=prog), reps) / steps
    a = B * H * W * 4                       # bytes of one channel plane over the batch
    n_modes = modes[0] * (modes[1] // 2 + 1)
    nbytes = a * (1 + 2 * lift + hidden)                                        # lifting
    nbytes += layers * (a * 5 * hidden + hidden * hidden * (n_modes * 8 + 4))   # layers
    nbytes += a * (hidden + 2 * proj + 2)                                       # projection
    return dict(op="FNO2DModule step", hidden=hidden, lifting=lift, projection=proj, layers=layers, batch=B,
                grid=[H, W], modes=modes, steps=steps, ms=ms, bytes=nbytes,
                hbm_fraction=nbytes / COPY_BYTES_PER_S / (ms * 1e-3), path="specialised" if hidden == 32 else "generic")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="16,32,64,128,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ops", default="spectral,fno", help="which rows: spectral, fno or both")
    ap.add_argument("--out", default=None, help="also write the rows as JSON lines to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for c in [int(v) for v in args.widths.split(",")]:
        if "spectral" in args.ops:
            rows.append(spectral_row(c, args.reps, dev))
        if "fno" in args.ops:
            rows.append(fno_row(c, args.steps, args.reps, dev))
    print(f"{'op':18s} {'width':>5s} {'ms':>9s} {'MB':>9s} {'HBM frac':>8s}")
    for r in rows:
        width = r.get("channels", r.get("hidden"))
        print(f"{r['op']:18s} {width:5d} {r['ms']:9.4f} {r['bytes'] / 1e6:9.1f} {r['hbm_fraction']:8.3f}")
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
