"""Times the pieces of the streamed soundness evaluation on the GPU and writes profiles/soundness_mi355x.json:

  * dlwp_climate_sums_acc_f32 on one chunk [B, K, C, H, W], window off and on (the window covering the chunk's second half):
    bytes read (out + target) over the time per call, beside the rate a plain device copy of the same bytes reaches in the same
    run, and the time of the torch composition of the same sums (`.double().sum(...)` and the window add) as the baseline;
  * ops.insolation for 365 x 180 x 360 beside the upload of the same tensor from pinned host memory.

Times are device-event times per call over `--reps` calls after `--warmup`, the calls walking a ring of input sets larger than
the 256 MiB Infinity Cache so that a call reads from memory; the insolation figure is also given as host wall time per call
(the tables are made on the host).  No GPU: the tool fails.

    python tools/bench_soundness.py [--out profiles/soundness_mi355x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dlwp_benchmark_amd import lib, ops  # noqa: E402

SHAPES = [(16, 8, 8, 32, 64), (4, 8, 8, 180, 360)]
RING_BYTES = 320 << 20


def event_ms(fn, n_sets, reps, warmup):
    """mean device time of fn(i) in ms, i walking the ring of input sets"""
    for i in range(warmup):
        fn(i % n_sets)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % n_sets)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_shape(shape, dev, reps, warmup):
    b, k, c, h, w = shape
    nbytes = 2 * 4 * b * k * c * h * w                      # out + target, read once
    n_sets = max(2, min(24, -(-RING_BYTES // nbytes)))
    g = torch.Generator(device=dev).manual_seed(1)
    sets = [(torch.randn(shape, device=dev, generator=g), torch.randn(shape, device=dev, generator=g)) for _ in range(n_sets)]
    dst = torch.empty(2, *shape, device=dev)
    zonal = torch.zeros(2, b, c, h, dtype=torch.float64, device=dev)
    window = torch.zeros(2, b, c, h, w, dtype=torch.float64, device=dev)
    wb, we = k // 2, k

    def copy(i):
        dst[0].copy_(sets[i][0])
        dst[1].copy_(sets[i][1])

    def kernel(win):
        def run(i):
            o, t = sets[i]
            lib.launch("dlwp_climate_sums_acc_f32", dev, o, t, zonal, window if win else None, b, k, c, h, w,
                       wb if win else 0, we if win else 0)
        return run

    def composition(win):
        def run(i):
            o, t = sets[i]
            zonal[0] += o.double().sum(dim=(1, 4))
            zonal[1] += t.double().sum(dim=(1, 4))
            if win:
                window[0] += o[:, wb:we].double().sum(dim=1)
                window[1] += t[:, wb:we].double().sum(dim=1)
        return run

    copy_ms = event_ms(copy, n_sets, reps, warmup)
    rec = {"shape": list(shape), "bytes_read": nbytes, "input_sets": n_sets, "reps": reps,
           "copy_ms": copy_ms, "copy_read_GBps": nbytes / copy_ms * 1e-6, "copy_read_plus_write_GBps": 2 * nbytes / copy_ms * 1e-6}
    for win in (False, True):
        tag = "window_on" if win else "window_off"
        km = event_ms(kernel(win), n_sets, reps, warmup)
        tm = event_ms(composition(win), n_sets, max(reps // 4, 5), max(warmup // 2, 2))
        rec[tag] = {"kernel_ms": km, "kernel_read_GBps": nbytes / km * 1e-6, "kernel_over_copy_read_rate": copy_ms / km,
                    "torch_composition_ms": tm, "torch_over_kernel": tm / km}
    return rec


def bench_insolation(dev, reps, warmup):
    t, h, w = 365, 180, 360
    dates = np.datetime64("2019-01-01T00:00:00") + np.arange(t) * np.timedelta64(24, "h")
    lat, lon = np.linspace(-89.5, 89.5, h), np.arange(w) * 1.0
    out = torch.empty(t, h, w, device=dev)
    host = torch.empty(t, h, w).pin_memory()
    dst = torch.empty(t, h, w, device=dev)
    gen_ms = event_ms(lambda i: ops.insolation(dates, lat, lon, out=out), 1, reps, warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        ops.insolation(dates, lat, lon, out=out)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) / reps * 1e3
    up_ms = event_ms(lambda i: dst.copy_(host, non_blocking=True), 1, reps, warmup)
    nbytes = 4 * t * h * w
    return {"shape": [t, h, w], "bytes": nbytes, "insolation_event_ms": gen_ms, "insolation_wall_ms": wall_ms,
            "insolation_write_GBps": nbytes / gen_ms * 1e-6, "pinned_upload_ms": up_ms, "pinned_upload_GBps": nbytes / up_ms * 1e-6,
            "upload_over_insolation_wall": up_ms / wall_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "soundness_mi355x.json"))
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soundness: no GPU -- a timing without one says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "climate_sums": [bench_shape(s, dev, args.reps, args.warmup) for s in SHAPES],
              "insolation": bench_insolation(dev, max(args.reps // 10, 10), 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
