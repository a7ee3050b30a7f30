"""Times dlwp_ensemble_sums_acc_f32 (csrc/ensemble_scores.hip) on the GPU and writes profiles/ensemble_mi355x.json.

Per member count M in {4, 16, 64}, on one chunk [M, B = 16, K = 14, C = 1, 64, 64] (the C1 grid) and its target:
  * the kernel call (partials + ordered combine), bytes read = (M + 1) planes, over the time per call;
  * a device-to-device copy of the same bytes in the same run (what reading them once costs when they are also written);
  * the torch composition of the same sums and ranks on the device: a sort of the whole ensemble along the member axis, the
    mean / variance / absolute-error reductions, the sorted-form pair sum and a bincount for the ranks.
Times are device-event times per call over `--reps` calls after `--warmup`, the calls walking a ring of input sets larger than
the 256 MiB Infinity Cache so that a call reads from memory; the three are measured in `--rounds` alternating rounds and every
round is recorded, so the spread is in the file.  The timings are recorded, not gated.  No GPU: the tool fails.

    python tools/bench_ensemble.py [--out profiles/ensemble_mi355x.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dlwp_benchmark_amd import lib  # noqa: E402
from dlwp_benchmark_amd.metrics import latitude_weights  # noqa: E402

MEMBERS = (4, 16, 64)
CHUNK = (16, 14, 1, 64, 64)          # B, K, C, H, W
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


def bench_members(m, dev, reps, warmup, rounds):
    b, k, c, h, w = CHUNK
    plane = b * k * c * h * w
    nbytes = 4 * (m + 1) * plane
    n_sets = max(2, min(24, -(-RING_BYTES // nbytes)))
    g = torch.Generator(device=dev).manual_seed(m)
    sets = []
    for _ in range(n_sets):
        y = torch.randn(CHUNK, device=dev, generator=g)
        sets.append((y + torch.randn((m,) + CHUNK, device=dev, generator=g), y))
    dst = torch.empty((m + 1,) + CHUNK, device=dev)
    latw = latitude_weights(torch.linspace(-90 + 90 / h, 90 - 90 / h, h)).to(dev)
    sums = torch.zeros(4, k, c, dtype=torch.float64, device=dev)
    ranks = torch.zeros(k, c, m + 1, dtype=torch.int64, device=dev)
    ws = lib.workspace(max(int(lib.load().dlwp_ensemble_sums_workspace_bytes(b, k, c, h, w)), 8), dev)
    coef = (2.0 * torch.arange(m, device=dev) - m + 1).view(m, 1, 1, 1, 1, 1)
    wt = latw.view(1, 1, 1, h, 1)
    kc = (torch.arange(k * c, device=dev) * (m + 1)).view(1, k, c, 1, 1)

    def copy(i):
        dst[:m].copy_(sets[i][0])
        dst[m].copy_(sets[i][1])

    def kernel(i):
        x, y = sets[i]
        lib.launch("dlwp_ensemble_sums_acc_f32", dev, x, y, latw, None, sums, ranks, m, plane, b, k, c, h, w, k, 0, ws, ws.numel())

    def composition(i):
        x, y = sets[i]
        mean = x.mean(dim=0)
        sums[0] += (wt * (mean - y) ** 2).double().sum(dim=(0, 3, 4))
        sums[1] += (wt * x.var(dim=0, unbiased=True)).double().sum(dim=(0, 3, 4))
        sums[2] += (wt * (x - y).abs().mean(dim=0)).double().sum(dim=(0, 3, 4))
        sums[3] += (wt * (coef * x.sort(dim=0).values).sum(dim=0)).double().sum(dim=(0, 3, 4))
        r = (x < y).sum(dim=0) + kc
        ranks.view(-1).add_(torch.bincount(r.reshape(-1), minlength=k * c * (m + 1)))

    # the two forms agree on one set before anything is timed
    kernel(0)
    got = (sums.clone(), ranks.clone())
    sums.zero_()
    ranks.zero_()
    composition(0)
    torch.cuda.synchronize()
    rel = float(((got[0] - sums).abs() / sums.abs().clamp_min(1e-30)).max())
    assert torch.equal(got[1], ranks) and rel < 1e-4, (m, rel)

    rec = {"members": m, "chunk": list(CHUNK), "bytes_read": nbytes, "input_sets": n_sets, "reps": reps,
           "kernel_vs_composition_max_rel_diff": rel, "rounds": []}
    for _ in range(rounds):
        cm = event_ms(copy, n_sets, reps, warmup)
        km = event_ms(kernel, n_sets, reps, warmup)
        tm = event_ms(composition, n_sets, max(reps // 10, 5), max(warmup // 5, 2))
        rec["rounds"].append({"copy_ms": cm, "kernel_ms": km, "torch_composition_ms": tm})
    cm, km, tm = (min(r[name] for r in rec["rounds"]) for name in ("copy_ms", "kernel_ms", "torch_composition_ms"))
    rec.update({"copy_ms": cm, "copy_read_GBps": nbytes / cm * 1e-6, "kernel_ms": km, "kernel_read_GBps": nbytes / km * 1e-6,
                "kernel_over_copy_time": km / cm, "torch_composition_ms": tm, "torch_over_kernel": tm / km})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_mi355x.json"))
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble: no GPU -- a timing without one says nothing")
    dev = torch.device("cuda", 0)
    result = {"tool": "bench_ensemble", "device": torch.cuda.get_device_name(0),
              "note": "best of the rounds in the top-level figures; every round is listed",
              "ensemble_sums": [bench_members(m, dev, args.reps, args.warmup, args.rounds) for m in MEMBERS]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
