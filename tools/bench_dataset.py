"""Times the batch gather of the device-resident dataset (dlwp_dataset_gather_f32, csrc/dataset.hip) on the GPU and writes
profiles/dataset_mi355x.json.

Per shape -- "c1": the 64x64 grid of BASELINE config C1 with one prognostic variable, batch 32; "hpx32": HEALPix 12x32x32
with three prognostic and one prescribed variable, batch 32 -- a batch of S = 15 frames with context 1, normalised, is
assembled three ways from the same store:
  * kernel        DeviceWeatherDataset.gather: one launch from a device frame table;
  * torch         a composition on the device: index_select of the frames, (x - mean) / std, nan_to_num, the input / target
                  slices made contiguous;
  * host          the numpy restatement of the reference's __getitem__ + collate (tests/dataset_ref.py) on host arrays, uploaded
                  through pinned memory by staging.DeviceStager.  This is NOT the reference's loader: that one goes through
                  xarray, which is not installed here and cannot be timed; the restatement does the same arithmetic on plain
                  arrays and is a lower bound of it.
Each form is warmed up, then timed with device events over at least a second of calls; the forms alternate in `--rounds`
rounds of one process and every round is recorded.  Batches walk a ring of item sets over a store larger than the 256 MiB
Infinity Cache.  Achieved bytes/s uses the batch's algorithmic bytes: every stored frame of a window read once, every
output written once.  Recorded, not gated.  No GPU: the tool fails.

    python tools/bench_dataset.py [--out profiles/dataset_mi355x.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dataset_ref as R  # noqa: E402
from dlwp_benchmark_amd.data import DeviceWeatherDataset  # noqa: E402
from dlwp_benchmark_amd.staging import DeviceStager  # noqa: E402

SHAPES = {       # tag -> (spatial, prognostic names, prescribed names, stored times)
    "c1": ((64, 64), ["a"], [], 32768),
    "hpx32": ((12, 32, 32), ["a", "b", "c"], ["d"], 4096),
}
BATCH, SEQ, CONTEXT, SETS = 32, 15, 1, 16


def timed(fn, min_ms=1000.0, warmup=5, reps=20):
    """(ms per call, calls timed): device-event time over at least `min_ms` of calls of fn(i)"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_ms:
            return ms / reps, reps
        reps = int(reps * max(2.0, 1.2 * min_ms / max(ms, 1e-3)))


def bench_shape(tag, dev, rounds):
    spatial, prog, pres, t = SHAPES[tag]
    plane = int(np.prod(spatial))
    names = prog + pres
    g = torch.Generator(device=dev).manual_seed(len(tag))
    store = torch.empty((t, len(names), plane), device=dev)
    for a in range(0, t, 1024):
        store[a:a + 1024] = 1e5 + 1e3 * torch.randn(store[a:a + 1024].shape, device=dev, generator=g)
    times = np.datetime64("1980-01-01T00", "h") + np.arange(t) * np.timedelta64(6, "h")
    stats = {n: {"mean": 1.0e5 + i, "std": 1.0e3 + i} for i, n in enumerate(names)}
    prog_dict = {n: [] for n in prog}
    ds = DeviceWeatherDataset(prog_dict, pres, None, times[0], times[-1], 1, None, SEQ, 0.0, True, 1, CONTEXT, times=times,
                              store=store, store_variables=[(n, None) for n in names], spatial_shape=spatial, stats=stats)
    rng = np.random.default_rng(0)
    item_sets = [rng.permutation(len(ds))[:BATCH] for _ in range(SETS)]
    bufs = []
    for items in item_sets:
        b = ds.buffers(BATCH)
        b.set_items(items)
        bufs.append(b)
    c, p = len(prog), len(pres)
    read = 4 * plane * BATCH * ((SEQ + 1) * c + SEQ * p)
    written = 4 * plane * BATCH * (SEQ * c + (SEQ - CONTEXT) * c + SEQ * p)

    def kernel(i):
        return ds.gather(bufs[i % SETS])

    mean = torch.tensor([stats[n]["mean"] for n in names], device=dev).view(1, -1, 1)
    std = torch.tensor([stats[n]["std"] for n in names], device=dev).view(1, -1, 1)
    frames_long = [b.frames.long().reshape(-1) for b in bufs]

    def composition(i):
        x = store.index_select(0, frames_long[i % SETS])
        x = ((x - mean) / std).view(BATCH, SEQ + 1, len(names), plane)
        pg = torch.nan_to_num(x[:, :, :c], nan=0.0)
        return (x[:, :SEQ, c:].contiguous() if p else None, pg[:, :SEQ].contiguous(), pg[:, 1 + CONTEXT:].contiguous())

    # the host form: numpy arrays of the same store, the restatement per sample, collate, pinned upload
    host = store.cpu().numpy()
    fields = {n: host[:, v].reshape((t,) + spatial) for v, n in enumerate(names)}
    used_times = ds.times[ds.used]

    def host_batch(i):
        samples = [R.getitem(fields, {}, R.window(ds.used, used_times, int(it), SEQ), prog_dict, pres, stats, True, CONTEXT)
                   for it in item_sets[i % SETS]]
        batch = tuple(torch.from_numpy(a) if a is not None else torch.tensor(float("nan")) for a in R.collate(samples))
        return next(iter(DeviceStager([batch], dev)))

    # the three forms agree on one batch before anything is timed
    k, c_, h = kernel(0), composition(0), host_batch(0)
    torch.cuda.synchronize()
    assert torch.equal(k[2], h[2]) and torch.equal(k[3], h[3]) and (p == 0 or torch.equal(k[1], h[1]))
    diff = float((k[2].reshape(c_[1].shape) - c_[1]).abs().max())
    rec = {"shape": tag, "spatial": list(spatial), "batch": BATCH, "sequence_length": SEQ, "context_size": CONTEXT,
           "prognostic_channels": c, "prescribed_channels": p, "store_bytes": store.numel() * 4, "bytes_read": read,
           "bytes_written": written, "kernel_vs_torch_max_abs_diff": diff, "kernel_vs_host_bitwise": True, "rounds": []}
    for _ in range(rounds):
        km, kn = timed(kernel)
        tm, tn = timed(composition)
        hm, hn = timed(host_batch, warmup=2, reps=5)
        rec["rounds"].append({"kernel_ms": km, "kernel_calls": kn, "torch_ms": tm, "torch_calls": tn, "host_ms": hm,
                              "host_calls": hn})
    km, tm, hm = (min(r[n] for r in rec["rounds"]) for n in ("kernel_ms", "torch_ms", "host_ms"))
    rec.update({"kernel_ms": km, "kernel_GBps": (read + written) / km * 1e-6, "torch_ms": tm, "torch_over_kernel": tm / km,
                "host_ms": hm, "host_over_kernel": hm / km})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_mi355x.json"))
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataset: no GPU -- a timing without one says nothing")
    dev = torch.device("cuda", 0)
    result = {"tool": "bench_dataset", "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
              "note": "best of the rounds in the top-level figures; every round is listed.  host = numpy restatement + pinned "
                      "upload, not the reference's xarray loader (not installed, not timed)",
              "gather": [bench_shape(tag, dev, args.rounds) for tag in SHAPES]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
