"""Times one GraphCastNet training step -- forward of a sequence_length 3 rollout (context 1, two predicted steps), MSE
loss, backward -- on the HIP kernels (csrc/graphcast.hip forward, csrc/graphcast_bwd.hip backward, `set_hip_training`)
against the torch composition of the same math under autograd (`_step_torch`) on the same GPU: median of alternated
runs, peak memory of one step above what is allocated before it, the gradients' rel-L2 between the two paths, one JSON
line per shape.  `default_path` records what the model trains on by default (models/graphcast.py HIP_TRAINING_DEFAULT).

Shapes (configs/model/graphcast.yaml: D = 512, 16 processor layers, level-3 multimesh):
  yaml_b1 / yaml_b4 / yaml_b<N>   32x64 at batch 1, 4, N (--big-batch, default 32)
  l3_64x128_b1                    64x128, level 3, batch 1

    python tools/bench_graphcast_train.py [--shapes yaml_b1,yaml_b4,yaml_b32,l3_64x128_b1] [--reps 5] [--out FILE]

A shape whose composition step runs out of memory is reported with "torch": "out of memory" and timed on HIP alone.
--hip-only runs only the HIP training step (`--reps` times after one warm-up) and times nothing: the command to put
under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

YAML = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, input_dim_mesh_nodes=3, input_dim_edges=4,
            processor_layers=16, hidden_layers=1, hidden_dim=512, aggregation="sum", activation_fn="silu",
            norm_type="LayerNorm", context_size=1)


def _shape(name):
    if name.startswith("yaml_b"):
        return (32, 64), int(name[len("yaml_b"):])
    if name == "l3_64x128_b1":
        return (64, 128), 1
    raise SystemExit(f"unknown shape {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="yaml_b1,yaml_b4,yaml_b32,l3_64x128_b1")
    ap.add_argument("--frames", type=int, default=3, help="sequence_length (context 1 + predicted steps)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    from dlwp_benchmark_amd.models import GraphCastNet

    dev = "cuda:0"
    out = None
    if a.out and not a.hip_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")
    for name in a.shapes.split(","):
        (h, w), b = _shape(name)
        m = GraphCastNet("icospheres_l3.json", input_height=h, input_width=w, **YAML)
        torch.manual_seed(0)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn_like(p) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 5.0))
            for mod in m.modules():
                if isinstance(mod, torch.nn.LayerNorm):
                    mod.weight.add_(1.0)
        m.invalidate_packed()
        m = m.to(dev).train()
        default_path = "hip" if m.uses_hip_training() else "torch composition"
        gen = torch.Generator().manual_seed(1)
        c = torch.randn(b, 1, YAML["constant_channels"], h, w, generator=gen).to(dev)
        p = torch.randn(b, a.frames, YAML["prescribed_channels"], h, w, generator=gen).to(dev)
        q = torch.randn(b, a.frames, YAML["prognostic_channels"], h, w, generator=gen).to(dev)

        def step(path):
            m.set_hip_training(path == "hip")
            m.zero_grad(set_to_none=True)
            y = m(constants=c, prescribed=p, prognostic=q)
            loss = torch.mean((y - q[:, YAML["context_size"]:]) ** 2)
            loss.backward()
            return loss

        if a.hip_only:
            for _ in range(a.reps + 1):
                step("hip")
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=name, hip_training_steps=a.reps + 1)), flush=True)
            continue
        paths = ["hip", "torch"]
        times = {k: [] for k in paths}
        peaks, losses, grads = {}, {}, {}
        for k in list(paths):                # warm-up + peak memory + gradients of one step
            try:
                step(k)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                losses[k] = float(step(k).detach())
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                m.zero_grad(set_to_none=True)
                torch.cuda.empty_cache()
                paths.remove(k)
                continue
            peaks[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            grads[k] = torch.cat([pp.grad.detach().double().flatten() for pp in m.parameters()])
        for _ in range(a.reps):
            for k in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(k)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        line = dict(shape=name, batch=b, sequence_length=a.frames, grid=[h, w], D=YAML["hidden_dim"],
                    processor_layers=YAML["processor_layers"], mesh_nodes=m.n_mesh, mesh_edges=int(m.mesh_src.numel()),
                    params=sum(pp.numel() for pp in m.parameters()), default_path=default_path)
        for k in ("hip", "torch"):
            if k in med:
                line.update({f"{k}_ms": round(med[k], 3), f"{k}_ms_all": [round(t, 3) for t in times[k]],
                             f"{k}_peak_MiB": round(peaks[k], 1), f"loss_{k}": losses[k]})
            else:
                line[k] = "out of memory"
        if len(med) == 2:
            line.update(speedup=round(med["torch"] / med["hip"], 3), peak_ratio=round(peaks["hip"] / peaks["torch"], 3),
                        grad_rel_l2_vs_torch=float((grads["hip"] - grads["torch"]).norm() / grads["torch"].norm()))
        print(json.dumps(line), flush=True)
        if out is not None:                  # line by line: a later shape that fails leaves the earlier lines
            out.write(json.dumps(line) + "\n")
            out.flush()
        del m, grads
        torch.cuda.empty_cache()
    if out is not None:
        out.close()


if __name__ == "__main__":
    main()
