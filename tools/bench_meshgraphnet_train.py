"""Times one MeshGraphNet training step -- forward of a sequence_length 3 rollout (context 1, two predicted steps), MSE
loss, backward -- on the HIP kernels (csrc/mgn.hip forward, csrc/mgn_bwd.hip backward, `uses_hip_training`) against the
torch composition of the same math under autograd (ops.mgn_mlp_torch / ops.mgn_layer_torch) on the same GPU: median of
alternated runs, peak memory of one step above what is allocated before it, one JSON line per shape.  The HIP path is
forced at every width (`set_fused_layers("always")`); `default_path` records what the model trains on by default
(models/mgn.py TRAIN_FUSED_MAX_WIDTH).

Shapes (batch 32, configs/training/default.yaml):
  yaml     configs/model/meshgraphnet.yaml, delaunay 32x64 (D = 34, 4 layers)
  grid128  yaml widths on grid_2d 128x256
  w48/w64  processor_size 15 at D = 48 / 64 (every encoder / decoder width the same), delaunay 32x64

    python tools/bench_meshgraphnet_train.py [--shapes yaml,grid128,w48,w64] [--reps 5] [--out FILE]

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

YAML = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, input_dim_edges=2, context_size=1,
            processor_size=4, hidden_dim_processor=34, hidden_dim_node_encoder=32, hidden_dim_edge_encoder=32,
            hidden_dim_node_decoder=32, graph_type="delaunay")


def _wide(d):
    return dict(YAML, processor_size=15, hidden_dim_processor=d, hidden_dim_node_encoder=d, hidden_dim_edge_encoder=d,
                hidden_dim_node_decoder=d)


SHAPES = {
    "yaml": (YAML, (32, 64)),
    "grid128": (dict(YAML, graph_type="grid_2d"), (128, 256)),
    "w48": (_wide(48), (32, 64)),
    "w64": (_wide(64), (32, 64)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="yaml,grid128,w48,w64")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=3, help="sequence_length (context 1 + predicted steps)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    from dlwp_benchmark_amd.models import MeshGraphNet
    from dlwp_benchmark_amd.rollout import rollout_train

    dev = "cuda:0"
    out = None
    if a.out and not a.hip_only:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")
    for name in a.shapes.split(","):
        kw, (h, w) = SHAPES[name]
        m = MeshGraphNet(**kw, graph=dict(height=h, width=w, periodic=True))
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
        m.set_fused_layers("always")         # "hip" below times the kernels at every width of the backward envelope
        if not m.uses_hip_training():
            raise SystemExit(f"{name}: outside the HIP training envelope")
        b, ctx = a.batch, kw["context_size"]
        gen = torch.Generator().manual_seed(1)
        c = torch.randn(b, 1, kw["constant_channels"], h, w, generator=gen).to(dev)
        p = torch.randn(b, a.frames, kw["prescribed_channels"], h, w, generator=gen).to(dev)
        q = torch.randn(b, a.frames, kw["prognostic_channels"], h, w, generator=gen).to(dev)

        def step(path):
            m.zero_grad(set_to_none=True)
            if path == "hip":
                y = m(constants=c, prescribed=p, prognostic=q)
            else:
                y = rollout_train(m._step_torch, ctx, c, p, q)
            loss = torch.mean((y - q[:, ctx:]) ** 2)
            loss.backward()
            return loss

        if a.hip_only:
            for _ in range(a.reps + 1):
                step("hip")
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=name, hip_training_steps=a.reps + 1)), flush=True)
            continue
        paths = ("hip", "torch")
        times = {k: [] for k in paths}
        peaks, losses, grads = {}, {}, {}
        for k in paths:                      # warm-up + peak memory + gradients of one step
            step(k)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            losses[k] = float(step(k).detach())
            torch.cuda.synchronize()
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
        err = float((grads["hip"] - grads["torch"]).norm() / grads["torch"].norm())
        line = dict(shape=name, batch=b, sequence_length=a.frames, grid=[h, w], D=kw["hidden_dim_processor"],
                    processor_size=kw["processor_size"], nodes=m.n_nodes, edges=m.n_edges,
                    params=sum(pp.numel() for pp in m.parameters()), hip_ms=round(med["hip"], 3),
                    torch_ms=round(med["torch"], 3), speedup=round(med["torch"] / med["hip"], 2),
                    hip_ms_all=[round(t, 3) for t in times["hip"]], torch_ms_all=[round(t, 3) for t in times["torch"]],
                    hip_peak_MiB=round(peaks["hip"], 1), torch_peak_MiB=round(peaks["torch"], 1),
                    loss_hip=losses["hip"], loss_torch=losses["torch"], grad_rel_l2_vs_torch=err,
                    default_path=default_path)
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
