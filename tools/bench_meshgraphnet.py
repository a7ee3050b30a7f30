"""Times one MeshGraphNet rollout step, the HIP kernels (csrc/mgn.hip) against the torch composition of the same math
(ops.mgn_mlp_torch / ops.mgn_layer_torch) on the same GPU: median of alternated runs, one JSON line per shape.

Shapes (batch 32):
  yaml        configs/model/meshgraphnet.yaml, delaunay 32x64 (D = 34)
  default     the class-default widths (D = 128, processor_size 15), delaunay 32x64
  mgn32m      the paper's mgn32m_l8_d470 read as D = 470 with processor_size 16 (the reading that gives ~32M parameters)
  grid128     yaml widths on grid_2d 128x256
  w48/64/96   processor_size 15 at D = 48, 64, 96 (the crossover against the torch composition)
Bytes model of a step (for GB/s): per processor layer the edge state read and written (2 B E D) plus the node state read
twice and written once (3 B N D), fp32; encoders / decoder ignored.

    python tools/bench_meshgraphnet.py [--shapes yaml,default,mgn32m,grid128] [--reps 5] [--out FILE]

--rollout-only runs only the HIP model's own rollout (forward, `--reps` times, 3 steps each) and times nothing: the
command to put under `rocprofv3 --kernel-trace --stats`, whose stats then hold exactly the launches of the product path."""
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
SHAPES = {
    "yaml": (YAML, (32, 64)),
    "default": (dict(YAML, processor_size=15, hidden_dim_processor=128, hidden_dim_node_encoder=128,
                     hidden_dim_edge_encoder=128, hidden_dim_node_decoder=128), (32, 64)),
    "mgn32m": (dict(YAML, processor_size=16, hidden_dim_processor=470, hidden_dim_node_encoder=470,
                    hidden_dim_edge_encoder=470, hidden_dim_node_decoder=470), (32, 64)),
    "grid128": (dict(YAML, graph_type="grid_2d"), (128, 256)),
    # the class-default depth at intermediate widths: where the fused kernels stop paying (models/mgn.py FUSED_MAX_WIDTH)
    "w48": (dict(YAML, processor_size=15, hidden_dim_processor=48), (32, 64)),
    "w64": (dict(YAML, processor_size=15, hidden_dim_processor=64), (32, 64)),
    "w96": (dict(YAML, processor_size=15, hidden_dim_processor=96), (32, 64)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="yaml,default,mgn32m,grid128")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rollout-only", action="store_true")
    a = ap.parse_args()
    from dlwp_benchmark_amd.models import MeshGraphNet

    dev = "cuda:0"
    lines = []
    for name in a.shapes.split(","):
        kw, (h, w) = SHAPES[name]
        m = MeshGraphNet(**kw, graph=dict(height=h, width=w, periodic=True))
        torch.manual_seed(0)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn_like(p) / (p.shape[-1] ** 0.5 if p.dim() == 2 else 5.0))
        m.invalidate_packed()
        m = m.to(dev).eval()
        default_path = "fused" if m.uses_fused_layers() else "torch composition"
        m.set_fused_layers("always")         # "hip" below times the kernels at every width
        b = a.batch
        cin = kw["constant_channels"] + (kw["prescribed_channels"] + kw["prognostic_channels"]) * kw["context_size"]
        x = torch.randn(b, cin, h, w, device=dev)
        if a.rollout_only:
            c = torch.randn(b, 1, kw["constant_channels"], h, w, device=dev)
            p = torch.randn(b, 4, kw["prescribed_channels"], h, w, device=dev)
            q = torch.randn(b, 4, kw["prognostic_channels"], h, w, device=dev)
            for _ in range(a.reps):
                m(constants=c, prescribed=p, prognostic=q)
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=name, rollouts=a.reps, steps_per_rollout=3)), flush=True)
            continue
        fns = {"hip": m.one_step, "torch": m._step_torch}
        times = {k: [] for k in fns}
        peaks = {}
        with torch.no_grad():
            for k, f in fns.items():            # warm-up + peak memory of one step
                f(x)
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                f(x)
                torch.cuda.synchronize()
                peaks[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            for _ in range(a.reps):
                for k, f in fns.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f(x)
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3)
            y_h, y_t = m.one_step(x), m._step_torch(x)
        err = float((y_h.double() - y_t.double()).norm() / y_t.double().norm())
        d, n, e = kw["hidden_dim_processor"], m.n_nodes, m.n_edges
        layers = kw["processor_size"]
        nbytes = layers * b * (2 * e * d + 3 * n * d) * 4
        # edge MLP 3D->D->D plus node MLP 2D->D->D per layer, 2 FLOP per FMA
        flops = layers * b * 2 * (e * (3 * d * d + d * d) + n * (2 * d * d + d * d))
        med = {k: statistics.median(v) for k, v in times.items()}
        line = dict(shape=name, batch=b, grid=[h, w], D=d, processor_size=layers, nodes=n, edges=e,
                    params=sum(p.numel() for p in m.parameters()), hip_ms=round(med["hip"], 3),
                    torch_ms=round(med["torch"], 3), speedup=round(med["torch"] / med["hip"], 2),
                    hip_GBps=round(nbytes / med["hip"] / 1e6, 1), hip_TFLOPs=round(flops / med["hip"] / 1e9, 2),
                    hip_peak_MiB=round(peaks["hip"], 1), torch_peak_MiB=round(peaks["torch"], 1), rel_l2_vs_torch=err,
                    default_path=default_path)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del m
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
