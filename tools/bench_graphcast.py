"""Times one GraphCastNet step (graphcast.yaml: D = 512, 16 processor layers, level-3 mesh) on the HIP gather-GEMM
(csrc/graphcast.hip) against the torch composition, alternated, median of --reps runs of --iters steps each, at 32x64
B = 1 and B = 4 and at 64x128 B = 1.  Reports the algorithmic FLOPs of both forms (the HIP form splits the first edge Linear
and caches the static embeddings), the share of the 157.3 TFLOP/s fp32 matrix peak and the peak memory of a step.  Each form is timed eager
(one_step) and replayed from a captured graph (GraphedStep, as rollouts run with set_step_graphs(True)).
One JSON line per shape.    python tools/bench_graphcast.py [--out profiles/graphcast.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dlwp_benchmark_amd.graphs import GraphedStep  # noqa: E402
from dlwp_benchmark_amd.models import GraphCastNet  # noqa: E402

PEAK = 157.3e12


def flops(m, b, hip):
    """2 * MACs of every Linear of one step; `hip`: the split first edge Linear and no static embeddings"""
    d = m.processor.processor_layers[0].edge_mlp.model[0].out_features
    G, N = m.n_grid, m.n_mesh
    e = {k: getattr(m, f"{k}_src").numel() for k in ("mesh", "g2m", "m2g")}
    # a MeshGraphMLP has hidden_layers + 1 Linears: in -> d, (hidden_layers - 1) x d -> d, d -> out
    n_hidden = sum(1 for x in m.finale.model if isinstance(x, torch.nn.Linear)) - 2

    def mlp(rows, din, dout):
        return 2 * rows * (din * d + n_hidden * d * d + d * dout)

    def edge(ne, n_s, n_d):
        return (mlp(ne, d, d) + 2 * (n_s + n_d) * d * d) if hip else mlp(ne, 3 * d, d)

    f = mlp(G * b, m.input_dim_grid_nodes, d)
    if not hip:
        f += mlp(N, 3, d) + mlp(e["mesh"], 4, d) + mlp(e["g2m"], 4, d) + mlp(e["m2g"], 4, d)
    f += edge(e["g2m"] * b, G * b, N if hip else N * b) + mlp(N * b, 2 * d, d) + mlp(G * b, d, d)
    layers = sum(len(p.pairs()) for p in (m.processor_encoder, m.processor, m.processor_decoder))
    f += layers * (edge(e["mesh"] * b, N * b, N * b) + mlp(N * b, 2 * d, d))
    f += edge(e["m2g"] * b, N * b, G * b) + mlp(G * b, 2 * d, d) + mlp(G * b, d, m.prognostic_channels)
    return f


def time_step(step, x, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        step(x)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--shapes", default="32x64x1,32x64x4,64x128x1", help="HxWxB list")
    ap.add_argument("--forms", default="hip,torch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    forms = a.forms.split(",")
    lines = []
    for spec in a.shapes.split(","):
        h, w, b = (int(v) for v in spec.split("x"))
        torch.manual_seed(0)
        m = GraphCastNet("icospheres_l3.json", input_height=h, input_width=w, constant_channels=4, prescribed_channels=1,
                         prognostic_channels=8, hidden_dim=512, processor_layers=16).to("cuda").eval()
        x = torch.randn(b, m.input_dim_grid_nodes, h, w, device="cuda")
        res = {}
        with torch.no_grad():
            for form in forms:
                m.set_hip_step(form == "hip")
                m.one_step(x)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                m.one_step(x)
                torch.cuda.synchronize()
                try:                         # the step as rollouts replay it with set_step_graphs(True)
                    graphed = GraphedStep(m.one_step)
                    graphed(x)
                    torch.cuda.synchronize()
                except RuntimeError as err:
                    print(f"{form}: graph capture failed: {err}", file=sys.stderr)
                    graphed = None
                res[form] = dict(eager=[], graphed=[], graph=graphed,
                                 peak_mb=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)
            for _ in range(a.reps):
                for form in forms:
                    m.set_hip_step(form == "hip")
                    res[form]["eager"].append(time_step(m.one_step, x, a.iters))
                    if res[form]["graph"] is not None:
                        res[form]["graphed"].append(time_step(res[form]["graph"], x, a.iters))
        line = dict(shape=f"{h}x{w}", batch=b, hidden_dim=512, processor_layers=16)
        for form in forms:
            f = flops(m, b, form == "hip")
            line[f"{form}_gflop"] = round(f / 1e9, 2)
            for kind in ("eager", "graphed"):
                ts = sorted(res[form][kind])
                if not ts:
                    line[f"{form}_{kind}_ms"] = None
                    continue
                t = ts[len(ts) // 2]
                line[f"{form}_{kind}_ms"] = round(t, 4)
                line[f"{form}_{kind}_peak_share"] = round(f / (t * 1e-3) / PEAK, 4)
            line[f"{form}_step_peak_mb"] = round(res[form]["peak_mb"], 1)
        if "hip" in forms and "torch" in forms:
            for kind in ("eager", "graphed"):
                if line.get(f"hip_{kind}_ms") and line.get(f"torch_{kind}_ms"):
                    line[f"speedup_{kind}"] = round(line[f"torch_{kind}_ms"] / line[f"hip_{kind}_ms"], 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.writelines(json.dumps(l) + "\n" for l in lines)


if __name__ == "__main__":
    main()
