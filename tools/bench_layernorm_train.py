"""Times LayerNorm and the Linear bias / GELU / residual epilogue in training: the operators alone (forward + backward) at the
shapes the C3 / C4 / C5 training steps meet, and one scripts/train.py-style step of SwinTransformer, FourCastNet and
PanguWeather at their BASELINE widths (tools/bench_models.py CONFIGS; --batch samples, one rollout step).

Two forms alternate repeat by repeat in one process:
  hip     training._LayerNormFn (dlwp_layernorm_bwd_f32) and training._LinearFn with act / resid (dlwp_act_f32,
          dlwp_bias_act_bwd_f32)
  parent  the same tree with ops.layer_norm / ops.linear routed as before these kernels existed: torch's layer_norm, and a
          _LinearFn without epilogue followed by F.gelu and `+ resid` as autograd nodes of their own, the bias gradient a
          torch column sum.  Every other operator stays on its HIP backward (NOT DLWP_TRAIN_TORCH_BACKWARD, which switches
          them all).
One JSON line per measurement:
  kind "step"     ms_<form>: median of --steps steps after --warmup of each (eager, events around the step); _lo3 / _hi3 the
                  three fastest and slowest repeats; mem_<form> peak bytes allocated during a step; saved_<form> bytes of
                  distinct tensors the graph saved for the backward
  kind "ln"       y = ops.layer_norm(x, ...); y.backward(gy) at one [rows, C]: ms_<form> eager (at small shapes the host's
                  enqueue time), ms_graph_<form> captured in a graph and replayed (the GPU's time), mem_ / saved_ as above;
                  ms_bwd dlwp_layernorm_bwd_f32 alone (two launches), floor_frac the time of 2 reads + 1 write of the tensor at
                  the 6.3 TB/s copy rate over ms_bwd
  kind "epilogue" the same for y = ops.linear(x, fc1, act=1); y.backward(gy) (GEMMs included in both forms); ms_bwd
                  dlwp_bias_act_bwd_f32 alone with the bias gradient (two launches: reads gy and z, writes gz)

Usage: python tools/bench_layernorm_train.py [--batch 4] [--steps 15] [--warmup 3] [--only C3_swin_32x64,...]
                                             [--out profiles/layernorm_train.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_RATE = 6.3e12


def spread(ms):
    s = sorted(ms)
    return dict(med=statistics.median(s), lo3=[round(v, 4) for v in s[:3]], hi3=[round(v, 4) for v in s[-3:]])


class _ParentLinearFn(torch.autograd.Function):
    """training._LinearFn as it was: no activation, no residual, the bias gradient a torch column sum"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from dlwp_benchmark_amd import ops

        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        with torch.no_grad():
            return ops.linear_raw(x.detach(), weight.detach(), bias.detach() if bias is not None else None)

    @staticmethod
    def backward(ctx, gy):
        from dlwp_benchmark_amd import ops

        x, weight = ctx.saved_tensors
        n, k = weight.shape
        gy2 = gy.reshape(-1, n).contiguous()
        x2 = x.reshape(-1, k)
        gx = gw = gb = None
        with torch.no_grad():
            if ctx.needs_input_grad[0]:
                gx = ops.linear_raw(gy2, weight.t().contiguous(), None).view(x.shape)
            if ctx.needs_input_grad[1]:
                gw = ops.linear_raw(gy2.t().contiguous(), x2.t().contiguous(), None)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb = gy2.sum(dim=0)
        return gx, gw, gb


def parent_layer_norm(x, weight, bias, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def parent_linear_fn(x, weight, bias, act=0, resid=None):
    y = _ParentLinearFn.apply(x, weight, bias)
    y = F.gelu(y) if act == 1 else y
    return y if resid is None else y + resid


def parent_activation(z, act):
    from dlwp_benchmark_amd import training as T

    return T._ACT_FNS[int(act)](z)


class Forms:
    """switches the three routing points of training.py between the two forms; `hip` holds the (possibly recording) originals"""

    def __init__(self):
        from dlwp_benchmark_amd import training as T

        self.T = T
        self.hip = dict(layer_norm=T.layer_norm, linear_fn=T.linear_fn, activation=T.activation)
        self.real = dict(self.hip)

    def set(self, form):
        src = self.hip if form == "hip" else dict(layer_norm=parent_layer_norm, linear_fn=parent_linear_fn,
                                                  activation=parent_activation)
        for k, v in src.items():
            setattr(self.T, k, v)

    def restore(self):
        for k, v in self.real.items():
            setattr(self.T, k, v)


def measured(fn):
    """(ms, peak bytes, saved bytes) of one call of fn, which runs a forward and its backward"""
    seen = {}

    def pack(t):
        if t.is_cuda:
            seen[(t.untyped_storage().data_ptr(), t.storage_offset(), tuple(t.shape))] = t.numel() * t.element_size()
        return t

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, sum(seen.values())


def alternate(run, forms, warmup, steps):
    """run(form) -> (ms, peak bytes, saved bytes); the forms alternated repeat by repeat"""
    for _ in range(warmup):
        for f in forms:
            run(f)
    t = {f: [] for f in forms}
    mem = {f: 0 for f in forms}
    saved = {f: 0 for f in forms}
    for _ in range(steps):
        for f in forms:
            ms, m, s = run(f)
            t[f].append(ms)
            mem[f], saved[f] = max(mem[f], m), max(saved[f], s)
    row = {}
    for f in forms:
        sp = spread(t[f])
        row.update({f"ms_{f}": sp["med"], f"ms_{f}_lo3": sp["lo3"], f"ms_{f}_hi3": sp["hi3"], f"mem_{f}": mem[f],
                    f"saved_{f}": saved[f]})
    row["ratio_parent_over_hip"] = row["ms_parent"] / row["ms_hip"]
    return row


def graph_ms(fn, args):
    """fn captured in a graph (after three eager runs on a side stream) and replayed: ms per replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    for _ in range(args.warmup):
        graph.replay()
    return spread(timed(graph.replay, args))


def timed(fn, args):
    ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / args.inner)
    return ms


def bench_net(name, args, forms, ln_shapes, fc1_shapes):
    import bench_models as BM
    from dlwp_benchmark_amd.synthetic import weatherbench
    from dlwp_benchmark_amd.weights import fill_state_dict
    from oracle.make_golden import rollout_mse

    cls, cfg, _, _, (h, w) = BM.CONFIGS[name]
    model = cls(**cfg)
    fill_state_dict(model, gain=0.7)
    model = model.to("cuda:0").train()
    ctx = cfg["context_size"]
    c, p, g = (t.to("cuda:0") for t in weatherbench(args.batch, ctx + 1, h, w, prognostic_channels=cfg["prognostic_channels"]))
    real_ln, real_lin = forms.hip["layer_norm"], forms.hip["linear_fn"]

    def rec_ln(x, weight, bias, eps=1e-5):
        ln_shapes.add((x.numel() // x.shape[-1], x.shape[-1]))
        return real_ln(x, weight, bias, eps)

    def rec_lin(x, weight, bias, act=0, resid=None):
        if act == 1:
            fc1_shapes.add((x.numel() // x.shape[-1], weight.shape[1], weight.shape[0]))
        return real_lin(x, weight, bias, act=act, resid=resid)

    forms.hip.update(layer_norm=rec_ln, linear_fn=rec_lin)

    def step():
        for q in model.parameters():
            q.grad = None
        rollout_mse(model(constants=c, prescribed=p, prognostic=g), g, ctx).backward()

    def run(form):
        forms.set(form)
        return measured(step)

    try:
        row = alternate(run, ("hip", "parent"), args.warmup, args.steps)
    finally:
        forms.hip.update(layer_norm=real_ln, linear_fn=real_lin)
        forms.restore()
    del model
    torch.cuda.empty_cache()
    return dict(kind="step", config=name, batch=args.batch, rollout_steps=1, steps=args.steps, **row)


def bench_op(kind, shape, args, forms):
    from dlwp_benchmark_amd import ops

    g = torch.Generator(device="cuda:0").manual_seed(2)
    rnd = lambda *s: torch.randn(*s, device="cuda:0", generator=g)
    if kind == "ln":
        rows, c = shape
        x = (0.5 + rnd(rows, c)).requires_grad_(True)
        gamma, beta = (1 + 0.5 * rnd(c)).requires_grad_(True), (0.5 * rnd(c)).requires_grad_(True)
        gy = rnd(rows, c)
        leaves = (x, gamma, beta)
        op = lambda: ops.layer_norm(x, gamma, beta, 1e-5)
        bwd = lambda: ops.layernorm_backward(x.detach(), gamma.detach(), gy, 1e-5)
        moved = 3 * 4 * rows * c
    else:
        rows, k, n = shape
        m = torch.nn.Linear(k, n).to("cuda:0")
        x = rnd(rows, k).requires_grad_(True)
        gy, z = rnd(rows, n), rnd(rows, n)
        leaves = (x, m.weight, m.bias)
        op = lambda: ops.linear(x, m, act=1)
        bwd = lambda: ops.bias_act_backward(gy, z, 1, True)
        moved = 3 * 4 * rows * n

    def fwd_bwd():
        for t in leaves:
            t.grad = None
        op().backward(gy)

    def run(form):
        forms.set(form)
        return measured(fwd_bwd)

    try:
        row = alternate(run, ("hip", "parent"), args.warmup, args.steps)
        for form in ("hip", "parent"):
            forms.set(form)
            sp = graph_ms(fwd_bwd, args)
            row.update({f"ms_graph_{form}": sp["med"], f"ms_graph_{form}_lo3": sp["lo3"], f"ms_graph_{form}_hi3": sp["hi3"]})
        row["graph_ratio_parent_over_hip"] = row["ms_graph_parent"] / row["ms_graph_hip"]
    finally:
        forms.restore()
    with torch.no_grad():
        for _ in range(args.warmup):
            bwd()
        k_ = spread(timed(bwd, args))
    return dict(kind=kind, shape=list(shape), steps=args.steps, **row, ms_bwd=k_["med"], ms_bwd_lo3=k_["lo3"], ms_bwd_hi3=k_["hi3"],
                floor_frac=(moved / COPY_RATE) / (k_["med"] * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layernorm_train.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_layernorm_train.py measures on an MI355X: no GPU found")
    configs = [t for t in args.only.split(",") if t] or ["C3_swin_32x64", "C4_fourcastnet_128x256", "C5_pangu_128x256x13"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    forms = Forms()
    ln_shapes, fc1_shapes = set(), set()
    for name in configs:
        emit(bench_net(name, args, forms, ln_shapes, fc1_shapes))
    for shape in sorted(ln_shapes):
        emit(bench_op("ln", shape, args, forms))
    for shape in sorted(fc1_shapes):
        emit(bench_op("epilogue", shape, args, forms))


if __name__ == "__main__":
    main()
