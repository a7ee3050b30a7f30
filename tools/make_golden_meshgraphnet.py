"""Writes tests/golden/mgn_*.npz: MeshGraphNet rollouts, gradient cases (one step, and multi-step training
rollouts: mgn_train_*), graphs and the state-dict layout, all from the REAL
reference class (models/mgn/meshgraphnet.py) on the CPU, imported through oracle.ref_import, with the filler weights of
dlwp_benchmark_amd.weights (`fill`, below).  Only outputs are stored; each file carries the weight SHA and the case, and a
test regenerates weights and inputs by name.

dgl is not installed here, so this tool carries a stand-in (`_install_dgl`).  It holds graph bookkeeping only --
from_networkx with the sorted node relabel, to_bidirected as the simple symmetric graph, batch as node offsets, edges,
num_nodes, ndata / edata / srcdata / dstdata, local_scope -- and the two message functions the reference calls: apply_edges
running the reference's own concat_message_function, and update_all(copy_e, sum | mean) as an index_add (a node without
incoming edges gets 0).  DGL's exact semantics are an ASSUMPTION of these fixtures, most of all the node numbering
h * width + w that the forward's "(b h w) d" rearrange presumes.  `s3fs` and `git` get empty stand-ins (imported by the
modulus utilities, never called).

The reference's in-model rollout crashes on its second step (`torch.stack(outs)...].to`, meshgraphnet.py:471), so
multi-step trajectories are driven one step at a time from here, like oracle/make_golden.py reference_rollout.

Runs where the reference tree is available:  python tools/make_golden_meshgraphnet.py"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dlwp_benchmark_amd import weights as W  # noqa: E402
from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

YAML = dict(constant_channels=4, prescribed_channels=1, prognostic_channels=8, input_dim_edges=2, context_size=1,
            processor_size=4, message_passing_steps=1, num_layers_node_processor=2, num_layers_edge_processor=2,
            hidden_dim_processor=34, hidden_dim_node_encoder=32, num_layers_node_encoder=2, hidden_dim_edge_encoder=32,
            num_layers_edge_encoder=2, hidden_dim_node_decoder=32, num_layers_node_decoder=2, aggregation="sum",
            do_concat_trick=False, num_processor_checkpoint_segments=0, graph_type="delaunay")


def _small(**kw):
    base = dict(constant_channels=2, prescribed_channels=0, prognostic_channels=3, input_dim_edges=2, context_size=1,
                processor_size=2, hidden_dim_processor=32, hidden_dim_node_encoder=32, hidden_dim_edge_encoder=16,
                hidden_dim_node_decoder=32)
    base.update(kw)
    return base


# tag -> (ctor kwargs, graph (H, W, periodic), batch, frames)
ROLLOUT_CASES = {
    "yaml_delaunay_32x64": (YAML, (32, 64, True), 2, 4),
    "grid_mean_mp2_16x16": (_small(graph_type="grid_2d", aggregation="mean", message_passing_steps=2,
                                   num_layers_node_processor=1, num_layers_edge_processor=1, hidden_dim_processor=48),
                            (16, 16, True), 2, 3),
    "stencil8_16x32": (_small(graph_type="grid_2d_8stencil", input_dim_edges=3, num_layers_node_processor=3,
                              num_layers_edge_processor=3, hidden_dim_processor=64), (16, 32, True), 2, 3),
    "default_widths_delaunay_8x16": (dict(constant_channels=2, prescribed_channels=1, prognostic_channels=2, context_size=1,
                                          graph_type="delaunay"), (8, 16, True), 1, 3),
    "d470_delaunay_8x16": (_small(graph_type="delaunay", hidden_dim_processor=470, hidden_dim_node_encoder=470,
                                  hidden_dim_edge_encoder=470, hidden_dim_node_decoder=470), (8, 16, True), 1, 2),
    "ctx2_prescribed_grid_8x16": (_small(graph_type="grid_2d", context_size=2, prescribed_channels=2), (8, 16, True), 2, 4),
    "grid_nonperiodic_8x16": (_small(graph_type="grid_2d"), (8, 16, False), 2, 3),
}
GRAD_CASE = ("grad_yaml_8x16", dict(YAML), (8, 16, True), 2, 2)
# training gradients through multi-step rollouts (stepwise_rollout), tag -> (ctor kwargs, graph, batch, frames):
# `mgn_train_<tag>.npz`, the HIP backward's fixtures (tests/test_meshgraphnet_train_gpu.py)
TRAIN_GRAD_CASES = {
    "mean_mp2_grid_8x16": (_small(graph_type="grid_2d", aggregation="mean", message_passing_steps=2), (8, 16, True), 2, 3),
    "stencil8_8x16": (_small(graph_type="grid_2d_8stencil", input_dim_edges=3), (8, 16, True), 2, 3),
    "ctx2_prescribed_grid_8x16": (_small(graph_type="grid_2d", context_size=2, prescribed_channels=2), (8, 16, True), 2, 4),
    "grid_nonperiodic_8x16": (_small(graph_type="grid_2d"), (8, 16, False), 2, 3),
    "d48_delaunay_8x16": (_small(graph_type="delaunay", hidden_dim_processor=48, hidden_dim_node_encoder=48,
                                 hidden_dim_edge_encoder=48, hidden_dim_node_decoder=48), (8, 16, True), 2, 3),
    "d64_delaunay_8x16": (_small(graph_type="delaunay", hidden_dim_processor=64, hidden_dim_node_encoder=64,
                                 hidden_dim_edge_encoder=64, hidden_dim_node_decoder=64), (8, 16, True), 2, 3),
}
GRAPH_CASES = [(t, h, w) for t in ("grid_2d", "grid_2d_8stencil", "delaunay") for h, w in ((32, 64), (16, 32))]


def fill(model: torch.nn.Module) -> str:
    """fill_state_dict, then LayerNorm scales around 1 (the filler gives 1-D weights N(0, 0.02), which would shrink every
    normalised output): a MeshGraphMLP's only 1-D `.weight` is its LayerNorm's"""
    sha = W.fill_state_dict(model, gain=1.0)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(".weight") and p.dim() == 1:
                p.add_(1.0)
    return sha


def case_inputs(tag, kw, batch, frames, hw):
    """(constants, prescribed, prognostic) of a case, regenerated by name"""
    h, w = hw
    const = W.normal(f"golden/mgn/{tag}/constants", (batch, 1, kw["constant_channels"], h, w), 1.0)
    pc = kw.get("prescribed_channels", 0)
    presc = W.normal(f"golden/mgn/{tag}/prescribed", (batch, frames, pc, h, w), 1.0) if pc else None
    prog = W.normal(f"golden/mgn/{tag}/prognostic", (batch, frames, kw["prognostic_channels"], h, w), 1.0)
    return const, presc, prog


class _Graph:
    """dgl.DGLGraph stand-in: bookkeeping only (see the module docstring)"""

    def __init__(self, src, dst, n, batch_size=1):
        self.src, self.dst, self.n, self.batch_size = src.long(), dst.long(), int(n), batch_size
        self.ndata, self.edata = {}, {}

    srcdata = property(lambda self: self.ndata)
    dstdata = property(lambda self: self.ndata)

    def num_nodes(self):
        return self.n

    def num_edges(self):
        return int(self.src.numel())

    def edges(self):
        return self.src, self.dst

    def nodes(self):
        return torch.arange(self.n)

    def to(self, device=None, **k):
        return self

    def local_scope(self):
        g = self

        class _Scope:
            def __enter__(self):
                self.saved = (dict(g.ndata), dict(g.edata))

            def __exit__(self, *a):
                g.ndata, g.edata = self.saved

        return _Scope()

    def apply_edges(self, fn):
        edges = types.SimpleNamespace(data=self.edata, src={k: v[self.src] for k, v in self.ndata.items()},
                                      dst={k: v[self.dst] for k, v in self.ndata.items()})
        self.edata.update(fn(edges))

    def update_all(self, msg, red):
        assert msg[0] == "copy_e"
        m = self.edata[msg[1]]
        out = torch.zeros((self.n,) + m.shape[1:], dtype=m.dtype).index_add_(0, self.dst, m)
        if red[0] == "mean":
            deg = torch.bincount(self.dst, minlength=self.n).clamp(min=1).to(m.dtype)
            out = out / deg.view(-1, *([1] * (m.dim() - 1)))
        self.ndata[red[2]] = out


def _install_dgl():
    dgl = types.ModuleType("dgl")
    fn = types.ModuleType("dgl.function")
    fn.copy_e = lambda e, m: ("copy_e", e, m)
    fn.sum = lambda m, h: ("sum", m, h)
    fn.mean = lambda m, h: ("mean", m, h)

    def from_networkx(g):
        nodes = sorted(g.nodes())
        idx = {v: i for i, v in enumerate(nodes)}
        pairs = [(idx[a], idx[b]) for a, b in g.edges()]
        src = [a for a, b in pairs] + [b for a, b in pairs]
        dst = [b for a, b in pairs] + [a for a, b in pairs]
        return _Graph(torch.tensor(src), torch.tensor(dst), len(nodes))

    def to_bidirected(g):
        e = torch.unique(torch.stack([torch.cat([g.src, g.dst]), torch.cat([g.dst, g.src])], 1), dim=0)
        e = e[e[:, 0] != e[:, 1]]
        return _Graph(e[:, 0], e[:, 1], g.n)

    def batch(graphs):
        off = torch.arange(len(graphs)) * graphs[0].n
        ne = graphs[0].num_edges()
        return _Graph(torch.cat([g.src for g in graphs]) + off.repeat_interleave(ne),
                      torch.cat([g.dst for g in graphs]) + off.repeat_interleave(ne), graphs[0].n * len(graphs), len(graphs))

    dgl.DGLGraph, dgl.from_networkx, dgl.to_bidirected, dgl.batch, dgl.function = _Graph, from_networkx, to_bidirected, batch, fn
    dgl.graph = _Graph                           # a return annotation only (meshgraphnet.py:286)
    sys.modules["dgl"], sys.modules["dgl.function"] = dgl, fn
    for name in ("s3fs", "git"):
        sys.modules.setdefault(name, types.ModuleType(name))


def load_reference_mgn():
    ref_import.load_reference()
    _install_dgl()
    for sub in ("graphcast", "mgn"):             # namespaces: graphcast/__init__.py imports GraphCastNet
        name = f"models.{sub}"
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(ref_import.REF_PKG, "models", sub)]
        sys.modules[name] = m
    return importlib.import_module("models.mgn.meshgraphnet")


def build(mod, kw, hwp):
    h, w, periodic = hwp
    return mod.MeshGraphNet(**kw, device="cpu", graph=types.SimpleNamespace(height=h, width=w, periodic=periodic)).eval()


def stepwise_rollout(m, const, presc, prog, ctx):
    """the reference forward one step at a time (its own loop crashes on step 2), the trajectory rebuilt as the loop
    intends: window = input frames before ctx, then the outputs so far"""
    outs = []
    for s in range(prog.shape[1] - ctx):
        t = s + ctx
        frames = [prog[:, f] if f < ctx else outs[f - ctx] for f in range(s, t)]
        win = torch.stack(frames + [frames[-1]], dim=1)           # the extra frame is the one step `forward` predicts from
        y = m(constants=const, prescribed=presc[:, s:t + 1] if presc is not None else None, prognostic=win)
        outs.append(y[:, 0])
    return torch.stack(outs, dim=1)


def _save(name, **arrays):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def gen_rollouts(mod):
    for tag, (kw, hwp, batch, frames) in ROLLOUT_CASES.items():
        torch.manual_seed(0)
        m = build(mod, kw, hwp)
        sha = fill(m)
        const, presc, prog = case_inputs(tag, kw, batch, frames, hwp[:2])
        with torch.no_grad():
            y = stepwise_rollout(m, const, presc, prog, kw["context_size"])
        case = dict(kwargs=kw, graph=list(hwp), batch=batch, frames=frames)
        _save(f"mgn_rollout_{tag}", y=y.numpy(), sha=np.array(sha), case=np.array(json.dumps(case)),
              state_spec=np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()])))


def gen_grad(mod, case=GRAD_CASE, prefix="mgn_"):
    tag, kw, hwp, batch, frames = case
    torch.set_num_threads(1)         # threaded CPU reductions of the backward differ run to run in the last bits
    m = build(mod, kw, hwp)
    sha = fill(m)
    m.train()
    const, presc, prog = case_inputs(tag, kw, batch, frames, hwp[:2])
    y = stepwise_rollout(m, const, presc, prog, kw["context_size"])
    loss = torch.mean((y - prog[:, kw["context_size"]:]) ** 2)
    loss.backward()
    names, norms, projs = [], [], []
    for name, p in m.named_parameters():
        g = p.grad.detach().double()
        names.append(name)
        norms.append(float(g.norm()))
        projs.append(float((g * W.normal(f"golden/mgn/{tag}/probe/{name}", tuple(g.shape), 1.0).double()).sum()))
    case = dict(kwargs=kw, graph=list(hwp), batch=batch, frames=frames)
    _save(f"{prefix}{tag}", names=np.array(json.dumps(names)), norms=np.array(norms), projs=np.array(projs),
          loss=np.array(float(loss.detach())), sha=np.array(sha), case=np.array(json.dumps(case)))


def gen_graphs(mod):
    for gt, h, w in GRAPH_CASES:
        kw = dict(_small(graph_type=gt, input_dim_edges=3 if gt == "grid_2d_8stencil" else 2))
        m = build(mod, kw, (h, w, True))
        src, dst = (t.numpy() for t in m.graph.edges())
        order = np.lexsort((dst, src))
        _save(f"mgn_graph_{gt}_{h}x{w}", src=src[order].astype(np.int32), dst=dst[order].astype(np.int32),
              feats=m.edge_features.numpy()[order], n_nodes=np.array(m.graph.num_nodes()))


def main():
    if not ref_import.reference_available():
        raise SystemExit("reference tree not available: these fixtures can only be regenerated where it is")
    mod = load_reference_mgn()
    os.makedirs(GOLDEN, exist_ok=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    only = set(sys.argv[1:])
    if not only or "graphs" in only:
        gen_graphs(mod)
    if not only or "rollouts" in only:
        gen_rollouts(mod)
    if not only or "grad" in only:
        gen_grad(mod)
    if not only or "train" in only:
        for tag, (kw, hwp, batch, frames) in TRAIN_GRAD_CASES.items():
            gen_grad(mod, (tag, kw, hwp, batch, frames), prefix="mgn_train_")


if __name__ == "__main__":
    main()
