"""Writes tests/golden/graphcast_*.npz: GraphCastNet rollouts, a gradient case and graphs from the REAL reference class
(models/graphcast/graph_cast_net.py) on the CPU, imported through oracle.ref_import, with the filler weights of
dlwp_benchmark_amd.weights.  The mesh file each case reads is written by dlwp_benchmark_amd.icosphere into a temporary
directory; every fixture carries the SHA-256 of that JSON text and the weight SHA.

dgl is not installed here, so this tool carries a stand-in: the one of tools/make_golden_meshgraphnet.py (graph
bookkeeping, to_bidirected as the simple symmetric graph sorted by (src, dst), apply_edges running the reference's own
concat_message_function, update_all(copy_e, sum | mean) as an index_add) plus `heterograph` with separate source and
destination node data, sized by the position tables the reference attaches.  DGL's exact semantics are an ASSUMPTION of
these fixtures.

The reference's in-model rollout crashes on its second step (graph_cast_net.py:640-643), so trajectories are driven one
step at a time, and the reference raises for B != 1, so every case is B = 1.

Runs where the reference tree is available:  python tools/make_golden_graphcast.py [graphs] [rollouts] [grad] [train]"""
import hashlib
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dlwp_benchmark_amd import icosphere  # noqa: E402
from dlwp_benchmark_amd import weights as W  # noqa: E402
from oracle import ref_import  # noqa: E402
import make_golden_meshgraphnet as mgn_golden  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

YAML = dict(input_height=32, input_width=64, constant_channels=4, prescribed_channels=1, prognostic_channels=8,
            input_dim_mesh_nodes=3, input_dim_edges=4, processor_layers=16, hidden_layers=1, hidden_dim=512,
            aggregation="sum", activation_fn="silu", norm_type="LayerNorm", context_size=1)


def _small(**kw):
    base = dict(YAML, input_height=8, input_width=16, constant_channels=2, prescribed_channels=1, prognostic_channels=3,
                processor_layers=3, hidden_dim=32)
    base.update(kw)
    return base


# tag -> (ctor kwargs, mesh level, frames)
ROLLOUT_CASES = {
    "yaml_l3_32x64": (YAML, 3, 3),
    "mean_hl2_relu_l2_8x16": (_small(aggregation="mean", hidden_layers=2, activation_fn="relu", hidden_dim=48), 2, 3),
    "ctx2_noconst_d40_l1_8x16": (_small(context_size=2, constant_channels=0, prescribed_channels=2, hidden_dim=40), 1, 4),
    "d512_l1_8x16": (_small(hidden_dim=512, processor_layers=4), 1, 2),
}
GRAD_CASE = ("grad_l1_8x16", _small(hidden_dim=24), 1, 3)
# more gradient cases (tests/golden/graphcast_train_<tag>.npz; B = 1: the reference raises for B > 1): the rollout cases'
# models, through their multi-step training rollouts
TRAIN_GRAD_CASES = [(f"train_{tag}", kw, level, frames) for tag, (kw, level, frames) in ROLLOUT_CASES.items()]
GRAPH_CASES = [(16, 32, 2), (32, 64, 3)]


class _Graph(mgn_golden._Graph):
    """homogeneous graph; `heterograph` below separates source and destination data"""

    def update_all(self, msg, red):
        assert msg[0] == "copy_e"
        m = self.edata[msg[1]]
        n = self._n_dst()
        out = torch.zeros((n,) + m.shape[1:], dtype=m.dtype).index_add_(0, self.dst, m)
        if red[0] == "mean":
            deg = torch.bincount(self.dst, minlength=n).clamp(min=1).to(m.dtype)
            out = out / deg.view(-1, *([1] * (m.dim() - 1)))
        self.dstdata[red[2]] = out

    def _n_dst(self):
        return self.n


class _HeteroGraph(_Graph):
    def __init__(self, src, dst, types_):
        super().__init__(torch.as_tensor(src), torch.as_tensor(dst), 0)
        self.types = types_
        self._src, self._dst = {}, {}

    srcdata = property(lambda self: self._src)
    dstdata = property(lambda self: self._dst)

    @property
    def ndata(self):
        return {k: {self.types[0]: self._src.get(k), self.types[2]: self._dst.get(k)} for k in set(self._src) | set(self._dst)}

    @ndata.setter
    def ndata(self, v):
        pass

    def _n_dst(self):
        return int(self._dst["pos"].shape[0])

    def local_scope(self):
        g = self

        class _Scope:
            def __enter__(self):
                self.saved = (dict(g._src), dict(g._dst), dict(g.edata))

            def __exit__(self, *a):
                g._src, g._dst, g.edata = self.saved

        return _Scope()

    def apply_edges(self, fn):
        edges = types.SimpleNamespace(data=self.edata, src={k: v[self.src] for k, v in self._src.items()},
                                      dst={k: v[self.dst] for k, v in self._dst.items()})
        self.edata.update(fn(edges))


def load_reference_graphcast():
    ref_import.load_reference()
    mgn_golden._install_dgl()
    dgl = sys.modules["dgl"]

    def graph(data, idtype=None):
        src, dst = (torch.as_tensor(np.asarray(t)).long() for t in data)
        return _Graph(src, dst, int(max(src.max(), dst.max())) + 1)

    def to_bidirected(g):
        e = torch.unique(torch.stack([torch.cat([g.src, g.dst]), torch.cat([g.dst, g.src])], 1), dim=0)
        e = e[e[:, 0] != e[:, 1]]
        return _Graph(e[:, 0], e[:, 1], g.n)

    def heterograph(spec, idtype=None):
        (labels, (_, (src, dst))), = spec.items()
        return _HeteroGraph(np.asarray(src), np.asarray(dst), labels)

    dgl.graph, dgl.to_bidirected, dgl.heterograph = graph, to_bidirected, heterograph
    name = "models.graphcast"
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(ref_import.REF_PKG, "models", "graphcast")]
    sys.modules[name] = m
    return importlib.import_module("models.graphcast.graph_cast_net")


def mesh_file(tmp, level):
    text = icosphere.to_json(icosphere.icospheres(level))
    path = os.path.join(tmp, f"icospheres_l{level}.json")
    with open(path, "w") as fh:
        fh.write(text)
    return path, hashlib.sha256(text.encode()).hexdigest()


def case_inputs(tag, kw, frames):
    h, w = kw["input_height"], kw["input_width"]
    cc, pc = kw["constant_channels"], kw["prescribed_channels"]
    const = W.normal(f"golden/graphcast/{tag}/constants", (1, 1, cc, h, w), 1.0) if cc else None
    presc = W.normal(f"golden/graphcast/{tag}/prescribed", (1, frames, pc, h, w), 1.0) if pc else None
    prog = W.normal(f"golden/graphcast/{tag}/prognostic", (1, frames, kw["prognostic_channels"], h, w), 1.0)
    return const, presc, prog


def stepwise_rollout(m, const, presc, prog, ctx):
    outs = []
    for s in range(prog.shape[1] - ctx):
        t = s + ctx
        frames = [prog[:, f] if f < ctx else outs[f - ctx] for f in range(s, t)]
        win = torch.stack(frames + [frames[-1]], dim=1)
        y = m(constants=const, prescribed=presc[:, s:t + 1] if presc is not None else None, prognostic=win)
        outs.append(y[:, 0])
    return torch.stack(outs, dim=1)


def gen_graphs(mod, tmp):
    for h, w, level in GRAPH_CASES:
        path, mesh_sha = mesh_file(tmp, level)
        m = mod.GraphCastNet(path, **_small(input_height=h, input_width=w))
        arrays = {}
        for name, g in (("mesh", m.mesh_graph), ("g2m", m.g2m_graph), ("m2g", m.m2g_graph)):
            arrays[f"{name}_src"] = g.src.numpy().astype(np.int32)
            arrays[f"{name}_dst"] = g.dst.numpy().astype(np.int32)
            arrays[f"{name}_feats"] = g.edata["x"].numpy()
        arrays["mesh_nodes"] = m.mesh_ndata.numpy()
        mgn_golden._save(f"graphcast_graph_l{level}_{h}x{w}", mesh_sha=np.array(mesh_sha), **arrays)


def gen_rollouts(mod, tmp):
    for tag, (kw, level, frames) in ROLLOUT_CASES.items():
        path, mesh_sha = mesh_file(tmp, level)
        torch.manual_seed(0)
        m = mod.GraphCastNet(path, **kw).eval()
        sha = mgn_golden.fill(m)
        const, presc, prog = case_inputs(tag, kw, frames)
        with torch.no_grad():
            y = stepwise_rollout(m, const, presc, prog, kw["context_size"])
        case = dict(kwargs=kw, level=level, frames=frames)
        mgn_golden._save(f"graphcast_rollout_{tag}", y=y.numpy(), sha=np.array(sha), mesh_sha=np.array(mesh_sha),
                         case=np.array(json.dumps(case)),
                         state_spec=np.array(json.dumps([[k, list(v.shape)] for k, v in m.state_dict().items()])))


def gen_grad(mod, tmp, case=GRAD_CASE):
    tag, kw, level, frames = case
    if case is GRAD_CASE:
        torch.set_num_threads(1)
    path, mesh_sha = mesh_file(tmp, level)
    m = mod.GraphCastNet(path, **kw)
    sha = mgn_golden.fill(m)
    m.train()
    const, presc, prog = case_inputs(tag, kw, frames)
    y = stepwise_rollout(m, const, presc, prog, kw["context_size"])
    loss = torch.mean((y - prog[:, kw["context_size"]:]) ** 2)
    loss.backward()
    names, norms, projs = [], [], []
    for name, p in m.named_parameters():
        g = p.grad.detach().double()
        names.append(name)
        norms.append(float(g.norm()))
        projs.append(float((g * W.normal(f"golden/graphcast/{tag}/probe/{name}", tuple(g.shape), 1.0).double()).sum()))
    case = dict(kwargs=kw, level=level, frames=frames)
    mgn_golden._save(f"graphcast_{tag}", names=np.array(json.dumps(names)), norms=np.array(norms), projs=np.array(projs),
                     loss=np.array(float(loss.detach())), sha=np.array(sha), mesh_sha=np.array(mesh_sha),
                     case=np.array(json.dumps(case)))


def main():
    if not ref_import.reference_available():
        raise SystemExit("reference tree not available: these fixtures can only be regenerated where it is")
    mod = load_reference_graphcast()
    os.makedirs(GOLDEN, exist_ok=True)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    only = set(sys.argv[1:])
    with tempfile.TemporaryDirectory() as tmp:
        if not only or "graphs" in only:
            gen_graphs(mod, tmp)
        if not only or "rollouts" in only:
            gen_rollouts(mod, tmp)
        if not only or "grad" in only:
            gen_grad(mod, tmp)
        if not only or "train" in only:
            for case in TRAIN_GRAD_CASES:
                gen_grad(mod, tmp, case)


if __name__ == "__main__":
    main()
