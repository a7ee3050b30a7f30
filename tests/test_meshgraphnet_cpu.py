"""MeshGraphNet (reference models/mgn/meshgraphnet.py) without a GPU: registry and config construction, the state-dict
layout, and the host-built graphs against what the REAL reference class built (tests/golden/mgn_*.npz, written by
tools/make_golden_meshgraphnet.py)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUTS = ["yaml_delaunay_32x64", "grid_mean_mp2_16x16", "stencil8_16x32", "default_widths_delaunay_8x16",
            "d470_delaunay_8x16", "ctx2_prescribed_grid_8x16", "grid_nonperiodic_8x16"]
GRAPHS = [(t, h, w) for t in ("grid_2d", "grid_2d_8stencil", "delaunay") for h, w in ((32, 64), (16, 32))]


def _build(g):
    from dlwp_benchmark_amd.models import MeshGraphNet

    case = json.loads(str(g["case"]))
    h, w, periodic = case["graph"]
    return MeshGraphNet(**case["kwargs"], device="cpu", graph=dict(height=h, width=w, periodic=periodic)), case


def test_shim_exports_meshgraphnet():
    shim = os.path.join(ROOT, "shim")
    old = sys.modules.pop("models", None)
    sys.path.insert(0, shim)
    try:
        ns = {}
        exec("from models import *", ns)
    finally:
        sys.path.remove(shim)
        sys.modules.pop("models", None)
        if old is not None:
            sys.modules["models"] = old
    assert issubclass(ns["MeshGraphNet"], torch.nn.Module)


def test_yaml_config_constructs():
    from dlwp_benchmark_amd.models import MeshGraphNet

    with open(os.path.join(ROOT, "tests", "golden", "model_configs.json")) as f:
        cfg = json.load(f)["meshgraphnet.yaml"]
    interp = {"${data.height}": 32, "${data.width}": 64, "${device}": "cpu"}
    cfg = {k: interp.get(v, v) if isinstance(v, str) else v for k, v in cfg.items()}
    cfg["graph"] = {k: interp.get(v, v) if isinstance(v, str) else v for k, v in cfg["graph"].items()}
    assert cfg["type"] == "MeshGraphNet"
    m = MeshGraphNet(**cfg)
    assert (m.n_nodes, m.n_edges) == (2048, 12032)
    assert sum(p.numel() for p in m.parameters()) == 50452
    assert len(m.state_dict()) == 87
    # an attribute object (Hydra's DictConfig) works as well as a mapping
    cfg["graph"] = types.SimpleNamespace(**cfg["graph"])
    assert MeshGraphNet(**cfg).n_edges == 12032


@pytest.mark.parametrize("tag", ROLLOUTS)
def test_state_dict_matches_reference(tag):
    g = load_golden(f"mgn_rollout_{tag}")
    m, _ = _build(g)
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    assert got == json.loads(str(g["state_spec"]))              # keys, shapes AND order, device_buffer included
    sd = {k: torch.randn(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.node_encoder.model[0].weight, sd["node_encoder.model.0.weight"])


@pytest.mark.parametrize("gt,h,w", GRAPHS)
def test_graph_matches_reference(gt, h, w):
    from dlwp_benchmark_amd.models.mgn import reference_graph

    g = load_golden(f"mgn_graph_{gt}_{h}x{w}")
    n, src, dst, feats = reference_graph(gt, h, w, True)
    assert n == int(g["n_nodes"])
    np.testing.assert_array_equal(src, g["src"])
    np.testing.assert_array_equal(dst, g["dst"])
    np.testing.assert_array_equal(feats, g["feats"])           # bit-exact, the reference's quirks included


def test_graph_buffers_are_csc_and_not_persistent():
    from dlwp_benchmark_amd.models import MeshGraphNet

    m = MeshGraphNet(graph_type="grid_2d", graph=dict(height=8, width=16, periodic=[False, True]), processor_size=1)
    rp, src, dst = m.graph_row_ptr.long(), m.graph_src.long(), m.graph_dst.long()
    assert rp[0] == 0 and rp[-1] == src.numel() and torch.all(rp[1:] >= rp[:-1])
    for n in range(m.n_nodes):
        assert torch.all(dst[rp[n]:rp[n + 1]] == n)
    assert not any(k.startswith("graph_") for k in m.state_dict())


class _ListConfigLike:
    """a non-list sequence, like Hydra's ListConfig"""

    def __init__(self, *v):
        self.v = list(v)

    def __len__(self):
        return len(self.v)

    def __getitem__(self, i):
        return self.v[i]

    def __bool__(self):
        return True


def test_periodic_accepts_any_sequence():
    from dlwp_benchmark_amd.models import MeshGraphNet

    kw = dict(graph_type="grid_2d", processor_size=1)
    a = MeshGraphNet(**kw, graph=dict(height=8, width=16, periodic=_ListConfigLike(False, True)))
    b = MeshGraphNet(**kw, graph=dict(height=8, width=16, periodic=(False, True)))
    c = MeshGraphNet(**kw, graph=dict(height=8, width=16, periodic=True))
    assert torch.equal(a.graph_src, b.graph_src) and torch.equal(a.graph_dst, b.graph_dst)
    assert a.n_edges < c.n_edges                 # rows not wrapped


def test_do_concat_trick_raises():
    from dlwp_benchmark_amd.models import MeshGraphNet

    with pytest.raises(NotImplementedError):
        MeshGraphNet(do_concat_trick=True, graph=dict(height=8, width=16, periodic=True))


def test_edge_width_mismatch_raises():
    from dlwp_benchmark_amd.models import MeshGraphNet

    with pytest.raises(ValueError):      # the 8-stencil's edge features are 3 wide; the reference crashes later with 2
        MeshGraphNet(graph_type="grid_2d_8stencil", input_dim_edges=2, graph=dict(height=8, width=16, periodic=True))
