"""GraphCastNet on the CPU: the icosphere generator, the three graphs and their features against the real reference's
construction (tests/golden/graphcast_graph_*.npz), the state-dict layout, construction from graphcast.yaml through the shim,
the torch composition against the rollout and gradient fixtures, and the flags that raise."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden, per_step_rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_graphcast as t
    finally:
        sys.path.pop(0)
    return t


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_icosphere_counts_norms_nesting_centroids(level):
    from dlwp_benchmark_amd import icosphere as I

    ico = I.icospheres(level)
    assert I.max_order(ico) == level
    for k in range(level + 1):
        v, f = ico[f"order_{k}_vertices"], ico[f"order_{k}_faces"]
        assert len(v) == [12, 42, 162, 642][k] and len(f) == 20 * 4 ** k
        assert np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-12)
        assert np.allclose(ico[f"order_{k}_face_centroid"], v[f].mean(axis=1))
        if k:
            prev = ico[f"order_{k - 1}_vertices"]
            assert np.array_equal(v[:len(prev)], prev)
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert (np.einsum("ij,ij->i", n, v[f].mean(1)) > 0).all()            # consistently outward


def test_icosphere_cli_writes_the_reference_schema(tmp_path):
    from dlwp_benchmark_amd import icosphere as I

    out = tmp_path / "icospheres_l2.json"
    I.main(["--level", "2", "--out", str(out)])
    d = json.loads(out.read_text())
    assert d["vertices"] == [] and d["faces"] == []
    assert len([k for k in d if "faces" in k]) - 2 == 2                      # Graph.max_order (utils/graph.py:79-81)
    assert np.array_equal(I.load(str(out))["order_2_faces"], I.icospheres(2)["order_2_faces"])


@pytest.mark.parametrize("h,w,level", [(16, 32, 2), (32, 64, 3)])
def test_graphs_match_reference_construction(h, w, level):
    from dlwp_benchmark_amd import icosphere as I

    g = load_golden(f"graphcast_graph_l{level}_{h}x{w}")
    ico = I.icospheres(level)
    assert hashlib.sha256(I.to_json(ico).encode()).hexdigest() == str(g["mesh_sha"])
    got = I.graphcast_graphs(ico, h, w)
    for name in ("mesh", "g2m", "m2g"):
        src, dst, feats = got[name]
        assert np.array_equal(src, g[f"{name}_src"]) and np.array_equal(dst, g[f"{name}_dst"]), name
        assert np.abs(feats.numpy() - g[f"{name}_feats"]).max() <= 1e-7, name
    assert np.abs(got["mesh_nodes"].numpy() - g["mesh_nodes"]).max() <= 1e-7


def test_state_dict_layout_matches_reference():
    from dlwp_benchmark_amd.models import GraphCastNet

    for tag in ("yaml_l3_32x64", "mean_hl2_relu_l2_8x16"):
        g = load_golden(f"graphcast_rollout_{tag}")
        case = json.loads(str(g["case"]))
        m = GraphCastNet(f"icospheres_l{case['level']}.json", **case["kwargs"])
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == json.loads(str(g["state_spec"]))


def test_yaml_constructs_through_the_shim():
    yaml = pytest.importorskip("yaml")
    sys.path.insert(0, os.path.join(ROOT, "shim"))
    try:
        import models as shim_models
    finally:
        sys.path.pop(0)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "graphcast_yaml.yaml")))
    cls = getattr(shim_models, cfg["type"])
    m = cls(**cfg)
    assert type(m).__name__ == "GraphCastNet" and m.n_mesh == 642 and m.n_grid == 32 * 64


@pytest.mark.parametrize("tag", ["mean_hl2_relu_l2_8x16", "ctx2_noconst_d40_l1_8x16", "d512_l1_8x16"])
def test_torch_composition_matches_rollout_golden(tag):
    from dlwp_benchmark_amd.models import GraphCastNet
    from dlwp_benchmark_amd.rollout import rollout_train

    tool = _tool()
    g = load_golden(f"graphcast_rollout_{tag}")
    case = json.loads(str(g["case"]))
    m = GraphCastNet(f"icospheres_l{case['level']}.json", **case["kwargs"]).eval()
    assert tool.mgn_golden.fill(m) == str(g["sha"])
    c, p, q = tool.case_inputs(tag, case["kwargs"], case["frames"])
    with torch.no_grad():
        y = rollout_train(m._step_torch, case["kwargs"]["context_size"], c, p, q)
    assert max(per_step_rel_l2(y, torch.from_numpy(g["y"]))) <= 1e-5


def test_torch_composition_gradient_matches_golden():
    from dlwp_benchmark_amd.models import GraphCastNet
    from dlwp_benchmark_amd.rollout import rollout_train

    tool = _tool()
    g = load_golden("graphcast_grad_l1_8x16")
    case = json.loads(str(g["case"]))
    m = GraphCastNet(f"icospheres_l{case['level']}.json", **case["kwargs"]).train()
    assert tool.mgn_golden.fill(m) == str(g["sha"])
    c, p, q = tool.case_inputs("grad_l1_8x16", case["kwargs"], case["frames"])
    y = rollout_train(m._step_torch, case["kwargs"]["context_size"], c, p, q)
    loss = torch.mean((y - q[:, 1:]) ** 2)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) <= 1e-5 * abs(float(g["loss"]))
    params = dict(m.named_parameters())
    for name, norm, proj in zip(json.loads(str(g["names"])), g["norms"], g["projs"]):
        grad = params[name].grad.double()
        assert abs(float(grad.norm()) - norm) <= 1e-4 * norm + 1e-9, name
        probe = tool.W.normal(f"golden/graphcast/grad_l1_8x16/probe/{name}", tuple(grad.shape), 1.0).double()
        # direction: |<g - g_ref, probe>| <= |g - g_ref| |probe|, with |g - g_ref| <= 1e-4 |g_ref|
        assert abs(float((grad * probe).sum()) - proj) <= 1e-4 * norm * float(probe.norm()) + 1e-9, name


@pytest.mark.parametrize("kw,exc", [(dict(processor_layers=2), ValueError), (dict(do_concat_trick=True), NotImplementedError),
                                    (dict(use_cugraphops_processor=True), NotImplementedError),
                                    (dict(partition_size=2), NotImplementedError)])
def test_unsupported_flags_raise(kw, exc):
    from dlwp_benchmark_amd.models import GraphCastNet

    with pytest.raises(exc):
        GraphCastNet("icospheres_l1.json", input_height=8, input_width=16, hidden_dim=16, **kw)


def test_mesh_level_from_path_suffix():
    from dlwp_benchmark_amd.models import GraphCastNet

    m = GraphCastNet("nowhere/icospheres_l2.json", input_height=8, input_width=16, hidden_dim=16, processor_layers=3)
    assert m.n_mesh == 162
