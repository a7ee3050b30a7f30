"""GraphCastNet training without a GPU: the gradient fixtures of the HIP training path load and are single-sample, the
training envelope, and CPU tensors train on the torch composition."""
import json

import pytest
import torch

from helpers import load_golden

TRAIN_CASES = ["train_yaml_l3_32x64", "train_mean_hl2_relu_l2_8x16", "train_ctx2_noconst_d40_l1_8x16",
               "train_d512_l1_8x16"]


@pytest.mark.parametrize("tag", TRAIN_CASES)
def test_training_fixtures_load_single_sample(tag):
    g = load_golden(f"graphcast_{tag}")
    case = json.loads(str(g["case"]))
    names = json.loads(str(g["names"]))
    assert len(names) == len(g["norms"]) == len(g["projs"]) and names
    assert case["frames"] - case["kwargs"]["context_size"] >= 1
    assert "batch" not in case["kwargs"]                  # B = 1: the reference raises for B > 1
    assert float(g["loss"]) > 0


def _small(**kw):
    from dlwp_benchmark_amd.models import GraphCastNet

    args = dict(input_height=8, input_width=16, constant_channels=2, prescribed_channels=1, prognostic_channels=3,
                processor_layers=3, hidden_dim=24)
    args.update(kw)
    return GraphCastNet("icospheres_l1.json", **args)


def test_training_envelope():
    m = _small()
    assert not m.uses_hip_training()                      # the composition by default
    assert m.set_hip_training(True).uses_hip_training()
    assert not _small(activation_fn="gelu").set_hip_training(True).uses_hip_training()
    assert not _small(hidden_dim=520).set_hip_training(True).uses_hip_training()
    assert not _small(norm_type=None).set_hip_training(True).uses_hip_training()
    assert not m.set_hip_step(False).uses_hip_training()


def test_cpu_tensors_train_on_the_composition():
    m = _small().set_hip_training(True).train()
    called = []
    orig = m._step_torch
    m._step_torch = lambda x: called.append(1) or orig(x)
    m._step_train = lambda x: pytest.fail("HIP training step on CPU tensors")
    x = torch.randn(1, m.input_dim_grid_nodes, 8, 16)
    y = m.one_step(x)
    y.sum().backward()
    assert called and y.shape == (1, 3, 8, 16)
