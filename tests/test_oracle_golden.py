"""Pins the oracle (CPU restatement) against fixtures made by the REAL reference
(oracle/make_golden.py, run where the reference is available).  CPU only."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import load_golden, rel_l2
from oracle.make_golden import PORTABLE_CPU_ENV, spectral_conv2d_case, tensor_sha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPECTRAL_CASES = {
    "c32_64x64_m12": (32, 32, 64, 64, 12, 12, 1),
    "c32_32x64_m8x6": (32, 32, 32, 64, 8, 6, 1),
    "c4_16x16_m4": (4, 4, 16, 16, 4, 4, 2),
}


@pytest.fixture(scope="module")
def spectral_portable(tmp_path_factory):
    """the restatement's output of every SPECTRAL_CASES entry, computed in a child interpreter with PORTABLE_CPU_ENV -- the
    environment the fixtures were made in, so that the bits do not depend on the CPU the suite runs on"""
    path = str(tmp_path_factory.mktemp("spectral") / "y.npz")
    code = ("import numpy as np; from oracle.make_golden import spectral_conv2d_case; "
            "from oracle.restate.fno import spectral_conv2d_ref; "
            f"cases = {SPECTRAL_CASES!r}; "
            f"np.savez({path!r}, **{{t: spectral_conv2d_ref(*spectral_conv2d_case(*c, t)).numpy() for t, c in cases.items()}})")
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], cwd=ROOT,
                       env=dict(os.environ, **PORTABLE_CPU_ENV), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("tag", list(SPECTRAL_CASES))
def test_spectral_conv2d_restatement_matches_reference(tag, spectral_portable):
    ci, co, h, w, m1, m2, b = SPECTRAL_CASES[tag]
    g = load_golden(f"spectral_conv2d_{tag}")
    x, w1, w2 = spectral_conv2d_case(ci, co, h, w, m1, m2, b, tag)
    assert tensor_sha(x, w1, w2) == str(g["sha"]), "filler drifted: regenerate fixtures"
    y = torch.from_numpy(spectral_portable[tag])
    # same torch build, same portable CPU arithmetic on both sides -> bit-identical
    assert torch.equal(y, torch.from_numpy(g["y"]))


# ------------------------------------------------------------------------------------------
# whole backbones: functional restatements vs trajectories produced by the real reference
# ------------------------------------------------------------------------------------------
import json

from dlwp_benchmark_amd.weights import fill_by_spec
from oracle.make_golden import MODEL_CASES, model_inputs
from oracle.restate import afno as R_afno
from oracle.restate import pangu as R_pangu
from oracle.restate import swin as R_swin
from oracle.restate import unet as R_unet

ROLLOUTS = {
    "swin": R_swin.swin_rollout,
    "afno": R_afno.afnonet_rollout,
    "pangu": R_pangu.pangu_rollout,
    "unet": R_unet.unet_rollout,
    "convlstm": R_unet.convlstm_rollout,
}


def oracle_case(tag):
    """(golden trajectory, oracle trajectory) for one MODEL_CASES entry."""
    family, cfg, (batch, frames), gain = MODEL_CASES[tag]
    g = load_golden(f"model_{tag}")
    spec = json.loads(str(g["param_spec"]))
    sd, sha = fill_by_spec(spec, gain=gain)
    assert sha == str(g["sha"]), "filler drifted: regenerate fixtures"
    constants, prescribed, prognostic = model_inputs(tag, cfg, batch, frames)
    with torch.no_grad():
        y = ROLLOUTS[family](sd, cfg, constants, prescribed, prognostic)
    return torch.from_numpy(g["y"]), y


@pytest.mark.parametrize("tag", list(MODEL_CASES))
def test_backbone_restatement_matches_reference(tag):
    want, got = oracle_case(tag)
    assert got.shape == want.shape
    # same torch build, same op sequence: expected bit-identical; allow last-ulp reassociation
    err = rel_l2(got, want)
    assert err < 1e-6, f"{tag}: rel L2 {err:.3e}"


# ------------------------------------------------------------------------------------------
# HEALPix (8f f3): face padding + HEALPix U-Net restatements vs the real reference
# ------------------------------------------------------------------------------------------
from dlwp_benchmark_amd import weights as W
from oracle.make_golden import (HPX_CONVLSTM_CASES, HPX_MODEL_CASES, HPX_MUNET_CASES, HPX_PAD_CASES, HPX_SWIN_CASES,
                                hpx_inputs)
from oracle.restate import healpix as R_hpx


@pytest.mark.parametrize("tag", list(HPX_PAD_CASES))
def test_healpix_padding_restatement_matches_reference(tag):
    b, c, h, w, p = HPX_PAD_CASES[tag]
    g = load_golden(f"healpix_pad_{tag}")
    x = W.normal(f"golden/hpxpad/{tag}/x", (b * 12, c, h, w), 1.0)
    assert tensor_sha(x) == str(g["sha"]), "filler drifted: regenerate fixtures"
    assert torch.equal(R_hpx.healpix_pad(x, p), torch.from_numpy(g["y"]))


@pytest.mark.parametrize("tag", list(HPX_MODEL_CASES))
def test_unet_hpx_restatement_matches_reference(tag):
    cfg, (batch, frames), hw = HPX_MODEL_CASES[tag]
    g = load_golden(f"model_{tag}")
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=1.0)
    assert sha == str(g["sha"]), "filler drifted: regenerate fixtures"
    constants, prescribed, prognostic = hpx_inputs(tag, cfg, batch, frames, hw)
    with torch.no_grad():
        y = R_hpx.unet_hpx_rollout(sd, cfg, constants, prescribed, prognostic)
    ref = torch.from_numpy(g["y"])
    assert y.shape == ref.shape
    assert max(rel_l2(y[:, t], ref[:, t]) for t in range(ref.shape[1])) < 1e-6


@pytest.mark.parametrize("tag", list(HPX_SWIN_CASES))
def test_swin_hpx_restatement_matches_reference(tag):
    cfg, (batch, frames), hw = HPX_SWIN_CASES[tag]
    g = load_golden(f"model_{tag}")
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=1.0)
    assert sha == str(g["sha"]), "filler drifted: regenerate fixtures"
    constants, prescribed, prognostic = hpx_inputs(tag, cfg, batch, frames, hw)
    with torch.no_grad():
        y = R_swin.swin_hpx_rollout(sd, cfg, constants, prescribed, prognostic)
    ref = torch.from_numpy(g["y"])
    assert y.shape == ref.shape
    assert max(rel_l2(y[:, t], ref[:, t]) for t in range(ref.shape[1])) < 1e-6


@pytest.mark.parametrize("tag", list(HPX_MUNET_CASES))
def test_munet_hpx_restatement_matches_reference(tag):
    """ResidualBlock / MiddleBlock / GroupNorm, pinned through the only ModernUNet the
    reference can run (MUNetHPX)."""
    cfg, (batch, frames), hw = HPX_MUNET_CASES[tag]
    g = load_golden(f"model_{tag}")
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=1.0)
    assert sha == str(g["sha"]), "filler drifted: regenerate fixtures"
    constants, prescribed, prognostic = hpx_inputs(tag, cfg, batch, frames, hw)
    with torch.no_grad():
        y = R_hpx.munet_hpx_rollout(sd, cfg, constants, prescribed, prognostic)
    ref = torch.from_numpy(g["y"])
    assert y.shape == ref.shape
    assert max(rel_l2(y[:, t], ref[:, t]) for t in range(ref.shape[1])) < 1e-6


@pytest.mark.parametrize("tag", list(HPX_CONVLSTM_CASES))
def test_convlstm_hpx_restatement_matches_reference(tag):
    """ConvLSTMHPX (convlstm.py:258-305) vs the trajectory of the real class."""
    cfg, (batch, frames), hw = HPX_CONVLSTM_CASES[tag]
    g = load_golden(f"model_{tag}")
    sd, sha = fill_by_spec(json.loads(str(g["param_spec"])), gain=1.0)
    assert sha == str(g["sha"]), "filler drifted: regenerate fixtures"
    constants, prescribed, prognostic = hpx_inputs(tag, cfg, batch, frames, hw)
    with torch.no_grad():
        y = R_hpx.convlstm_hpx_rollout(sd, cfg, constants, prescribed, prognostic)
    ref = torch.from_numpy(g["y"])
    assert y.shape == ref.shape
    assert max(rel_l2(y[:, t], ref[:, t]) for t in range(ref.shape[1])) < 1e-6


@pytest.mark.parametrize("tag", ["swin_c3_full_h12", "afno_c4_full_h20"])
def test_backbone_restatement_matches_reference_at_configured_horizon(tag):
    """C3 (12 steps) and C4 (20 steps) at full width: the restatement against the real classes' trajectory (C5's five
    steps take ~30 s of CPU and are covered on the GPU side only)."""
    from oracle.make_golden import HORIZON_CASES

    base, frames, stride = HORIZON_CASES[tag]
    family, cfg, (batch, _), gain = MODEL_CASES[base]
    g = load_golden(f"model_{tag}")
    spec = json.loads(str(load_golden(f"model_{base}")["param_spec"]))
    sd, sha = fill_by_spec(spec, gain=gain)
    assert sha == str(g["sha"]), "filler drifted: regenerate fixtures"
    constants, prescribed, prognostic = model_inputs(base, cfg, batch, frames)
    with torch.no_grad():
        y = ROLLOUTS[family](sd, cfg, constants, prescribed, prognostic)[..., ::stride, ::stride]
    want = torch.from_numpy(g["y"])
    assert y.shape == want.shape
    assert max(rel_l2(y[:, t], want[:, t]) for t in range(want.shape[1])) < 1e-6
