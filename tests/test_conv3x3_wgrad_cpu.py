"""The weight / bias gradient of the 3x3 convolutions without a GPU: the cases and fp64 references that
test_conv3x3_wgrad_gpu.py runs dlwp_conv3x3_wgrad_f32 against, the torch composition conv3x3_weight_grad_torch against the
same references, the DLWP_CONV_WGRAD switch and the C ABI table.

CASES: tag -> (B or faces, c0, c1, cout, H, W, pre_act, hpx, offset).  The smallest shapes at which each part of the kernel
(64 x 64 channel blocks as 2 x 2 waves of 32 x 32, 8 x 8 pixel tiles consumed two pixels per matrix instruction, K-slices of at
least 4 tiles) can go wrong:
  tiny         both channel axes almost entirely zero-fill, the map smaller than a tile, one slice
  odd_pixels   15 pixels: the last pixel pair is partial
  segments     two input segments split inside a channel block; odd cout; pre-activation at load
  tiles        a full and a partial 32-channel quarter on both axes
  ragged       H and W no multiples of the tile: the longitude wrap meets a partial tile, the zero latitude rows must stay
               zero under the pre-activation
  hpx_small    one sample, every face all border, the corner mean of ACTIVATED sources
  hpx_two      two samples (the table's sample base) and two segments
  multi_slice  five 1 x 1 maps of one channel: 5 tiles -> 2 slices of 4 and 1 tiles (asserted through
               dlwp_conv3x3_wgrad_slices on the GPU); on a 1-wide cylinder both longitude neighbours are the pixel itself
  offset_view  `segments` with x0, x1 and dz one float into their storage (4-byte-aligned pointers)"""
import functools

import pytest
import torch

from dlwp_benchmark_amd import healpix, lib, ops, training, weights
from dlwp_benchmark_amd.training import conv3x3_weight_grad_torch, conv_wgrad_mode, conv_wgrad_uses_hip  # noqa: F401 (the feature)

A = ops.ACTS
CASES = {
    "tiny": (1, 1, 0, 1, 4, 4, A["none"], False, False),
    "odd_pixels": (1, 2, 0, 3, 3, 5, A["none"], False, False),
    "segments": (2, 5, 3, 7, 8, 16, A["gelu"], False, False),
    "tiles": (1, 40, 0, 36, 8, 8, A["silu"], False, False),
    "ragged": (2, 4, 2, 4, 5, 20, A["relu"], False, False),
    "hpx_small": (12, 3, 0, 5, 4, 4, A["silu"], True, False),
    "hpx_two": (24, 6, 2, 4, 8, 8, A["gelu"], True, False),
    "multi_slice": (5, 1, 0, 1, 1, 1, A["none"], False, False),
    "offset_view": (2, 5, 3, 7, 8, 16, A["gelu"], False, True),
}


def make_inputs(tag, integer=False):
    """(x0, x1 or None, dz) of a case on the CPU, fp32, seeded by the tag; integer: whole numbers in [-3, 3]"""
    b, c0, c1, cout, h, w = CASES[tag][:6]

    def draw(name, shape):
        t = weights.normal(f"conv3x3_wgrad/{tag}/{name}", shape)
        return (1.5 * t).round().clamp(-3, 3) if integer else t

    x0 = draw("x0", (b, c0, h, w))
    x1 = draw("x1", (b, c1, h, w)) if c1 else None
    return x0, x1, draw("dz", (b, cout, h, w))


@functools.lru_cache(maxsize=None)
def inputs(tag):
    return make_inputs(tag)


def reference_of(x0, x1, dz, pre_act, hpx):
    """(dW, db) in fp64: autograd of training.conv3x3_torch with respect to weight and bias, output gradient dz"""
    d = lambda t: t.double() if t is not None else None
    cin = x0.shape[1] + (x1.shape[1] if x1 is not None else 0)
    wgt = torch.zeros(dz.shape[1], cin, 3, 3, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(dz.shape[1], dtype=torch.float64, requires_grad=True)
    table = healpix.device_table(x0.shape[2], x0.shape[3], 1, "cpu") if hpx else None
    y = training.conv3x3_torch(d(x0), d(x1), wgt, bias, None, pre_act, 0, table)
    dw, db = torch.autograd.grad(y, (wgt, bias), d(dz))
    return dw, db


@functools.lru_cache(maxsize=None)
def reference(tag, pre_act=None):
    """the fp64 (dW, db) of a case (pre_act: instead of the case's); computed once, not to be modified"""
    x0, x1, dz = inputs(tag)
    return reference_of(x0, x1, dz, CASES[tag][6] if pre_act is None else pre_act, CASES[tag][7])


def deviation(got, want):
    return float((got.detach().double().cpu() - want).norm() / want.norm())


@pytest.mark.parametrize("tag", ["segments", "hpx_two"])
@pytest.mark.parametrize("act", sorted(ops.ACTS.values()))
def test_torch_composition_matches_fp64_autograd(tag, act):
    x0, x1, dz = inputs(tag)
    hpx = CASES[tag][7]
    table = healpix.device_table(x0.shape[2], x0.shape[3], 1, "cpu") if hpx else None
    dw, db = training.conv3x3_weight_grad_torch(x0, x1, dz, act, table)
    want_w, want_b = reference(tag, act)
    assert dw.dtype == torch.float32 and dw.shape == want_w.shape and db.shape == want_b.shape
    print(tag, act, "dW %.2e db %.2e" % (deviation(dw, want_w), deviation(db, want_b)))
    assert deviation(dw, want_w) <= 1e-5 and deviation(db, want_b) <= 1e-5


@pytest.mark.parametrize("tag", [t for t in CASES if t not in ("segments", "hpx_two", "offset_view")])
def test_torch_composition_matches_on_every_case(tag):
    x0, x1, dz = inputs(tag)
    pre_act, hpx = CASES[tag][6:8]
    table = healpix.device_table(x0.shape[2], x0.shape[3], 1, "cpu") if hpx else None
    dw, db = training.conv3x3_weight_grad_torch(x0, x1, dz, pre_act, table)
    want_w, want_b = reference(tag)
    assert deviation(dw, want_w) <= 1e-5 and deviation(db, want_b) <= 1e-5


def test_torch_composition_honours_the_need_flags():
    x0, x1, dz = inputs("segments")
    dw, db = training.conv3x3_weight_grad_torch(x0, x1, dz, 0, None, need_bias=False)
    assert db is None and dw is not None
    dw, db = training.conv3x3_weight_grad_torch(x0, x1, dz, 0, None, need_weight=False)
    assert dw is None and db is not None


def test_integer_inputs_are_exact_in_fp32():
    """what the GPU mapping check relies on: whole numbers in [-3, 3], every partial sum far below 2^24"""
    for tag in ("segments", "tiles", "hpx_two"):
        x0, x1, dz = make_inputs(tag, integer=True)
        for t in (x0, x1, dz):
            if t is not None:
                assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3 and len(t.unique()) == 7
        pixels = dz.shape[0] * dz.shape[2] * dz.shape[3]
        assert 9 * pixels < 2 ** 24
        dw, _ = reference_of(x0, x1, dz, 0, CASES[tag][7])
        assert torch.equal(dw * 2, (dw * 2).round())          # HEALPix corner means are half-integers at worst
        assert float(dw.abs().max()) > 0


def test_conv_wgrad_mode_parses(monkeypatch):
    monkeypatch.delenv("DLWP_CONV_WGRAD", raising=False)
    assert training.conv_wgrad_mode() == "auto"
    for mode in ("auto", "hip", "torch"):
        monkeypatch.setenv("DLWP_CONV_WGRAD", mode)
        assert training.conv_wgrad_mode() == mode
    monkeypatch.setenv("DLWP_CONV_WGRAD", "miopen")
    with pytest.raises(lib.DlwpError):
        training.conv_wgrad_mode()
    monkeypatch.setenv("DLWP_CONV_WGRAD", "torch")
    assert not training.conv_wgrad_uses_hip(2, 64, 0, 64, 8, 16, False)     # decided without touching the library


def test_c_abi_table_has_the_entries():
    for name in ("dlwp_conv3x3_wgrad_workspace_bytes", "dlwp_conv3x3_wgrad_slices", "dlwp_conv3x3_wgrad_f32"):
        assert name in lib.SIGNATURES
    assert len(lib.SIGNATURES["dlwp_conv3x3_wgrad_f32"][1]) == 16
