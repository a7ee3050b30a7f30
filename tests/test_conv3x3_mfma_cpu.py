"""Host side of the matrix-pipe 3x3 convolution forms: every module of the U-Net / ConvLSTM / diffusion families that calls
ops.conv3x3* carries `conv_form`, `compute_precision` (constructor kwarg and setter) and set_conv_form reach it, models
without such modules are untouched, and the C ABI of csrc/conv_mfma.hip is in the ctypes table."""
import pytest
from torch import nn

import dlwp_benchmark_amd.models as M
from dlwp_benchmark_amd import lib as L
from dlwp_benchmark_amd.models import diffusion as D
from dlwp_benchmark_amd.models import unet as U

UNET = dict(constant_channels=2, prescribed_channels=1, prognostic_channels=2, hidden_channels=[4, 8], n_convolutions=2)
CLSTM = dict(constant_channels=2, prescribed_channels=1, prognostic_channels=2, hidden_sizes=[4, 4], height=8, width=16)
MUNET = dict(constant_channels=1, prescribed_channels=1, prognostic_channels=2, hidden_channels=[4, 8], norm=True)
DIFF = dict(constant_channels=1, prescribed_channels=1, prognostic_channels=2, hidden_channels=[8, 16], norm=True,
            num_refinement_step=2)
FAMILIES = [("UNet", UNET), ("ConvLSTM", CLSTM), ("MUNetHPX", MUNET), ("DiffMUNetHPX", DIFF)]
# the module classes whose forward calls ops.conv3x3* (directly or through _run_stack)
CONV_BEARING = (U.HEALPixLayer, U.ResidualBlock, U._UNetEncoder, U._UNetDecoder, U._ConvLSTMCell, U.ConvLSTM, D.ResidualBlock)
EXPECT = {"fp32": "direct", "f16x3": "bf16x6", "bf16attn": "direct", "bf16": "bf16"}


def _forms(model):
    bearing = [m for m in model.modules() if isinstance(m, CONV_BEARING)]
    assert bearing, "no conv-bearing module found"
    for m in bearing:
        assert "conv_form" in m.__dict__, type(m).__name__
    # nothing else carries the attribute
    assert {id(m) for m in model.modules() if "conv_form" in m.__dict__} == {id(m) for m in bearing}
    return {m.conv_form for m in bearing}


@pytest.mark.parametrize("name,cfg", FAMILIES)
def test_conv_form_defaults_to_direct(name, cfg):
    model = getattr(M, name)(**cfg)
    assert _forms(model) == {"direct"}
    assert model.compute_precision == "fp32"


@pytest.mark.parametrize("name,cfg", FAMILIES)
@pytest.mark.parametrize("precision", list(EXPECT))
def test_compute_precision_kwarg_selects_the_conv_form(name, cfg, precision):
    model = getattr(M, name)(**cfg, compute_precision=precision)
    assert _forms(model) == {EXPECT[precision]}
    assert model.compute_precision == precision
    # and the setter, from any state, back and forth
    model.set_compute_precision("fp32")
    assert _forms(model) == {"direct"}
    model.set_compute_precision(precision)
    assert _forms(model) == {EXPECT[precision]}


@pytest.mark.parametrize("name,cfg", FAMILIES)
def test_set_conv_form(name, cfg):
    model = getattr(M, name)(**cfg)
    for form in ("bf16x6", "bf16", "direct"):
        assert model.set_conv_form(form) is model
        assert _forms(model) == {form}
    with pytest.raises(L.DlwpError, match="nope"):
        model.set_conv_form("nope")
    assert _forms(model) == {"direct"}
    with pytest.raises(L.DlwpError):
        getattr(M, name)(**cfg, compute_precision="nope")


def test_hpx_subclasses_pass_the_kwarg_on():
    assert _forms(M.UNetHPX(**UNET, compute_precision="bf16")) == {"bf16"}
    assert _forms(M.ConvLSTMHPX(**CLSTM, compute_precision="f16x3")) == {"bf16x6"}
    assert _forms(M.ModernUNet(**MUNET, compute_precision="bf16")) == {"bf16"}
    assert _forms(M.DiffModernUNet(**DIFF, compute_precision="bf16")) == {"bf16"}


def test_set_conv_form_drops_a_captured_step():
    model = M.UNet(**UNET)
    model._graphed = ("key", object())
    model.set_conv_form("bf16x6")
    assert model._graphed is None


def test_models_without_3x3_convolutions_are_untouched():
    model = M.SwinTransformer(constant_channels=1, prescribed_channels=0, prognostic_channels=1, context_size=1, img_height=8,
                              img_width=16, patch_size=2, embed_dim=8, depths=[2], num_heads=[2], window_size=2)
    assert not [m for m in model.modules() if hasattr(m, "conv_form")]
    before = {id(m): dict(m.__dict__) for m in model.modules()}
    model.set_conv_form("bf16")
    assert not [m for m in model.modules() if hasattr(m, "conv_form")]
    for m in model.modules():
        assert {k: v for k, v in m.__dict__.items() if k != "_graphed"} == \
            {k: v for k, v in before[id(m)].items() if k != "_graphed"}


def test_conv_entries_of_compute_precisions():
    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd.models._base import HipBackbone

    assert ops.CONV_FORMS == ("direct", "bf16x6", "bf16")
    assert {k: v[3] for k, v in HipBackbone.COMPUTE_PRECISIONS.items()} == EXPECT


def test_diffusion_has_no_step_graph():
    model = M.DiffMUNetHPX(**DIFF)
    assert model.set_step_graphs(False) is model
    with pytest.raises(L.DlwpError, match="no captured step"):
        model.set_step_graphs(True)


def test_variant_query():
    """dlwp_conv3x3_mfma_variant: 16 * tile width + NF, the launcher's rule (live fragments, then 512 workgroups)"""
    v = L.load().dlwp_conv3x3_mfma_variant
    assert v(0, 8, 8, 8) == 0 and v(1, 8, 8, 0) == 0
    assert v(12, 8, 8, 6) == 8 * 16 + 1         # 8 x 8: 4 live two-row fragments against 8 half-empty rows
    assert v(1, 9, 10, 17) == 16 * 16 + 1       # 9 x 10: 9 rows of 16 against 2 x 5 fragments
    assert v(384, 32, 32, 136) == 16 * 16 + 4   # tie -> 8 x 16; 8 tiles x 384 faces x 3 chunks >= 512
    assert v(8, 64, 64, 64) == 16 * 16 + 2 and v(24, 20, 20, 200) == 8 * 16 + 4


def test_the_3x3_queries_are_the_kxk_queries_at_k3():
    """the padded 3x3 layer is (k 3, stride 1, pad 1) of the k x k planner and pack: one tile rule, one pack size"""
    lib = L.load()
    sizes = (1, 2, 3, 7, 8, 9, 15, 16, 17, 20, 32, 33, 37, 64, 181)
    for b in (1, 2, 8, 12, 24, 32, 384, 513):
        for H in sizes:
            for W in sizes:
                for co in (1, 15, 16, 17, 33, 120, 136, 170, 272, 512):
                    assert lib.dlwp_conv3x3_mfma_variant(b, H, W, co) == lib.dlwp_conv2d_mfma_variant(0, b, H, W, co, 3, 1, 1), (b, H, W, co)
    for co, ci in ((1, 1), (16, 33), (170, 19), (272, 272), (65536, 65536), (1 << 20, 1 << 20)):
        got = lib.dlwp_conv3x3_mfma_packed_bytes(co, ci)        # the last two: 0 or a size, no crash
        assert got == lib.dlwp_conv2d_mfma_packed_bytes(co, ci, 3), (co, ci)
    assert lib.dlwp_conv3x3_mfma_packed_bytes(272, 272) == 3 * 9 * 9 * 17 * 1024


def test_c_abi_is_in_the_ctypes_table():
    for name in ("dlwp_conv3x3_mfma_f32", "dlwp_conv3x3_mfma_pack_f32", "dlwp_conv3x3_mfma_packed_bytes",
                 "dlwp_conv3x3_mfma_variant"):
        assert name in L.SIGNATURES, name
    assert len(L.SIGNATURES["dlwp_conv3x3_mfma_f32"][1]) == 17
    lib = L.load()
    assert lib.dlwp_conv3x3_mfma_packed_bytes(0, 8) == 0 and lib.dlwp_conv3x3_mfma_packed_bytes(8, -1) == 0
    # three bf16 images x 9 taps x ceil(cin / 32) slabs x ceil(cout / 16) fragments x 1 KiB
    assert lib.dlwp_conv3x3_mfma_packed_bytes(170, 19) == 3 * 9 * 1 * 11 * 1024
    assert lib.dlwp_conv3x3_mfma_packed_bytes(16, 33) == 3 * 9 * 2 * 1 * 1024


def test_unknown_form_is_refused_before_any_tensor_check():
    import torch

    from dlwp_benchmark_amd import ops

    x, w = torch.zeros(1, 3, 4, 4), torch.zeros(2, 3, 3, 3)
    for fn in (ops.conv3x3, ops.conv3x3_cyl, ops.conv3x3_hpx):
        with pytest.raises(L.DlwpError, match="unknown conv form"):
            fn(x, w, None, form="fp32")
