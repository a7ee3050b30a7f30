"""The weight / bias gradient of the strided, 1x1 and transposed convolutions without a GPU: the cases and fp64 references that
test_conv2_wgrad_gpu.py runs dlwp_conv2d_wgrad_f32 against, the library form conv2d_weight_grad_torch against the same
references, the exchange of roles that lets one kernel serve Conv2d and ConvTranspose2d, the DLWP_CONV_WGRAD switch and the
C ABI table.

CASES: tag -> (B, cin, cout, H, W of the layer's input, k, stride, padding, pre_act, transposed, offset).  The kernel
(csrc/conv_wgrad.hip) works on 64 x 64 channel blocks as 2 x 2 waves of 32 x 32, on tiles of the smaller map of 8 x 8 pixels
(stride 1) or 4 x 8 (stride 2) consumed two pixels per matrix instruction, one instantiation per (k, stride), the taps of k = 4
in two groups of two kernel rows, K-slices of at least 256 pixels (4 / 8 tiles).  Each case is the smallest at which a part of
it can go wrong:
  pointwise     k1 s1: one tap, 15 pixels (a partial last pair), both channel axes mostly zero-fill
  down_even     k3 s2 p1, GELU at load: top / left padding read, bottom / right not
  down_odd      k3 s2 p1: padding read on all four sides, partial tile
  down_unread   k2 s2 p0 on 5 x 7: the last row and column of x belong to no output
  down_s1       k3 s1 p1, SiLU at load: stride 1 with padding
  up2           convT k2 s2 p0: disjoint taps
  up4           convT k4 s2 p1: sixteen taps in two groups, taps falling outside the output on every side
  up4_ragged    convT k4 s2 p1 on 3 x 5: map no multiple of any tile
  blocks_down   k3 s2 p1, 40 -> 36: a full and a partial 32-channel quarter on both axes
  blocks_up     convT k4 s2 p1, 68 -> 40: a second 64-channel block with 4 live channels
  multi_slice   five 1 x 1 maps through a 1x1 convolution: 5 stride-1 tiles -> 2 slices of 4 and 1 tiles
  offset_view   down_even with every tensor one float into its storage (4-byte-aligned pointers)
and, for edges this tiling adds:
  multi_slice_s2  convT k2 s2 on nine 1 x 1 maps: 9 stride-2 tiles -> 2 slices of 8 and 1; the bias summed from the large map
  down_tiles    k3 s2 p1 on 10 x 18 -> 5 x 9: two tile rows and columns of the 4 x 8 tile, the halo origin of a later tile
  up4_tiles     convT k4 s2 p1 on 5 x 9: the same for the transposed layer, whose bias is summed from overlapping halos (each
                position owned by one tile, the last tile row / column owning the halo's tail)
  up1_holes     convT k1 s2: k < stride, output positions no tap reaches still count in db
  point_s2      k1 s2 (the strided 1x1 shortcut): the (1, 2) instantiation on a map with unread rows and columns
  k2_s1         convT k2 s1: the (2, 1) instantiation
  k4_s1         k4 s1 p1, ReLU at load: the (4, 1) instantiation, two tap groups over an 8 x 8 tile"""
import functools

import pytest
import torch

from dlwp_benchmark_amd import lib, ops, training, weights
from dlwp_benchmark_amd.training import conv2d_weight_grad_torch, conv2_wgrad_uses_hip  # noqa: F401 (the feature)

A = ops.ACTS
CASES = {
    "pointwise": (2, 5, 7, 3, 5, 1, 1, 0, A["none"], False, False),
    "down_even": (2, 6, 4, 8, 16, 3, 2, 1, A["gelu"], False, False),
    "down_odd": (1, 3, 5, 5, 7, 3, 2, 1, A["none"], False, False),
    "down_unread": (1, 3, 2, 5, 7, 2, 2, 0, A["none"], False, False),
    "down_s1": (1, 2, 3, 4, 4, 3, 1, 1, A["silu"], False, False),
    "up2": (2, 6, 5, 4, 8, 2, 2, 0, A["none"], True, False),
    "up4": (1, 5, 6, 4, 4, 4, 2, 1, A["none"], True, False),
    "up4_ragged": (2, 3, 4, 3, 5, 4, 2, 1, A["none"], True, False),
    "blocks_down": (1, 40, 36, 8, 8, 3, 2, 1, A["none"], False, False),
    "blocks_up": (1, 68, 40, 4, 4, 4, 2, 1, A["none"], True, False),
    "multi_slice": (5, 1, 1, 1, 1, 1, 1, 0, A["none"], False, False),
    "offset_view": (2, 6, 4, 8, 16, 3, 2, 1, A["gelu"], False, True),
    "multi_slice_s2": (9, 2, 3, 1, 1, 2, 2, 0, A["none"], True, False),
    "down_tiles": (1, 3, 2, 10, 18, 3, 2, 1, A["tanh"], False, False),
    "up4_tiles": (1, 2, 3, 5, 9, 4, 2, 1, A["none"], True, False),
    "up1_holes": (1, 2, 3, 3, 5, 1, 2, 0, A["none"], True, False),
    "point_s2": (1, 3, 2, 5, 7, 1, 2, 0, A["none"], False, False),
    "k2_s1": (1, 2, 2, 3, 3, 2, 1, 0, A["none"], True, False),
    "k4_s1": (1, 2, 2, 5, 5, 4, 1, 1, A["relu"], False, False),
}


def out_hw(tag):
    _, _, _, h, w, k, s, p, _, transposed, _ = CASES[tag]
    if transposed:
        return (h - 1) * s - 2 * p + k, (w - 1) * s - 2 * p + k
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def make_inputs(tag, integer=False):
    """(x, dz) of a case on the CPU, fp32, seeded by the tag; integer: whole numbers in [-3, 3]"""
    b, cin, cout, h, w = CASES[tag][:5]
    seed_tag = "down_even" if tag == "offset_view" else tag

    def draw(name, shape):
        t = weights.normal(f"conv2_wgrad/{seed_tag}/{name}", shape)
        return (1.5 * t).round().clamp(-3, 3) if integer else t

    return draw("x", (b, cin, h, w)), draw("dz", (b, cout, *out_hw(tag)))


@functools.lru_cache(maxsize=None)
def inputs(tag):
    return make_inputs(tag)


def reference_of(x, dz, k, stride, padding, pre_act, transposed):
    """(dW, db) in fp64: autograd of training.conv2d_torch / conv_transpose2d_torch with respect to weight and bias, output
    gradient dz"""
    cin, cout = x.shape[1], dz.shape[1]
    wgt = torch.zeros((cin, cout, k, k) if transposed else (cout, cin, k, k), dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    if transposed:
        assert pre_act == 0
        y = training.conv_transpose2d_torch(x.double(), wgt, bias, stride, padding, 0)
    else:
        y = training.conv2d_torch(x.double(), wgt, bias, None, stride, padding, pre_act, 0)
    assert y.shape == dz.shape
    return torch.autograd.grad(y, (wgt, bias), dz.double())


@functools.lru_cache(maxsize=None)
def reference(tag, pre_act=None):
    """the fp64 (dW, db) of a case (pre_act: instead of the case's); computed once, not to be modified"""
    x, dz = inputs(tag)
    k, s, p, act, transposed = CASES[tag][5:10]
    return reference_of(x, dz, k, s, p, act if pre_act is None else pre_act, transposed)


def deviation(got, want):
    return float((got.detach().double().cpu() - want).norm() / want.norm())


@pytest.mark.parametrize("tag", [t for t in CASES if t != "offset_view"])
def test_library_form_matches_fp64_autograd(tag):
    x, dz = inputs(tag)
    k, s, p, act, transposed = CASES[tag][5:10]
    dw, db = training.conv2d_weight_grad_torch(x, dz, k, s, p, act, transposed)
    want_w, want_b = reference(tag)
    assert dw.dtype == torch.float32 and dw.shape == want_w.shape and db.shape == want_b.shape
    print(tag, "dW %.2e db %.2e" % (deviation(dw, want_w), deviation(db, want_b)))
    assert deviation(dw, want_w) <= 1e-5 and deviation(db, want_b) <= 1e-5


@pytest.mark.parametrize("tag", [t for t in CASES if not CASES[t][9] and t != "offset_view"])
@pytest.mark.parametrize("act", sorted(ops.ACTS.values()))
def test_library_form_matches_for_every_activation(tag, act):
    x, dz = inputs(tag)
    k, s, p = CASES[tag][5:8]
    dw, db = training.conv2d_weight_grad_torch(x, dz, k, s, p, act, False)
    want_w, want_b = reference(tag, act)
    assert deviation(dw, want_w) <= 1e-5 and deviation(db, want_b) <= 1e-5


@pytest.mark.parametrize("tag", [t for t in CASES if CASES[t][9]])
def test_transposed_gradient_is_the_plain_one_with_the_maps_exchanged(tag):
    """what lets one kernel serve both layers: dW of ConvTranspose2d(x -> z) from (x, dz) is dW of Conv2d(z -> x) from
    (input dz, output gradient x), index for index ([cin][cout][k][k] both ways)"""
    x, dz = inputs(tag)
    k, s, p = CASES[tag][5:8]
    want_w, want_b = reference(tag)
    swapped_w, _ = reference_of(dz, x, k, s, p, 0, False)
    assert swapped_w.shape == want_w.shape
    assert float((swapped_w - want_w).abs().max()) <= 1e-12 * float(want_w.abs().max())
    assert float((dz.double().sum(dim=(0, 2, 3)) - want_b).abs().max()) <= 1e-12 * float(want_b.abs().max())


def test_library_form_honours_the_need_flags():
    for tag in ("down_even", "up4"):
        x, dz = inputs(tag)
        k, s, p, act, transposed = CASES[tag][5:10]
        dw, db = training.conv2d_weight_grad_torch(x, dz, k, s, p, act, transposed, need_bias=False)
        assert db is None and dw is not None
        dw, db = training.conv2d_weight_grad_torch(x, dz, k, s, p, act, transposed, need_weight=False)
        assert dw is None and db is not None


def test_integer_inputs_are_exact_in_fp32():
    """what the GPU mapping check relies on: whole numbers in [-3, 3], every partial sum far below 2^24"""
    for tag in ("blocks_down", "down_tiles", "blocks_up", "up4_tiles"):
        x, dz = make_inputs(tag, integer=True)
        for t in (x, dz):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3 and len(t.unique()) == 7
        k, s, p, _, transposed = CASES[tag][5:10]
        pixels = max(x.shape[0] * x.shape[2] * x.shape[3], dz.shape[0] * dz.shape[2] * dz.shape[3])
        assert 9 * pixels < 2 ** 24
        dw, db = reference_of(x, dz, k, s, p, 0, transposed)
        assert torch.equal(dw, dw.round()) and torch.equal(db, db.round())
        assert float(dw.abs().max()) > 0
        got_w, got_b = training.conv2d_weight_grad_torch(x, dz, k, s, p, 0, transposed)
        assert torch.equal(got_w, dw.float()) and torch.equal(got_b, db.float())


def test_conv_wgrad_switch_governs_these_layers(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("the library was asked")

    layer = (2, 64, 64, 8, 16, 3, 2, 1, False)
    monkeypatch.setattr(ops, "conv2d_weight_grad_supported", refuse)
    monkeypatch.setenv("DLWP_CONV_WGRAD", "torch")
    assert not training.conv2_wgrad_uses_hip(*layer)                        # decided without touching the library
    monkeypatch.delenv("DLWP_CONV_WGRAD", raising=False)
    monkeypatch.setattr(training, "CONV2_WGRAD_AUTO_MIN_FLOPS", 1e9)
    flops = training.conv2_wgrad_flops(*layer)
    assert flops == 2.0 * 2 * 4 * 8 * 64 * 64 * 9 and flops < 1e9
    assert not training.conv2_wgrad_uses_hip(*layer)                        # auto, below the threshold: likewise
    assert training.conv2_wgrad_flops(2, 64, 64, 8, 16, 4, 2, 1, True) == 2.0 * 2 * 8 * 16 * 64 * 64 * 16
    monkeypatch.setattr(ops, "conv2d_weight_grad_supported", lambda *a: "asked")
    monkeypatch.setattr(training, "CONV2_WGRAD_AUTO_MIN_FLOPS", flops)
    assert training.conv2_wgrad_uses_hip(*layer) == "asked"                 # auto, at the threshold
    monkeypatch.setenv("DLWP_CONV_WGRAD", "hip")
    monkeypatch.setattr(training, "CONV2_WGRAD_AUTO_MIN_FLOPS", float("inf"))
    assert training.conv2_wgrad_uses_hip(*layer) == "asked"
    monkeypatch.setenv("DLWP_CONV_WGRAD", "miopen")
    with pytest.raises(lib.DlwpError):
        training.conv2_wgrad_uses_hip(*layer)


def test_envelope_needs_no_gpu():
    assert ops.conv2d_weight_grad_supported(2, 64, 64, 8, 16, 3, 2, 1)
    assert ops.conv2d_weight_grad_supported(1, 1024, 1024, 1, 1, 4, 2, 1, True)
    assert not ops.conv2d_weight_grad_supported(1, 1025, 1, 4, 4, 1, 1, 0)
    assert not ops.conv2d_weight_grad_supported(1, 1, 1, 4, 4, 5, 1, 0)
    assert not ops.conv2d_weight_grad_supported(1, 1, 1, 4, 4, 3, 3, 0)
    assert not ops.conv2d_weight_grad_supported(1, 1, 1, 4, 4, 3, 1, 3)
    assert not ops.conv2d_weight_grad_supported(1, 1, 1, 2, 2, 3, 1, 0)          # the kernel does not fit the map
    assert not ops.conv2d_weight_grad_supported(1, 1, 1, 1, 1, 2, 2, 1, True)    # ConvTranspose2d with an empty output


def test_padded_3x3_layer_is_planned_as_k3_s1_p1():
    """one planner: the 3x3 entry points' slice count and workspace are those of the k x k ones at k 3, stride 1, padding 1,
    shape for shape (the reruns of both are bit-identical by the one slice rule); channels past the envelope give 0 on both"""
    l = lib.load()
    for b in (1, 4, 5, 8, 9):
        for h, w in ((1, 1), (3, 32), (3, 33), (8, 8)):
            for cin, cout in ((1, 1), (2, 3), (65, 64), (1024, 1024), (1025, 1)):
                slices = int(l.dlwp_conv3x3_wgrad_slices(b, h, w, cin, cout))
                nbytes = int(l.dlwp_conv3x3_wgrad_workspace_bytes(b, h, w, cin, cout))
                assert slices == int(l.dlwp_conv2d_wgrad_slices(b, cin, h, w, cout, 3, 1, 1, 0)), (b, h, w, cin, cout)
                assert nbytes == int(l.dlwp_conv2d_wgrad_workspace_bytes(b, cin, h, w, cout, 3, 1, 1, 0)), (b, h, w, cin, cout)
                assert (slices > 0) == (nbytes > 0) == (cin <= 1024)


@pytest.mark.parametrize("tag", ["multi_slice", "tiles"])
def test_cylinder_and_zero_padding_share_the_centre_column(tag):
    """which taps tell CylinderPad(1) from zero padding: the rules differ in the wrapped longitude columns -1 and W alone (the
    latitude rows are zeros under both), and tap (ky, kx) reads column x + kx - 1, so only kx = 0 and kx = 2 reach them.
    In fp64: dW[:, :, :, 1] and db agree, each of the other two columns differs.  What the GPU comparison of the two loaders
    (test_conv2_wgrad_gpu.test_padded_3x3_layer_is_the_k3_s1_p1_instance) relies on."""
    import test_conv3x3_wgrad_cpu as c3

    x0, x1, dz = c3.inputs(tag)
    assert x1 is None and not c3.CASES[tag][7]
    cyl_w, cyl_b = c3.reference(tag, A["relu"])
    zero_w, zero_b = reference_of(x0, dz, 3, 1, 1, A["relu"], False)
    scale = float(cyl_w.abs().max())
    assert float((cyl_w[:, :, :, 1] - zero_w[:, :, :, 1]).abs().max()) <= 1e-12 * scale and scale > 0
    assert float((cyl_b - zero_b).abs().max()) <= 1e-12 * float(cyl_b.abs().max())
    for kx in (0, 2):
        assert float((cyl_w[:, :, :, kx] - zero_w[:, :, :, kx]).abs().max()) > 1e-3 * scale


def test_c_abi_table_has_the_entries():
    for name in ("dlwp_conv2d_wgrad_workspace_bytes", "dlwp_conv2d_wgrad_slices", "dlwp_conv2d_wgrad_f32"):
        assert name in lib.SIGNATURES
    assert len(lib.SIGNATURES["dlwp_conv2d_wgrad_f32"][1]) == 17
    assert len(lib.SIGNATURES["dlwp_conv2d_wgrad_slices"][1]) == 9
