"""The HIP input gradients of the non-3x3 convolutions and of AvgPool2d(2) on the GPU (DLWP_CONV_DGRAD=hip), op by op.

Reference: float64 autograd of F.conv2d / F.conv_transpose2d / F.avg_pool2d, computed here.  Bounds: the "bf16x6" form's own
 -- rel-L2 <= 1e-6 and max-abs <= 1e-5 max(1, |want|) against float64; the gradient kernels run the same
arithmetic (three-part bf16 splits, fp32 accumulation), so nothing is widened.  Beyond the bounds: positions no tap reaches
are exactly 0.0, whole-number inputs reproduce float64 exactly, a NaN-filled dx comes back finite, reruns are bit-identical.

Shapes: those of test_conv2_wgrad_cpu.CASES, then what this kernel's tiling adds -- the 4 x 4 window on odd maps, narrow
fragments (two rows of 8 GEMM pixels), several tiles, and a case per (policy, NF, fragment shape) instance, which
test_cases_cover_every_instance asserts through the launcher's own query."""
import functools

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2
from test_conv2_wgrad_cpu import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, ABS = 1e-6, 1e-5


def _from_cases(tag):
    b, cin, cout, h, w, k, s, p, _, transposed, offset = CASES[tag]
    return (b, cin, cout, h, w, k, s, p, offset)


# tag -> (B, cin, cout, H, W of the layer's input, k, stride, padding, offset view)
CONV_CASES = {t: _from_cases(t) for t in ("pointwise", "down_even", "down_odd", "down_unread", "point_s2", "down_s1", "k4_s1",
                                          "down_tiles", "blocks_down", "offset_view")}
CONV_CASES.update({
    "k4_odd_5x7": (1, 3, 2, 5, 7, 4, 2, 1, False),          # the last row and column take a gradient from tap 3 alone
    "k4_odd_3x3": (2, 2, 3, 3, 3, 4, 2, 1, False),
    "k2_s1_p1": (1, 3, 2, 4, 5, 2, 1, 1, False),            # the adjoint padding k - 1 - p = 0
    "narrow_16": (1, 72, 70, 16, 16, 3, 2, 1, False),       # 8 x 8 GEMM pixels: two rows of 8; three K slabs, five fragments
    "narrow_15": (1, 72, 70, 15, 15, 3, 2, 1, False),       # the same grid, cropped in both axes
    "tiles_19x35": (1, 3, 2, 19, 35, 3, 2, 1, False),       # 10 x 18 GEMM pixels: three tiles of two rows of 8
    "tiles_20x63": (1, 3, 2, 20, 63, 4, 2, 1, False),       # 10 x 32 GEMM pixels: 2 x 2 tiles, rows of 16, odd width
    "tiles_s1": (1, 3, 2, 19, 35, 3, 1, 1, False),
    "window_p0": (1, 3, 2, 6, 9, 3, 2, 0, False),           # what the 4 x 4 window holds beside the required envelope
    "window_p2": (1, 2, 3, 5, 6, 4, 2, 2, False),
    "par_nf4_tw8": (64, 208, 8, 16, 16, 3, 2, 1, False),
    "par_nf2_tw8": (64, 128, 8, 16, 16, 3, 2, 1, False),
    "par_nf4_tw16": (64, 208, 8, 16, 32, 4, 2, 1, False),
    "par_nf2_tw16": (64, 128, 8, 16, 32, 2, 2, 0, False),
    "s1_nf4_tw8": (128, 208, 8, 8, 8, 3, 1, 1, False),
    "s1_nf2_tw8": (128, 128, 8, 8, 8, 1, 1, 0, False),
    "s1_nf4_tw16": (128, 208, 8, 8, 16, 1, 1, 0, False),
    "s1_nf2_tw16": (128, 128, 8, 8, 16, 3, 1, 1, False),
    "s1_nf1_tw16": (1, 2, 3, 8, 16, 3, 1, 1, False),
})
UP_CASES = {t: _from_cases(t) for t in ("up2", "up4", "up4_ragged", "up4_tiles", "up1_holes", "k2_s1", "blocks_up")}
REFUSED = ((4, 2, 3), (5, 1, 2), (5, 2, 2), (3, 3, 1), (2, 2, 1))


def out_hw(h, w, k, s, p, transposed=False):
    if transposed:
        return (h - 1) * s - 2 * p + k, (w - 1) * s - 2 * p + k
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


def _draw(name, shape, integer, std=1.0):
    from dlwp_benchmark_amd import weights

    t = weights.normal(name, shape, std=1.0 if integer else std)
    return (4.0 * t).round().clamp(-8, 8) if integer else t


@functools.lru_cache(maxsize=None)
def case(tag, transposed=False, integer=False):
    """(weight, gz, want) on the CPU: fp32 inputs and the float64 input gradient by autograd; computed once, not to be modified"""
    b, cin, cout, h, w, k, s, p, _ = (UP_CASES if transposed else CONV_CASES)[tag]
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    wgt = _draw(f"conv2_dgrad/{tag}/w", wshape, integer, std=(k * k * cout) ** -0.5)
    gz = _draw(f"conv2_dgrad/{tag}/gz", (b, cout, *out_hw(h, w, k, s, p, transposed)), integer)
    x = torch.zeros(b, cin, h, w, dtype=torch.float64, requires_grad=True)
    conv = F.conv_transpose2d if transposed else F.conv2d
    want = torch.autograd.grad(conv(x, wgt.double(), stride=s, padding=p), x, gz.double())[0]
    return wgt, gz, want


def _offset(t):
    """the same values one float into a fresh storage: a 4-byte-aligned, not 8-byte-aligned pointer"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 == 4
    return v


def _run_conv(tag, integer=False, prefill=None):
    from dlwp_benchmark_amd import ops

    b, cin, cout, h, w, k, s, p, offset = CONV_CASES[tag]
    wgt, gz, want = case(tag, False, integer)
    put = _offset if offset else (lambda t: t.to(DEV))
    wd, gd = put(wgt), put(gz)
    out = None
    if offset or prefill is not None:
        out = _offset(torch.empty(b, cin, h, w)) if offset else torch.empty(b, cin, h, w, device=DEV)
        out.fill_(float("nan") if prefill is None else prefill)
    got = ops.conv2d_input_grad(gd, wd, (b, cin, h, w), s, p, out=out)
    torch.cuda.synchronize()
    return got, want, wd, gd


def check(got, want, tag):
    rel = rel_l2(got, want)
    worst = float(((got.double().cpu() - want).abs() / want.abs().clamp_min(1.0)).max())
    print(tag, "rel-L2 %.2e max-abs/max(1,|want|) %.2e" % (rel, worst))
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert rel <= REL and worst <= ABS, (tag, rel, worst)


def dgrad_variant(tag):
    """(policy, fragment width, NF) the launcher takes: 0 ZeroPadWindow<8> on the reversed pack, 1 DgradParity"""
    from dlwp_benchmark_amd import lib

    b, cin, cout, h, w, k, s, p, _ = CONV_CASES[tag]
    v = int(lib.load().dlwp_conv2d_dgrad_mfma_variant(b, cin, cout, h, w, k, s, p))
    assert v > 0, tag
    return (v >> 10) & 1, (v & 1023) // 16, v & 15


def test_cases_cover_every_instance():
    seen = {dgrad_variant(t) for t in CONV_CASES}
    assert seen == {(pol, tw, nf) for pol in (0, 1) for tw in (8, 16) for nf in (1, 2, 4)}, seen
    assert dgrad_variant("narrow_16")[1] == 8 and dgrad_variant("narrow_15")[1] == 8
    assert dgrad_variant("tiles_20x63") == (1, 16, 1)


@pytest.mark.parametrize("tag", sorted(CONV_CASES))
def test_conv2d_input_grad(tag):
    got, want, wd, gd = _run_conv(tag, prefill=float("nan"))
    assert bool(torch.isfinite(got).all()), "an element of dx was not written"
    check(got, want, tag)
    # positions no tap reaches: exactly 0.0 (computed, not left over)
    b, cin, cout, h, w, k, s, p, _ = CONV_CASES[tag]
    x = torch.zeros(1, 1, h, w, dtype=torch.float64, requires_grad=True)
    oh, ow = out_hw(h, w, k, s, p)
    reach = torch.autograd.grad(F.conv2d(x, torch.ones(1, 1, k, k, dtype=torch.float64), stride=s, padding=p), x,
                                torch.ones(1, 1, oh, ow, dtype=torch.float64))[0][0, 0] > 0
    if not bool(reach.all()):
        dead = got.cpu()[:, :, ~reach]
        assert dead.numel() and torch.equal(dead, torch.zeros_like(dead)), tag
    if tag in ("down_unread", "point_s2"):
        assert not bool(reach.all())


@pytest.mark.parametrize("tag", ["pointwise", "down_odd", "down_unread", "point_s2", "k4_s1", "blocks_down", "k4_odd_5x7",
                                 "narrow_15", "tiles_20x63", "window_p2", "k2_s1_p1"])
def test_whole_numbers_are_exact(tag):
    """inputs in [-8, 8]: every product and partial sum is a whole number below 2^24, so fp32 accumulation of the three-part
    splits is exact and the result equals float64's"""
    got, want, _, _ = _run_conv(tag, integer=True)
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(got.double().cpu(), want), tag


@pytest.mark.parametrize("tag", ["down_odd", "down_s1", "narrow_15", "par_nf2_tw8"])
def test_reruns_are_bit_identical(tag):
    a, _, _, _ = _run_conv(tag)
    b, _, _, _ = _run_conv(tag, prefill=123.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("tag", sorted(UP_CASES))
def test_conv_transpose2d_input_grad(tag):
    from dlwp_benchmark_amd import ops

    b, cin, cout, h, w, k, s, p, _ = UP_CASES[tag]
    wgt, gz, want = case(tag, True)
    assert ops.conv_transpose2d_input_grad_supported(b, cin, cout, *gz.shape[2:], k, s, p)
    wd = wgt.to(DEV)
    got = ops.conv_transpose2d_input_grad(gz.to(DEV), wd, s, p)
    check(got, want, tag)
    assert torch.equal(got, ops.conv_transpose2d_input_grad(gz.to(DEV), wd, s, p))
    wi, gi, wanti = case(tag, True, True)
    assert torch.equal(ops.conv_transpose2d_input_grad(gi.to(DEV), wi.to(DEV), s, p).double().cpu(), wanti)


@pytest.mark.parametrize("k,s,p", REFUSED)
def test_refused_geometries(k, s, p, monkeypatch):
    """the C entry answers DLWP_ERR_UNSUPPORTED before any launch, ops raises, and the autograd Function gives the library's
    gradient: bit for bit what DLWP_CONV_DGRAD=torch gives"""
    from dlwp_benchmark_amd import lib, ops, training, weights

    h, w = 9, 12
    oh, ow = out_hw(h, w, k, s, p)
    wgt = weights.normal(f"conv2_dgrad/refused/{k}{s}{p}/w", (4, 3, k, k)).to(DEV)
    gz = weights.normal(f"conv2_dgrad/refused/{k}{s}{p}/gz", (1, 4, oh, ow)).to(DEV)
    assert not ops.conv2d_input_grad_supported(1, 3, 4, h, w, k, s, p)
    dx = torch.full((1, 3, h, w), 7.0, device=DEV)
    pk = torch.zeros(3 * 16 * 1024 // 4, dtype=torch.int32, device=DEV)
    rc = lib.launch("dlwp_conv2d_dgrad_mfma_f32", gz.device, gz, pk, dx, 1, 3, h, w, 4, k, s, p, accept=(lib.ERR_UNSUPPORTED,))
    torch.cuda.synchronize()
    assert rc == lib.ERR_UNSUPPORTED and bool((dx == 7.0).all())
    with pytest.raises(lib.DlwpError, match="no HIP kernel"):
        ops.conv2d_input_grad(gz, wgt, (1, 3, h, w), s, p)

    x = weights.normal(f"conv2_dgrad/refused/{k}{s}{p}/x", (1, 3, h, w)).to(DEV)
    grads = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("DLWP_CONV_DGRAD", mode)
        calls = []
        real = training.conv2d_input_grad_torch
        monkeypatch.setattr(training, "conv2d_input_grad_torch", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
        xi, wi = x.clone().requires_grad_(True), wgt.clone().requires_grad_(True)
        ops.conv2d(xi, wi, None, stride=s, padding=p, act=ops.ACTS["gelu"]).backward(gz)
        monkeypatch.setattr(training, "conv2d_input_grad_torch", real)
        assert calls == [1], mode
        grads[mode] = (xi.grad, wi.grad)
    if k <= 4 and s <= 2 and p < k:      # the forward kernel takes the layer, so only dx is the library's under "hip"
        assert rel_l2(grads["hip"][0], grads["torch"][0]) <= 1e-5
    else:
        assert torch.equal(grads["hip"][0], grads["torch"][0]) and torch.equal(grads["hip"][1], grads["torch"][1])


def test_weight_update_repacks_the_adjoint():
    """the ops called directly cache their packs under the project's one derivation rule: forward and adjoint packs of one
    tensor live in slots of their own, an in-place write re-derives both, a write through .data is signalled by the pack epoch.
    (The training path reads no cached pack at all: test_forward_and_dx_follow_the_optimizer.)"""
    from dlwp_benchmark_amd import ops

    for tag in ("down_odd", "down_s1"):
        b, cin, cout, h, w, k, s, p, _ = CONV_CASES[tag]
        wgt, gz, want = case(tag)
        wd, gd = wgt.to(DEV).requires_grad_(True), gz.to(DEV)
        x = torch.zeros(b, cin, h, w, device=DEV)
        with torch.no_grad():
            y0 = ops.conv2d(x + 1.0, wd, None, stride=s, padding=p, form="bf16x6")
            dx0 = ops.conv2d_input_grad(gd, wd, x.shape, s, p)
            fwd, adj = ops.conv2d_weights(wd).get(wd), None
            v = dgrad_variant(tag)
            adj = ops.conv2d_adjoint_weights(wd, k + (k & 1) if v[0] else k, not v[0]).get(wd)
            assert fwd.data_ptr() != adj.data_ptr()
            wd.mul_(2.0)                                  # an in-place update, as an optimizer's: the version moves
            dx1 = ops.conv2d_input_grad(gd, wd, x.shape, s, p)
            y1 = ops.conv2d(x + 1.0, wd, None, stride=s, padding=p, form="bf16x6")
            assert torch.equal(dx1, 2.0 * dx0) and torch.equal(y1, 2.0 * y0)
            wd.data.mul_(2.0)                             # a write through .data keeps the version: the pack epoch is the signal
            ops.bump_pack_epoch()
            dx2 = ops.conv2d_input_grad(gd, wd, x.shape, s, p)
            assert torch.equal(dx2, 4.0 * dx0)
        check(dx2 / 4.0, want, tag)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 2, 2), (2, 4, 64, 64), (4, 17, 255, 257)])
def test_avgpool_backward(shape):
    """the last shape lies past the grid cap (planes * OH * OW > 2^20): the grid-stride loop takes more than one trip"""
    from dlwp_benchmark_amd import ops, weights

    n, c, h, w = shape
    if shape[0] == 4:
        assert n * c * (h // 2) * (w // 2) > 2 ** 20
    gy = weights.normal(f"conv2_dgrad/pool/{h}x{w}", (n, c, h // 2, w // 2)).to(DEV)
    x = torch.zeros(shape, device=DEV, requires_grad=True)
    want = torch.autograd.grad(F.avg_pool2d(x, 2), x, gy)[0]
    got = ops.avgpool2x2_backward(gy, h, w)
    assert torch.equal(got, want)


def test_avgpool_autograd(monkeypatch):
    from dlwp_benchmark_amd import ops, weights

    x0 = weights.normal("conv2_dgrad/pool/x", (2, 3, 5, 7)).to(DEV)
    gy = weights.normal("conv2_dgrad/pool/gy", (2, 3, 2, 3)).to(DEV)
    monkeypatch.setenv("DLWP_CONV_DGRAD", "hip")
    monkeypatch.setattr(F, "avg_pool2d", _raiser("F.avg_pool2d"))
    x = x0.clone().requires_grad_(True)
    y = ops.avgpool2x2(x)
    y.backward(gy)
    monkeypatch.undo()
    xr = x0.clone().requires_grad_(True)
    yr = F.avg_pool2d(xr, 2)
    yr.backward(gy)
    assert rel_l2(y, yr) <= 1e-6 and torch.equal(x.grad, xr.grad)


def _raiser(name):
    def f(*a, **kw):
        raise AssertionError(f"{name} was called under DLWP_CONV_DGRAD=hip")
    return f


WIRING = {   # tag -> (B, cin, cout, H, W, k, s, p, pre_act, transposed)
    "down_even": (2, 6, 4, 8, 16, 3, 2, 1, "gelu", False),
    "down_odd": (1, 3, 5, 5, 7, 3, 2, 1, "silu", False),
    "pointwise": (2, 5, 7, 3, 5, 1, 1, 0, "none", False),
    "k4_s1": (1, 2, 2, 5, 5, 4, 1, 1, "relu", False),
    "up4_ragged": (2, 3, 4, 3, 5, 4, 2, 1, "none", True),
    "up2": (2, 6, 5, 4, 8, 2, 2, 0, "none", True),
}


# (x, weight, bias, resid) of needs_input_grad; the transposed layer has no residual
NEEDS = [(True, True, True, True), (True, False, False, False), (False, True, True, False), (False, False, False, True)]
WIRING_RUNS = [(t, n) for t in sorted(WIRING) for n in NEEDS if any(n[:3]) or not WIRING[t][9]]


@pytest.mark.parametrize("tag,needs", WIRING_RUNS)
def test_autograd_wiring(tag, needs, monkeypatch):
    """ops.conv2d with pre-activation, GELU and residual, ops.conv_transpose2d with GELU, under DLWP_CONV_DGRAD=hip with the
    library calls replaced by functions that raise: output and every wanted gradient against float64 autograd (bound 1e-5, that
    of test_conv2_wgrad_gpu.test_autograd_wiring), every subset of needs_input_grad"""
    from dlwp_benchmark_amd import ops, training, weights

    b, cin, cout, h, w, k, s, p, pre, transposed = WIRING[tag]
    pre_act, act = ops.ACTS[pre], ops.ACTS["gelu"]
    oh, ow = out_hw(h, w, k, s, p, transposed)
    x = weights.normal(f"conv2_dgrad/wire/{tag}/x", (b, cin, h, w))
    wgt = weights.normal(f"conv2_dgrad/wire/{tag}/w", (cin, cout, k, k) if transposed else (cout, cin, k, k), std=(k * k * cin) ** -0.5)
    bias = weights.normal(f"conv2_dgrad/wire/{tag}/b", (cout,), std=0.5)
    resid = None if transposed else weights.normal(f"conv2_dgrad/wire/{tag}/r", (b, cout, oh, ow))
    gy = weights.normal(f"conv2_dgrad/wire/{tag}/gy", (b, cout, oh, ow))
    tensors = [t for t in (x, wgt, bias, resid) if t is not None]
    needs = list(needs)[:len(tensors)]

    def run(ins, conv, up):
        return up(ins[0], ins[1], ins[2]) if transposed else conv(*ins)

    ref = [t.double().requires_grad_(n) for t, n in zip(tensors, needs)]
    yr = run(ref, lambda x_, w_, b_, r_: training.conv2d_torch(x_, w_, b_, r_, s, p, pre_act, act),
             lambda x_, w_, b_: training.conv_transpose2d_torch(x_, w_, b_, s, p, act))
    yr.backward(gy.double())

    monkeypatch.setenv("DLWP_CONV_DGRAD", "hip")
    monkeypatch.setenv("DLWP_CONV_WGRAD", "hip")
    for name in ("conv2d_torch", "conv_transpose2d_torch", "conv2d_input_grad_torch"):
        monkeypatch.setattr(training, name, _raiser(name))
    ins = [t.to(DEV).requires_grad_(n) for t, n in zip(tensors, needs)]
    y = run(ins, lambda x_, w_, b_, r_: ops.conv2d(x_, w_, b_, stride=s, padding=p, pre_act=pre_act, act=act, resid=r_),
            lambda x_, w_, b_: ops.conv_transpose2d(x_, w_, b_, stride=s, padding=p, act=act))
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    print(tag, "y %.2e" % rel_l2(y, yr))
    assert rel_l2(y, yr) <= 1e-5
    for name, got, want, need in zip(("x", "weight", "bias", "resid"), ins, ref, needs):
        if not need:
            assert got.grad is None, name
            continue
        print(tag, name, "%.2e" % rel_l2(got.grad, want.grad))
        assert rel_l2(got.grad, want.grad) <= 1e-5, name

    # act = 0: the forward under autograd is the inference form "bf16x6" bit for bit
    y0 = run(ins, lambda x_, w_, b_, r_: ops.conv2d(x_, w_, b_, stride=s, padding=p, pre_act=pre_act, act=0, resid=r_),
             lambda x_, w_, b_: ops.conv_transpose2d(x_, w_, b_, stride=s, padding=p, act=0))
    with torch.no_grad():
        y1 = run(ins, lambda x_, w_, b_, r_: ops.conv2d(x_, w_, b_, stride=s, padding=p, pre_act=pre_act, act=0, resid=r_, form="bf16x6"),
                 lambda x_, w_, b_: ops.conv_transpose2d(x_, w_, b_, stride=s, padding=p, act=0, form="bf16x6"))
    assert y0.requires_grad and torch.equal(y0.detach(), y1)


def test_wide_healpix_input_grad(monkeypatch):
    """_conv3x3_backward's two-step form with HPX_DX_DIRECT_MAX_COUT patched to 0: dlwp_conv2d_dgrad_mfma_f32 (k 3, stride 1,
    adjoint padding 2) onto the padded face + dlwp_healpix_pad_bwd_f32, against the direct kernel's result.  Both are fp32-grade
    evaluations of the same sum, each within 1e-6 of float64 by its own tests: 2e-6 between them."""
    from dlwp_benchmark_amd import ops, training, weights

    monkeypatch.setenv("DLWP_CONV_DGRAD", "hip")
    x = weights.normal("conv2_dgrad/hpx/x", (12, 5, 8, 8)).to(DEV)
    wgt = weights.normal("conv2_dgrad/hpx/w", (7, 5, 3, 3), std=45 ** -0.5).to(DEV)
    gy = weights.normal("conv2_dgrad/hpx/gy", (12, 7, 8, 8)).to(DEV)

    def dx_of():
        xi = x.clone().requires_grad_(True)
        ops.conv3x3(xi, wgt, None, act=ops.ACTS["gelu"], pre_act=ops.ACTS["silu"], hpx=True).backward(gy)
        return xi.grad

    direct = dx_of()
    monkeypatch.setattr(training, "HPX_DX_DIRECT_MAX_COUT", 0)
    monkeypatch.setattr(F, "conv_transpose2d", _raiser("F.conv_transpose2d"))
    calls = []
    real = ops.conv2d_input_grad
    monkeypatch.setattr(ops, "conv2d_input_grad", lambda *a, **kw: (calls.append(a[2:]), real(*a, **kw))[1])
    wide = dx_of()
    assert calls == [((12, 5, 10, 10), 1, 0)]
    print("wide-HEALPix dx against the direct kernel: %.2e" % rel_l2(wide, direct))
    assert rel_l2(wide, direct) <= 2e-6


def test_unset_switch_calls_no_new_op(monkeypatch):
    from dlwp_benchmark_amd import ops, weights

    monkeypatch.delenv("DLWP_CONV_DGRAD", raising=False)
    for name in ("conv2d_input_grad", "conv_transpose2d_input_grad", "avgpool2x2_backward"):
        monkeypatch.setattr(ops, name, _raiser(name))
    x = weights.normal("conv2_dgrad/unset/x", (1, 3, 6, 8)).to(DEV).requires_grad_(True)
    wgt = weights.normal("conv2_dgrad/unset/w", (4, 3, 3, 3)).to(DEV).requires_grad_(True)
    wup = weights.normal("conv2_dgrad/unset/wu", (4, 2, 2, 2)).to(DEV).requires_grad_(True)
    y = ops.conv_transpose2d(ops.avgpool2x2(ops.conv2d(x, wgt, None, stride=1, padding=1)), wup, None, stride=2)
    y.sum().backward()
    want = F.conv_transpose2d(F.avg_pool2d(F.conv2d(x.detach(), wgt.detach(), padding=1), 2), wup.detach(), stride=2)
    assert rel_l2(y, want) <= 1e-6 and x.grad is not None


# ---- the training path never reads a cached pack -----------------------------------------------------------------------
# Parameters are also written by launches that move no version counter (optim.FusedAdamW writes through a device table of raw
# pointers; a write through .data) and inside replayed step graphs.  The Functions therefore pack the weight in every call.
LIVE = {   # tag -> (B, cin, cout, H, W, k, s, p, transposed)
    "down_odd": (1, 3, 5, 5, 7, 3, 2, 1, False),
    "down_s1": (1, 2, 3, 4, 4, 3, 1, 1, False),
    "up4_ragged": (2, 3, 4, 3, 5, 4, 2, 1, True),
}


def _live_layer(tag):
    from dlwp_benchmark_amd import weights

    b, cin, cout, h, w, k, s, p, transposed = LIVE[tag]
    wgt = weights.normal(f"conv2_dgrad/live/{tag}/w", (cin, cout, k, k) if transposed else (cout, cin, k, k), std=(k * k * cin) ** -0.5)
    bias = weights.normal(f"conv2_dgrad/live/{tag}/b", (cout,), std=0.5)
    x = weights.normal(f"conv2_dgrad/live/{tag}/x", (b, cin, h, w))
    gy = weights.normal(f"conv2_dgrad/live/{tag}/gy", (b, cout, *out_hw(h, w, k, s, p, transposed)))
    return wgt, bias, x, gy


def _live_run(tag, wgt, bias, x, gy):
    """(y, dx) of the layer under autograd, act = 0"""
    from dlwp_benchmark_amd import ops

    s, p, transposed = LIVE[tag][6:]
    xi = x.detach().clone().requires_grad_(True)
    y = ops.conv_transpose2d(xi, wgt, bias, stride=s, padding=p) if transposed else ops.conv2d(xi, wgt, bias, stride=s, padding=p)
    dx, = torch.autograd.grad(y, xi, gy)
    return y.detach(), dx


def _live_want(tag, wgt, bias, x, gy):
    """the same in float64 from the values the parameters hold NOW"""
    s, p, transposed = LIVE[tag][6:]
    xi = x.detach().double().cpu().requires_grad_(True)
    conv = F.conv_transpose2d if transposed else F.conv2d
    y = conv(xi, wgt.detach().double().cpu(), bias.detach().double().cpu(), stride=s, padding=p)
    dx, = torch.autograd.grad(y, xi, gy.double().cpu())
    return y.detach(), dx


def _live_check(tag, got, want, what):
    for name, g, w_ in zip(("y", "dx"), got, want):
        rel = rel_l2(g, w_)
        print(tag, what, name, "%.2e" % rel)
        assert rel <= REL, (tag, what, name, rel)


@pytest.mark.parametrize("tag", sorted(LIVE))
def test_forward_and_dx_follow_the_optimizer(tag, monkeypatch):
    """forward, backward, FusedAdamW.step(), forward again under DLWP_CONV_DGRAD=hip: the second forward and dx are those of the
    updated weights (bound: the op's own 1e-6 against float64; stale weights would be off by the update, O(0.1)); the same
    after ExponentialMovingAverage's apply_shadow / restore and after a write through .data, with no call in between"""
    from dlwp_benchmark_amd import optim, training

    monkeypatch.setenv("DLWP_CONV_DGRAD", "hip")
    for name in ("conv2d_torch", "conv_transpose2d_torch", "conv2d_input_grad_torch"):
        monkeypatch.setattr(training, name, _raiser(name))
    wgt, bias, x, gy = (t.to(DEV) for t in _live_layer(tag))
    wgt, bias = torch.nn.Parameter(wgt), torch.nn.Parameter(bias)
    s, p, transposed = LIVE[tag][6:]
    from dlwp_benchmark_amd import ops

    opt = optim.FusedAdamW([wgt, bias], lr=0.1, weight_decay=0.0)
    before = wgt.detach().clone()
    for step in range(2):
        xi = x.clone().requires_grad_(True)
        y = ops.conv_transpose2d(xi, wgt, bias, stride=s, padding=p) if transposed else ops.conv2d(xi, wgt, bias, stride=s, padding=p)
        y.backward(gy)
        opt.step()
        opt.zero_grad()
        torch.cuda.synchronize()
        assert float((wgt.detach() - before).abs().max()) > 0.05 * (step + 1) * 0.9, "the optimizer did not move the weights"
        _live_check(tag, _live_run(tag, wgt, bias, x, gy), _live_want(tag, wgt, bias, x, gy), f"after step {step}")

    class _M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w, self.b = wgt, bias

    ema = optim.ExponentialMovingAverage(_M(), 0.5)
    ema.register()
    with torch.no_grad():
        wgt.data.mul_(3.0)
    ema.update()
    ema.apply_shadow()
    _live_check(tag, _live_run(tag, wgt, bias, x, gy), _live_want(tag, wgt, bias, x, gy), "under the EMA shadow")
    ema.restore()
    _live_check(tag, _live_run(tag, wgt, bias, x, gy), _live_want(tag, wgt, bias, x, gy), "after restore")

    version = wgt._version
    wgt.data.mul_(2.0)                      # neither pointer nor version moves, and nobody bumps the pack epoch
    assert wgt._version == version
    _live_check(tag, _live_run(tag, wgt, bias, x, gy), _live_want(tag, wgt, bias, x, gy), "after .data.mul_(2)")


@pytest.mark.parametrize("tag", ["down_odd", "up4_ragged"])
def test_replayed_step_reads_the_live_weights(tag, monkeypatch):
    """forward + backward captured once and replayed after the weights changed in place: the pack launch is part of the capture,
    so the replay computes with the new values"""
    monkeypatch.setenv("DLWP_CONV_DGRAD", "hip")
    wgt, bias, x, gy = (t.to(DEV) for t in _live_layer(tag))
    wgt, bias = torch.nn.Parameter(wgt), torch.nn.Parameter(bias)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _live_run(tag, wgt, bias, x, gy)            # every kernel has run once before anything is captured
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, dx = _live_run(tag, wgt, bias, x, gy)
    for factor in (1.0, -2.0, 0.5):
        wgt.data.mul_(factor)
        graph.replay()
        torch.cuda.synchronize()
        _live_check(tag, (y, dx), _live_want(tag, wgt, bias, x, gy), f"replay x{factor}")


def test_avgpool_backward_past_32_bit_indices():
    """planes * H * W >= 2^31: the launcher takes the kernel's 64-bit index form (every other shape here takes the 32-bit one);
    odd width, so the last column is the uncovered one.  Checked against the closed form, block by block of rows."""
    from dlwp_benchmark_amd import ops

    n, c, h, w = 1, 2, 32768, 32769
    assert n * c * h * w >= 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(5)
    gy = torch.randn(n, c, h // 2, w // 2, device=DEV, generator=g)
    got = ops.avgpool2x2_backward(gy, h, w)
    torch.cuda.synchronize()
    assert not bool(got[:, :, :, w - 1].any())
    for r0 in range(0, h, 4096):
        want = 0.25 * gy[:, :, r0 // 2:(r0 + 4096) // 2].repeat_interleave(2, 2).repeat_interleave(2, 3)
        assert torch.equal(got[:, :, r0:r0 + 4096, :w - 1], want), r0
