"""The AFNO block's kernels against independent float64 references (tests/afno_ref.py, proved on the CPU by
tests/test_afno_ref_cpu.py, which also holds the case tables and the inputs):

  csrc/afno.hip   dlwp_afno2d_mix_f32 / dlwp_afno2d_mix_scaled_f32: afno_mix_kernel<4 / 8 / 32> and the MFMA form of block size 16,
                  full and kept-column layouts, in place and out of place, grid-stride loops, ragged tiles, fractions below 1;
                  dlwp_afno2d_mix_bwd_f32: gx and the four per-point factors, then the weight-gradient sums formed from them;
                  ops.afno2d_filter_backward as a whole against float64 autograd of the float64 filter
  csrc/norm.hip   dlwp_afno_merge_f32, dlwp_layernorm_nhwc_to_nchw_f32: every NV instantiation, partial tiles and lane groups,
                  the large-LDS path, sum_bias / want_norm, the 4096-tile grid cap

Tolerances come from the references, never from the kernels:
  rel-L2 <= max(2e-6, 4 floor)  and  max |got - want| <= max(1e-5, 4 floor_max) max |want|      (merge / LayerNorm: 1e-6 and 1e-5)
where floor / floor_max are the same two figures of the SAME reference evaluated in float32 on the CPU on the same inputs (what
fp32 arithmetic itself costs there); 2e-6 / 1e-5 are the suite's bounds of this operator family and 4 allows another summation
order.  The ReLU and softshrink masks of the backward are discontinuous: a (point, block) entry with a pre-activation within
1e-4 of a threshold (afno_ref.near_threshold) may legitimately take the other branch in another precision, so gx, d1, d2 and the
sums formed from them are compared with those entries left out on both sides; at most 2 % of the entries may be left out.
The figures observed on the MI355X: DESIGN.md, "AFNO kernels against float64".
"""
import functools

import pytest
import torch

import afno_ref as R
import test_afno_ref_cpu as C
from helpers import rel_l2

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


def _figures(got, want):
    """(rel-L2, max |got - want| / max |want|) in float64 on the CPU"""
    got, want = got.detach().cpu(), want.detach().cpu()
    got = got.to(torch.complex128 if got.is_complex() else torch.float64)
    want = want.to(got.dtype)
    d = got - want
    return float(torch.linalg.vector_norm(d) / torch.linalg.vector_norm(want)), float(d.abs().max() / want.abs().max())


def _check(tag, got, want, f32, failures, l2_floor=2e-6, max_floor=1e-5):
    """got (the kernel) and f32 (the float32 CPU evaluation of the reference) against want (float64); figures are printed
    before anything is judged"""
    e, em = _figures(got, want)
    floor, floor_m = _figures(f32, want)
    tol, tol_m = max(l2_floor, 4 * floor), max(max_floor, 4 * floor_m)
    print("%-58s rel-L2 %.2e (<= %.2e, floor %.2e)  max %.2e (<= %.2e, floor %.2e)" % (tag, e, tol, floor, em, tol_m, floor_m))
    if not e <= tol:
        failures.append((tag, "rel-L2", e, "bound", tol, "floor", floor))
    if not em <= tol_m:
        failures.append((tag, "max", em, "bound", tol_m, "floor", floor_m))


def _kept_mask(case, wf):
    _, _, _, h, _, frac, _ = case
    lo, hi, km = R.kept_region(h, wf, frac)
    keep = torch.zeros(h, wf, dtype=torch.bool)
    keep[lo:hi, :km] = True
    return keep, (lo, hi, km)


def _real_buffer(shape, fill=NAN):
    """interleaved-complex float32 buffer [B, C, H, Wf, 2] on the device"""
    return torch.full((*shape, 2), fill, dtype=torch.float32, device=_dev())


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def _mix_launch(case, xr, yr, wts):
    """the unscaled entry point for the full layout, the scaled one for the kept layout; xr / yr [B, C, H, Wf, 2] device"""
    from dlwp_benchmark_amd import lib as L

    b, c, nb, h, w, frac, layout = case
    wf = xr.shape[3]
    assert xr.is_contiguous() and yr.is_contiguous() and tuple(xr.shape) == tuple(yr.shape) == (b, c, h, wf, 2)
    assert all(t.is_contiguous() and t.device == xr.device and t.dtype == torch.float32 for t in wts)
    if layout == "full":
        L.launch("dlwp_afno2d_mix_f32", xr.device, xr, yr, *wts, b, h, wf, c, nb, C.LAM, frac)
    else:
        si, so = C.scales(case)
        L.launch("dlwp_afno2d_mix_scaled_f32", xr.device, xr, yr, *wts, b, h, wf, c, nb, C.LAM, frac, si, so)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", C.FWD_CASES, ids=C.case_id)
def test_mix_forward_matches_the_fp64_reference(case):
    b, c, nb, h, w, frac, layout = case
    xf, *wts = C.forward_inputs(case)
    wf = xf.shape[-1]
    assert wf == C.spectrum_width(case)
    si, so = C.scales(case)
    want, _ = R.mix(xf, *wts, nb, C.LAM, frac, in_scale=si, out_scale=so)
    f32, _ = R.mix(xf, *wts, nb, C.LAM, frac, in_scale=si, out_scale=so, dtype=torch.float32)
    assert f32.dtype == torch.complex64 and not f32.is_cuda
    keep, (lo, hi, km) = _kept_mask(case, wf)
    assert km >= 1 and bool((want[:, :, ~keep] == 0).all())

    dwts = [t.contiguous().to(_dev()) for t in wts]
    xr = torch.view_as_real(xf).contiguous().to(_dev())
    yr = _real_buffer(xf.shape)
    _mix_launch(case, xr, yr, dwts)
    assert torch.equal(xr.cpu(), torch.view_as_real(xf)), "out of place: the input must survive"
    got = torch.view_as_complex(yr.cpu())
    assert not torch.isnan(yr).any(), f"{int(torch.isnan(yr).sum())} elements were never written"
    outside = torch.view_as_real(got)[:, :, ~keep]
    assert bool((outside == 0).all()), f"{int((outside != 0).sum())} non-zero values outside rows [{lo}, {hi}) x columns [0, {km})"
    failures = []
    _check(f"mix {C.case_id(case)}", got[:, :, keep], want[:, :, keep], f32[:, :, keep], failures)
    if layout == "kept":
        buf = xr.clone()
        _mix_launch(case, buf, buf, dwts)
        assert torch.equal(buf, yr), "in place differs from out of place"
    assert not failures, failures


def test_mix_refusals_are_typed():
    from dlwp_benchmark_amd import lib as L

    dev = _dev()
    z = lambda *s: torch.zeros(*s, device=dev)
    b, h, wf = 1, 12, 7

    def fwd(c, nb, frac):
        bs = c // nb
        L.launch("dlwp_afno2d_mix_scaled_f32", dev, z(b, c, h, wf, 2), z(b, c, h, wf, 2), z(2, nb, bs, bs), z(2, nb, bs), z(2, nb, bs, bs),
                 z(2, nb, bs), b, h, wf, c, nb, C.LAM, frac, 1.0, 1.0)

    def bwd(c, nb, frac):
        bs = c // nb
        bufs = [z(b, c, h, wf, 2) for _ in range(7)]
        L.launch("dlwp_afno2d_mix_bwd_f32", dev, *bufs, z(2, nb, bs, bs), z(2, nb, bs), z(2, nb, bs, bs), z(2, nb, bs), b, h, wf, c, nb,
                 12, C.LAM, frac, 1.0, 1.0)

    for call, args, status, word in ((fwd, (4, 2, 1.0), L.ERR_UNSUPPORTED, "block size 2"),
                                     (bwd, (32, 1, 1.0), L.ERR_UNSUPPORTED, "block size 32"),
                                     (fwd, (8, 2, 0.1), -1, "keeps no mode"),         # int(7 * 0.1) = 0; DLWP_ERR_INVALID_ARGUMENT
                                     (bwd, (8, 2, 0.1), -1, "keeps no mode")):
        with pytest.raises(L.DlwpError) as err:
            call(*args)
        assert err.value.status == status and word in str(err.value), (args, err.value)
    fwd(8, 2, 1.0)       # the same calls with arguments inside the envelope go through
    bwd(8, 2, 1.0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# backward, kernel level
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ("gx", "xin", "o1", "d1", "d2")


@pytest.mark.parametrize("case", C.BWD_CASES, ids=C.case_id)
def test_mix_backward_matches_the_fp64_reference(case):
    from dlwp_benchmark_amd import lib as L

    b, c, nb, h, w, frac, layout = case
    bs = c // nb
    xf, gf, *wts = C.backward_inputs(case)
    wf = xf.shape[-1]
    si, so = C.scales(case)
    want = R.mix_backward(xf, gf, *wts, nb, C.LAM, frac, w, in_scale=si, out_scale=so)
    f32 = R.mix_backward(xf, gf, *wts, nb, C.LAM, frac, w, in_scale=si, out_scale=so, dtype=torch.float32)
    keep, (lo, hi, km) = _kept_mask(case, wf)
    flags = C.bwd_flags(case)                                            # [B, nb, rows, km]
    share = C.flagged_share(flags)
    print(f"{C.case_id(case)}: {100 * share:.2f} % of {flags.numel()} entries flagged")
    assert share <= C.CAP, share

    dev = _dev()
    dwts = [t.contiguous().to(dev) for t in wts]
    xr, gr = (torch.view_as_real(t).contiguous().to(dev) for t in (xf, gf))
    outs = [_real_buffer(xf.shape) for _ in NAMES]
    assert all(o.is_contiguous() and tuple(o.shape) == (b, c, h, wf, 2) == tuple(xr.shape) == tuple(gr.shape) for o in outs)
    L.launch("dlwp_afno2d_mix_bwd_f32", dev, xr, gr, *outs, *dwts, b, h, wf, c, nb, w, C.LAM, frac, si, so)
    torch.cuda.synchronize()
    got = []
    for name, o in zip(NAMES, outs):
        assert not torch.isnan(o).any(), f"{name}: {int(torch.isnan(o).sum())} elements were never written"
        o = o.cpu()
        outside = o[:, :, ~keep]
        assert bool((outside == 0).all()), f"{name}: {int((outside != 0).sum())} non-zero values outside the kept region"
        got.append(torch.view_as_complex(o))

    region = lambda t: t.view(b, nb, bs, h, wf)[:, :, :, lo:hi, :km]
    ok = (~flags)[:, :, None].expand(b, nb, bs, hi - lo, km)             # the entries no threshold is near
    failures = []
    for name, g, wnt, f in zip(NAMES, got, want, f32):
        g, wnt, f = region(g), region(wnt), region(f)
        if name in ("xin", "o1"):                                        # continuous in the inputs: compared everywhere
            _check(f"bwd {C.case_id(case)} {name}", g, wnt, f, failures)
        else:
            _check(f"bwd {C.case_id(case)} {name} (unflagged)", g[ok], wnt[ok], f[ok], failures)
    # the four weight-gradient sums, formed in float64 from the kernel's factors, flagged entries left out on both sides
    keep_full = torch.zeros(b, nb, h, wf, dtype=torch.bool)
    keep_full[:, :, lo:hi, :km] = ~flags
    sums = lambda t: C.weight_gradients(t[1], t[2], t[3], t[4], nb, keep=keep_full)
    for name, g, wnt, f in zip(("dw1", "db1", "dw2", "db2"), sums(got), sums(want), sums(f32)):
        e, floor = rel_l2(g, wnt), rel_l2(f, wnt)
        tol = max(2e-6, 4 * floor)
        print("%-58s rel-L2 %.2e (<= %.2e, floor %.2e)" % (f"bwd {C.case_id(case)} {name}", e, tol, floor))
        if not e <= tol:
            failures.append((name, "rel-L2", e, "bound", tol, "floor", floor))
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# backward, the whole filter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.FILTER_BWD_CASES, ids=C.case_id)
def test_filter_backward_matches_float64_autograd(case):
    """rfft2 of the dx of ops.afno2d_filter_backward against rfft2 of the float64-autograd dx, over the kept half-spectrum entries
    that are not flagged.  The C2R transform symmetrises the self-conjugate columns (0 and W / 2) over the rows h and (H - h) % H,
    so there a flagged entry also takes its mirror row out."""
    from dlwp_benchmark_amd import ops

    b, c, nb, h, w, frac = case
    bs = c // nb
    x, gy, *wts = C.filter_inputs(case)
    lo, hi, km = R.kept_region(h, w // 2 + 1, frac)
    assert km == ops.afno_kept_cols(h, w, frac)

    xin = x.double().requires_grad_(True)
    out, pre = C.filter64(xin, *wts, nb, frac)
    (dx_want,) = torch.autograd.grad(out, xin, gy.double())
    flags = R.near_threshold(tuple(p.detach() for p in pre), C.LAM, C.MARGIN)            # [B, nb, rows, km]
    share = C.flagged_share(flags)
    assert share <= C.CAP, share
    excluded = flags.clone()
    rows = torch.arange(lo, hi)
    mirror = (h - rows) % h
    inside = (mirror >= lo) & (mirror < hi)
    for col in (0, w // 2):
        if col < km:
            excluded[:, :, mirror[inside] - lo, col] |= flags[:, :, rows[inside] - lo, col]
    ok = (~excluded)[:, :, None].expand(b, nb, bs, hi - lo, km)
    print(f"{C.case_id(case)}: {100 * share:.2f} % flagged, {100 * C.flagged_share(excluded):.2f} % excluded with the mirror rows")

    # the floor: the same pipeline (unnormalised transforms around mix_backward) in float32 on the CPU
    s = 1.0 / float(h * w) ** 0.5
    gx32 = R.mix_backward(torch.fft.rfft2(x)[..., :km], torch.fft.rfft2(gy)[..., :km], *wts, nb, C.LAM, frac, w, in_scale=s, out_scale=s,
                          dtype=torch.float32)[0]
    pad = torch.zeros(b, c, h, w // 2 + 1, dtype=torch.complex64)
    pad[..., :km] = gx32
    dx32 = torch.fft.irfft2(pad, s=(h, w)) * (h * w)
    assert dx32.dtype == torch.float32

    got = ops.afno2d_filter_backward(*(t.to(_dev()) for t in (x, gy, *wts)), nb, C.LAM, frac)
    assert got is not None, "the grid should be covered by the hand-written transforms"
    torch.cuda.synchronize()
    spec = lambda t: torch.fft.rfft2(t.detach().double().cpu()).view(b, nb, bs, h, w // 2 + 1)[:, :, :, lo:hi, :km][ok]
    failures = []
    _check(f"filter bwd {C.case_id(case)} rfft2(dx) (unflagged)", spec(got[0]), spec(dx_want), spec(dx32), failures)
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------
# merge and LayerNorm transpose (csrc/norm.hip)
# ---------------------------------------------------------------------------------------------------------------------
EPS = 1e-6
# (B, H, W, C)
NORM_CASES = [
    (3, 5, 7, 20),         # 35 tokens: a partial tile; C = 20: 5 of 16 lanes
    (1, 1, 1, 4),          # one token, one lane
    (2, 9, 7, 64),         # 63 tokens; NV 1, every lane
    (2, 5, 13, 68),        # 65 tokens: a tile of one; NV 2 with one lane in the second group
    (1, 8, 12, 192),       # NV 3; 64 x 196 and 192 x 65 floats: past 48 KiB of LDS, the attribute path
    (2, 4, 16, 256),       # NV 4, the widest
    (2, 362, 363, 4),      # 2 x 2054 = 4108 tiles against the 4096-workgroup cap: the tile loop
]


@functools.lru_cache(maxsize=2)
def _norm_inputs(case):
    b, h, w, c = case
    gen = torch.Generator(device="cpu").manual_seed(31 * c + h)
    rn = lambda *s: torch.randn(*s, generator=gen)
    f, l, x = 2 * rn(b, c, h, w) + 0.5, 2 * rn(b, c, h, w) + 0.5, 2 * rn(b, h, w, c) + 0.5
    return f, l, x, 1 + 0.2 * rn(c), 0.2 * rn(c), 0.2 * rn(c)             # ..., gamma, beta, sum_bias


def _check_merge(tag, s, n, f, l, x, gamma, beta, sb, want_norm, failures):
    """s, n: what the kernel stored (n None without want_norm)"""
    import torch.nn.functional as F

    want_s, want_n = R.merge(f, l, x, gamma, beta, EPS, sum_bias=sb)
    s32 = (f + l).permute(0, 2, 3, 1) + x                                # float32, the kernel's order
    stored32 = s32 + sb if sb is not None else s32
    assert s.shape == x.shape and s.is_contiguous()
    assert torch.equal(s.cpu(), stored32), f"{tag}: the stored sum is not (f + l) + x (+ sum_bias) in float32"
    _check(f"{tag} sum", s, want_s, stored32, failures, l2_floor=1e-6)
    if want_norm:
        assert n.shape == x.shape and n.is_contiguous() and not torch.isnan(n).any()
        _check(f"{tag} norm", n, want_n, F.layer_norm(s32, (x.shape[-1],), gamma, beta, EPS), failures, l2_floor=1e-6)
    else:
        assert n is None


@pytest.mark.parametrize("case", NORM_CASES, ids=C.case_id)
def test_afno_merge_matches_the_fp64_reference(case):
    from dlwp_benchmark_amd import ops

    f, l, x, gamma, beta, sb = _norm_inputs(case)
    dev = _dev()
    df, dl, dx, dg, dbt, dsb = (t.to(dev) for t in (f, l, x, gamma, beta, sb))
    failures = []
    for bias in (None, dsb):
        for want_norm in (True, False):
            s, n = ops.afno_merge(df, dl, dx, dg, dbt, EPS, sum_bias=bias, want_norm=want_norm)
            torch.cuda.synchronize()
            _check_merge(f"merge {C.case_id(case)} bias={bias is not None} norm={want_norm}", s, n, f, l, x, gamma, beta,
                         sb if bias is not None else None, want_norm, failures)
    assert not failures, failures


@pytest.mark.parametrize("case", NORM_CASES, ids=C.case_id)
def test_layernorm_nhwc_to_nchw_matches_the_fp64_reference(case):
    import torch.nn.functional as F

    from dlwp_benchmark_amd import ops

    _, _, x, gamma, beta, _ = _norm_inputs(case)
    b, h, w, c = case
    got = ops.layernorm_nhwc_to_nchw(x.to(_dev()), gamma.to(_dev()), beta.to(_dev()), EPS)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (b, c, h, w) and got.is_contiguous()
    failures = []
    _check(f"layernorm->nchw {C.case_id(case)}", got, R.layernorm_to_nchw(x, gamma, beta, EPS),
           F.layer_norm(x, (c,), gamma, beta, EPS).permute(0, 3, 1, 2), failures, l2_floor=1e-6)
    assert not failures, failures


def test_norm_kernels_write_every_element():
    """the two entry points launched directly into NaN-filled outputs (ops allocates with torch.empty): 35 tokens of 20 channels,
    a partial tile and partial lane groups"""
    import torch.nn.functional as F

    from dlwp_benchmark_amd import lib as L

    case = NORM_CASES[0]
    b, h, w, c = case
    f, l, x, gamma, beta, sb = _norm_inputs(case)
    dev = _dev()
    df, dl, dx, dg, dbt, dsb = (t.contiguous().to(dev) for t in (f, l, x, gamma, beta, sb))
    s, n = (torch.full((b, h, w, c), NAN, device=dev) for _ in range(2))
    L.launch("dlwp_afno_merge_f32", dev, df, dl, dx, dg, dbt, dsb, s, n, b, h * w, c, EPS)
    y = torch.full((b, c, h, w), NAN, device=dev)
    L.launch("dlwp_layernorm_nhwc_to_nchw_f32", dev, dx, dg, dbt, y, b, h * w, c, EPS)
    torch.cuda.synchronize()
    for name, t in (("sum", s), ("norm", n), ("layernorm->nchw", y)):
        assert not torch.isnan(t).any(), f"{name}: {int(torch.isnan(t).sum())} elements were never written"
    failures = []
    _check_merge("merge raw", s, n, f, l, x, gamma, beta, sb, True, failures)
    _check("layernorm->nchw raw", y, R.layernorm_to_nchw(x, gamma, beta, EPS), F.layer_norm(x, (c,), gamma, beta, EPS).permute(0, 3, 1, 2),
           failures, l2_floor=1e-6)
    assert not failures, failures
