"""The float64 AFNO reference (tests/afno_ref.py) proved without a GPU, and the case tables / inputs of the GPU tests
(tests/test_afno_mix_fp64_gpu.py):

* forward: irfft2(mix(rfft2(x))) + x in float32 equals oracle.restate.afno.afno2d, which real-reference fixtures pin;
* backward: mix_backward's five outputs, pushed through the transform and the four einsums ops.afno2d_filter_backward forms,
  equal float64 autograd of the float64 filter -- this establishes the c_k convention (1 on the self-conjugate columns) with
  no kernel involved;
* the kept-mode count: kept_region, ops.afno_kept_cols and the slice of training.afno_filter_torch agree, at grids where
  float(fraction) * total falls below an integer that double(fraction) * total reaches;
* the inputs of every backward case keep the share of (point, block) entries near a ReLU / softshrink threshold under 2 %.
"""
import ctypes
import functools

import pytest
import torch

import afno_ref as R
from helpers import rel_l2

LAM = 0.01          # sparsity_threshold of every case
MARGIN = 1e-4       # near_threshold margin of the backward comparisons
CAP = 0.02          # largest share of flagged (b, block, row, col) entries a backward case may have

# (B, C, nb, H, W, fraction, layout).  "full": Wf = W / 2 + 1, spectrum rfft2(x, norm="ortho"), scales 1.
# "kept": Wf = the kept columns, unnormalised spectrum, scales 1 / sqrt(H W) (what ops.afno2d_filter_cf runs, in place).
FWD_CASES = [
    # bs 4
    (2, 16, 4, 12, 20, 1.0, "full"),
    (1, 8, 2, 18, 20, 0.7, "full"),           # 10 * 0.7 = 7 in double, 6.99.. with a float fraction
    (8, 4, 1, 512, 512, 1.0, "kept"),         # 1 052 672 points > 4096 x 256 threads: the grid-stride loop
    # bs 8
    (2, 16, 2, 32, 64, 0.5, "full"),
    (2, 16, 2, 32, 64, 0.5, "kept"),
    (3, 24, 3, 21, 30, 1.0, "full"),          # odd H
    # bs 32
    (1, 64, 2, 20, 30, 1.0, "full"),
    (2, 32, 1, 64, 32, 1.0, "full"),          # kept 33 clamped to Wf 17
    # bs 16: the MFMA form
    (2, 32, 2, 12, 20, 1.0, "full"),          # plane of 132 points: ragged last tile; two of four waves have a block
    (1, 128, 8, 16, 32, 0.5, "full"),         # two blocks per wave; Wf 17: tiles straddle rows
    (2, 16, 1, 128, 256, 1.0, "full"),        # 2064 tiles > 2048 workgroups: the prefetching stride loop
    (1, 16, 1, 18, 20, 0.7, "full"),          # the float-fraction case again
    (2, 64, 4, 32, 64, 0.5, "kept"),
]
# dlwp_afno2d_mix_bwd_f32 on random complex xf, gf; same tuple
BWD_CASES = [
    (2, 16, 4, 12, 20, 1.0, "full"),          # bs 4
    (2, 16, 2, 32, 32, 1.0, "full"),          # bs 8; the Nyquist column 16 is kept
    (2, 16, 2, 32, 64, 0.5, "full"),          # bs 8; Nyquist column dropped
    (1, 16, 1, 12, 21, 1.0, "full"),          # bs 16; odd width: no Nyquist column
    (8, 4, 1, 512, 512, 1.0, "kept"),         # bs 4; 1 052 672 points: the grid cap
    (1, 8, 2, 18, 20, 0.7, "full"),           # bs 4; the float-fraction grid: this entry point derives the count itself
]
# ops.afno2d_filter_backward: (B, C, nb, H, W, fraction)
FILTER_BWD_CASES = [(2, 16, 2, 32, 64, 0.5), (2, 16, 4, 32, 32, 1.0), (2, 32, 2, 64, 64, 0.7)]
# seeds of the backward inputs; a case that exceeds CAP gets another seed here, never another cap or margin
SEEDS = {}


def case_id(case):
    return "x".join(str(v) for v in case)


def _seed(kind, case):
    return SEEDS.get((kind, case), 7919 * (1 + "fwd bwd filter".split().index(kind)) + sum(int(100 * v) * (i + 1) for i, v in enumerate(case[:6])))


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def weights(gen, nb, bs):
    w1, w2 = (0.3 * _randn(gen, 2, nb, bs, bs) for _ in range(2))
    b1, b2 = (0.3 * _randn(gen, 2, nb, bs) for _ in range(2))
    return w1, b1, w2, b2


def scales(case):
    _, _, _, h, w, _, layout = case
    s = 1.0 / float(h * w) ** 0.5 if layout == "kept" else 1.0
    return s, s


def spectrum_width(case):
    _, _, _, h, w, frac, layout = case
    return R.kept_region(h, w // 2 + 1, frac)[2] if layout == "kept" else w // 2 + 1


@functools.lru_cache(maxsize=2)
def forward_inputs(case):
    """(xf complex64 [B, C, H, Wf] contiguous, w1, b1, w2, b2), CPU"""
    b, c, nb, h, w, frac, layout = case
    gen = torch.Generator(device="cpu").manual_seed(_seed("fwd", case))
    x = _randn(gen, b, c, h, w)
    wts = weights(gen, nb, c // nb)
    xf = torch.fft.rfft2(x, norm="ortho") if layout == "full" else torch.fft.rfft2(x)[..., :spectrum_width(case)]
    return (xf.contiguous(), *wts)


@functools.lru_cache(maxsize=2)
def backward_inputs(case):
    """(xf, gf complex64 [B, C, H, Wf], w1, b1, w2, b2), CPU; random complex spectra of the magnitude the layout's transform gives"""
    b, c, nb, h, w, frac, layout = case
    gen = torch.Generator(device="cpu").manual_seed(_seed("bwd", case))
    wf = spectrum_width(case)
    amp = float(h * w) ** 0.5 if layout == "kept" else 1.0
    xf = torch.complex(_randn(gen, b, c, h, wf), _randn(gen, b, c, h, wf)) * (amp * 0.5 ** 0.5)
    gf = torch.complex(_randn(gen, b, c, h, wf), _randn(gen, b, c, h, wf)) * (amp * 0.5 ** 0.5)
    return (xf, gf, *weights(gen, nb, c // nb))


@functools.lru_cache(maxsize=None)
def filter_inputs(case):
    """(x, gy [B, C, H, W], w1, b1, w2, b2), CPU float32"""
    b, c, nb, h, w, frac = case
    gen = torch.Generator(device="cpu").manual_seed(_seed("filter", case))
    x = _randn(gen, b, c, h, w)
    wts = weights(gen, nb, c // nb)
    return (x, _randn(gen, b, c, h, w), *wts)


def filter64(x, w1, b1, w2, b2, nb, frac):
    """the float64 filter irfft2(mix(rfft2(x, "ortho")), "ortho") of a channels-first field, and mix's pre-activations"""
    h, w = x.shape[-2:]
    y, pre = R.mix(torch.fft.rfft2(x.double(), norm="ortho"), w1, b1, w2, b2, nb, LAM, frac)
    return torch.fft.irfft2(y, s=(h, w), norm="ortho"), pre


def flagged_share(mask):
    return float(mask.double().mean())


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,h,w,c,nb,frac", [(2, 12, 20, 16, 4, 1.0), (1, 18, 20, 16, 2, 0.7), (1, 21, 30, 24, 3, 0.5)])
def test_forward_matches_the_fixture_pinned_restatement(b, h, w, c, nb, frac):
    from oracle.restate.afno import afno2d

    gen = torch.Generator(device="cpu").manual_seed(11 + h)
    x = _randn(gen, b, h, w, c)                                         # token-major, as the restatement takes it
    w1, b1, w2, b2 = weights(gen, nb, c // nb)
    want = afno2d(x, w1, b1, w2, b2, nb, LAM, frac)
    x_cf = x.permute(0, 3, 1, 2).contiguous()
    y, _ = R.mix(torch.fft.rfft2(x_cf, norm="ortho"), w1, b1, w2, b2, nb, LAM, frac, dtype=torch.float32)
    assert y.dtype == torch.complex64
    got = (torch.fft.irfft2(y, s=(h, w), norm="ortho") + x_cf).permute(0, 2, 3, 1)
    e = rel_l2(got, want)
    print(f"rel-L2 {e:.2e}")
    assert got.shape == want.shape and e <= 1e-6, e
    # the filter must matter for this to mean anything: without it the output would be x
    assert rel_l2(x, want) > 0.1


# (B, C, nb, H, W, fraction): even width with the Nyquist column kept / dropped, odd width
@pytest.mark.parametrize("case", [(2, 8, 2, 12, 12, 1.0), (2, 8, 2, 12, 20, 1.0), (2, 12, 3, 12, 21, 0.7), (1, 16, 1, 18, 20, 0.7)],
                         ids=case_id)
def test_backward_matches_float64_autograd(case):
    """kept layout, unnormalised transforms and scales 1 / sqrt(H W): exactly what ops.afno2d_filter_backward feeds the kernel"""
    b, c, nb, h, w, frac = case
    bs = c // nb
    gen = torch.Generator(device="cpu").manual_seed(3 + w)
    x, gy = _randn(gen, b, c, h, w).double(), _randn(gen, b, c, h, w).double()
    wts = [t.double() for t in weights(gen, nb, bs)]
    ins = [t.clone().requires_grad_(True) for t in (x, *wts)]
    out, _ = filter64(*ins, nb, frac)
    want = torch.autograd.grad(out, ins, gy)

    lo, hi, km = R.kept_region(h, w // 2 + 1, frac)
    assert (w % 2 == 0 and w // 2 < km) == (case == (2, 8, 2, 12, 12, 1.0)), "which case keeps the Nyquist column"
    s = 1.0 / float(h * w) ** 0.5
    xf, gf = torch.fft.rfft2(x)[..., :km], torch.fft.rfft2(gy)[..., :km]
    gx, xin, o1, d1, d2 = R.mix_backward(xf, gf, *wts, nb, LAM, frac, w, in_scale=s, out_scale=s)
    pad = torch.zeros(b, c, h, w // 2 + 1, dtype=torch.complex128)
    pad[..., :km] = gx
    dx = torch.fft.irfft2(pad, s=(h, w)) * (h * w)                       # the unnormalised C2R
    got = (dx, *weight_gradients(xin, o1, d1, d2, nb))
    for name, a, g in zip(("dx", "dw1", "db1", "dw2", "db2"), got, want):
        e = rel_l2(a, g)
        print(f"{name} {e:.2e}")
        assert a.shape == g.shape and e <= 1e-10, (name, e)


def weight_gradients(xin, o1, d1, d2, nb, keep=None):
    """(dw1, db1, dw2, db2) in the reference layout [2, nb, bs(, bs)], float64, from the backward kernel's factors: the four sums
    ops.afno2d_filter_backward forms.  keep: optional bool [B, nb, H, Wf]; entries outside it are left out of the sums."""
    b, c, h, wf = xin.shape
    cv = lambda t: t.to(torch.complex128).view(b, nb, c // nb, h, wf)
    xin, o1, d1, d2 = cv(xin), cv(o1), cv(d1), cv(d2)
    if keep is not None:
        d1, d2 = d1 * keep[:, :, None], d2 * keep[:, :, None]
    gw1 = torch.einsum("bnihk,bnohk->nio", xin.conj(), d1)
    gw2 = torch.einsum("bnihk,bnohk->nio", o1.conj(), d2)
    gb1, gb2 = d1.sum(dim=(0, 3, 4)), d2.sum(dim=(0, 3, 4))
    ri = lambda t: torch.stack([t.real, t.imag], dim=0)
    return ri(gw1), ri(gb1), ri(gw2), ri(gb2)


# ---------------------------------------------------------------------------------------------------------------------
# (H, fraction, kept): the last column is written out by hand (total = H // 2 + 1, kept = int(total * fraction) in doubles)
KEPT_TABLE = [(18, 0.7, 7), (19, 0.7, 7), (18, 0.9, 9), (19, 0.9, 9), (38, 0.7, 14), (58, 0.7, 21), (32, 1.0, 17), (32, 0.5, 8),
              (32, 0.7, 11), (64, 1.0, 33), (64, 0.7, 23), (64, 0.5, 16), (128, 1.0, 65), (128, 0.5, 32), (128, 0.3, 19),
              (21, 0.5, 5), (12, 0.2, 1)]
# the entries where total * float(fraction) stays below the integer total * fraction reaches: a float parameter loses a mode
FLOAT_LOSES_A_MODE = {(18, 0.7), (19, 0.7), (18, 0.9), (19, 0.9), (38, 0.7), (58, 0.7)}


@pytest.mark.parametrize("h,frac,kept", KEPT_TABLE)
def test_kept_count_rule(h, frac, kept):
    from dlwp_benchmark_amd import ops, training

    total = h // 2 + 1
    w = 2 * h + 2                                                        # Wf = h + 2 > kept: nothing is clamped along W
    wf = w // 2 + 1
    lo, hi, km = R.kept_region(h, wf, frac)
    assert (lo, hi, km) == (total - kept, min(total + kept, h), kept)
    assert ops.afno_kept_cols(h, w, frac) == kept
    assert R.kept_region(h, 3, frac)[2] == min(kept, 3) == ops.afno_kept_cols(h, 4, frac)        # clamped to Wf
    # what a C `float` parameter makes of the same fraction (the defect this table is for)
    as_float = int(float(total) * ctypes.c_float(frac).value)
    assert as_float == (kept - 1 if (h, frac) in FLOAT_LOSES_A_MODE else kept)
    # the slice training.afno_filter_torch cuts: with zero weights and b2 = 1 the output spectrum is softshrink(1) on the kept
    # modes and 0 elsewhere; the C2R symmetrises column 0 over rows, so rows are read off column 1 and columns off row total - 1
    z = lambda *s: torch.zeros(*s)
    b2 = z(2, 1, 1)
    b2[0] = 1.0
    out = training.afno_filter_torch(z(1, 1, h, w), z(2, 1, 1, 1), z(2, 1, 1), z(2, 1, 1, 1), b2, 1, LAM, frac)
    on = torch.fft.rfft2(out.double(), norm="ortho")[0, 0].abs() > 1e-3
    assert on[total - 1].nonzero().flatten().tolist() == list(range(km))
    if km >= 2:
        assert on[:, 1].nonzero().flatten().tolist() == list(range(lo, hi))
    # and the reference itself on the same table
    y, _ = R.mix(torch.zeros(1, 1, h, wf, dtype=torch.complex128), z(2, 1, 1, 1), z(2, 1, 1), z(2, 1, 1, 1), b2, 1, LAM, frac)
    want_on = torch.zeros(h, wf, dtype=torch.bool)
    want_on[lo:hi, :km] = True
    assert torch.equal(y[0, 0].abs() > 1e-3, want_on)


def test_fraction_crosses_the_c_abi_as_double():
    """hard_thresholding_fraction of the three mixing entry points (the parameter after sparsity_threshold)"""
    from dlwp_benchmark_amd import lib as L

    for name, pos in (("dlwp_afno2d_mix_f32", 12), ("dlwp_afno2d_mix_scaled_f32", 12), ("dlwp_afno2d_mix_bwd_f32", 18)):
        args = L.SIGNATURES[name][1]
        assert args[pos - 1] is ctypes.c_float and args[pos] is ctypes.c_double, name


# ---------------------------------------------------------------------------------------------------------------------
def bwd_flags(case):
    """near_threshold of a kernel-level backward case: bool [B, nb, rows, km] over the kept region"""
    b, c, nb, h, w, frac, layout = case
    xf, gf, *wts = backward_inputs(case)
    si, so = scales(case)
    _, pre = R.mix(xf, *wts, nb, LAM, frac, in_scale=si, out_scale=so)
    return R.near_threshold(pre, LAM, MARGIN)


def filter_flags(case):
    b, c, nb, h, w, frac = case
    x, gy, *wts = filter_inputs(case)
    _, pre = filter64(x, *wts, nb, frac)
    return R.near_threshold(pre, LAM, MARGIN)


@pytest.mark.parametrize("case", BWD_CASES + FILTER_BWD_CASES, ids=case_id)
def test_backward_inputs_keep_clear_of_the_thresholds(case):
    """a condition on the INPUTS (asserted again where the GPU tests use the mask): too large a share of excluded entries would
    hollow out the comparison.  A case that exceeds the cap gets another seed (SEEDS)."""
    flags = bwd_flags(case) if len(case) == 7 else filter_flags(case)
    share = flagged_share(flags)
    print(f"{case_id(case)}: {100 * share:.2f} % of {flags.numel()} (point, block) entries within {MARGIN} of a threshold")
    assert flags.numel() > 0 and share <= CAP, share
