"""float64 reference of the AFNO block's kernels (TEST INFRASTRUCTURE; plain torch, any device, no HIP).

* `mix` / `mix_backward`: what dlwp_afno2d_mix_f32 / dlwp_afno2d_mix_scaled_f32 / dlwp_afno2d_mix_bwd_f32 compute, written from
  the operator's definition (reference fourcastnet.py:87-121): per channel block a COMPLEX two-layer MLP
      z1 = xin W1 + b1,  o1 = relu(Re z1) + i relu(Im z1),  z2 = o1 W2 + b2,  y = softshrink(Re z2) + i softshrink(Im z2)
  on the kept modes (rows [total - kept, total + kept), columns [0, kept), total = H // 2 + 1, kept = int(total * fraction) --
  the column count comes from H, the reference's quirk), zeros elsewhere.  Complex einsums, no loop of the kernels, and no
  import of dlwp_benchmark_amd: ops.afno_kept_cols and training.afno_filter_torch are among the things this module checks.
* `merge` / `layernorm_to_nchw`: dlwp_afno_merge_f32 / dlwp_layernorm_nhwc_to_nchw_f32 (fourcastnet.py:127, :180-193).

dtype=torch.float32 evaluates the same formulas in single precision: on the CPU that is the "floor" the GPU tests scale
their tolerances by (what fp32 arithmetic itself costs on the inputs at hand).
"""
import torch
import torch.nn.functional as F


def kept_region(H, Wf, fraction):
    """(row_lo, row_hi, km): the kept rows [row_lo, row_hi) and columns [0, km) of an [H, Wf] half spectrum, in Python
    arithmetic (fourcastnet.py:93-96), clamped as slicing clamps."""
    total = H // 2 + 1
    kept = int(total * fraction)
    if kept < 1:
        return 0, 0, 0
    return max(total - kept, 0), min(total + kept, H), min(kept, Wf)


def _complex_dtype(dtype):
    return {torch.float64: torch.complex128, torch.float32: torch.complex64}[dtype]


def _weights(w1, b1, w2, b2, dtype):
    """[2, nb, bs(, bs)] real pairs -> complex [nb, bs(, bs)]"""
    return tuple(torch.complex(t[0].to(dtype), t[1].to(dtype)) for t in (w1, b1, w2, b2))


def _apply(a, w):
    """per-block vector-matrix product: a [B, nb, bs_in, R, K] times w [nb, bs_in, bs_out]"""
    return torch.einsum("bnirk,nio->bnork", a, w)


def _forward(xf, w1, b1, w2, b2, nb, lam, fraction, in_scale, dtype):
    b, c, h, wf = xf.shape
    bs = c // nb
    lo, hi, km = kept_region(h, wf, fraction)
    W1, B1, W2, B2 = _weights(w1, b1, w2, b2, dtype)
    xin = (xf.to(_complex_dtype(dtype)) * in_scale).view(b, nb, bs, h, wf)[:, :, :, lo:hi, :km]
    z1 = _apply(xin, W1) + B1[None, :, :, None, None]
    o1 = torch.complex(F.relu(z1.real), F.relu(z1.imag))
    z2 = _apply(o1, W2) + B2[None, :, :, None, None]
    return (lo, hi, km), (W1, W2), xin, z1, o1, z2


def _full(t, region, shape):
    """a kept-region tensor [B, nb, bs, R, K] zero-padded to the full spectrum [B, C, H, Wf]"""
    lo, hi, km = region
    b, c, h, wf = shape
    out = torch.zeros(b, t.shape[1], t.shape[2], h, wf, dtype=t.dtype, device=t.device)
    out[:, :, :, lo:hi, :km] = t
    return out.view(b, c, h, wf)


def mix(xf, w1, b1, w2, b2, nb, lam, fraction, in_scale=1.0, out_scale=1.0, dtype=torch.float64):
    """xf complex [B, C, H, Wf] channels-first -> (y, pre).  y: the full output spectrum out_scale * mlp(in_scale * xf), zeros
    outside the kept region.  pre = (Re z1, Im z1, Re z2, Im z2) over the kept region only, each [B, nb, bs, rows, km]: the values
    the ReLU and the softshrink decide on.  Differentiable."""
    region, _, _, z1, _, z2 = _forward(xf, w1, b1, w2, b2, nb, lam, fraction, in_scale, dtype)
    y = torch.complex(F.softshrink(z2.real, lam), F.softshrink(z2.imag, lam)) * out_scale
    return _full(y, region, xf.shape), (z1.real, z1.imag, z2.real, z2.imag)


def mix_backward(xf, gf, w1, b1, w2, b2, nb, lam, fraction, width, in_scale=1.0, out_scale=1.0, dtype=torch.float64):
    """The outputs of dlwp_afno2d_mix_bwd_f32, each complex [B, C, H, Wf] and zero outside the kept region: (gx, xin, o1, d1, d2)
    for xf = R2C(x), gf = R2C(grad_y) with UNNORMALISED transforms of a field `width` points wide:
        d2 = out_scale c_k gf where |z2| > lam (re / im apart),  d1 = (d2 W2^H) where z1 > 0 (re / im apart),
        gx = in_scale (d1 W1^H) / c_k,        c_k = 1 on the self-conjugate columns (0, and width / 2 for even width), else 2.
    C2R(gx) is the gradient of the field; the weight gradients are sums over points of conj(xin) (x) d1 and conj(o1) (x) d2."""
    b, c, h, wf = xf.shape
    bs = c // nb
    region, (W1, W2), xin, z1, o1, z2 = _forward(xf, w1, b1, w2, b2, nb, lam, fraction, in_scale, dtype)
    lo, hi, km = region
    ck = torch.full((wf,), 2.0, dtype=dtype, device=xf.device)
    ck[0] = 1.0
    if width % 2 == 0 and width // 2 < wf:
        ck[width // 2] = 1.0
    ck = ck[:km]
    gz = gf.to(_complex_dtype(dtype)).view(b, nb, bs, h, wf)[:, :, :, lo:hi, :km] * (out_scale * ck)
    d2 = torch.complex(gz.real * (z2.real.abs() > lam), gz.imag * (z2.imag.abs() > lam))
    t = torch.einsum("bnork,nio->bnirk", d2, W2.conj())
    d1 = torch.complex(t.real * (z1.real > 0), t.imag * (z1.imag > 0))
    gx = torch.einsum("bnork,nio->bnirk", d1, W1.conj()) * (in_scale / ck)
    return tuple(_full(t, region, xf.shape) for t in (gx, xin, o1, d1, d2))


def near_threshold(pre, lam, margin):
    """bool [B, nb, rows, km]: a (point, block) where one of the block's 2 bs layer-1 pre-activations lies within `margin` of 0
    (the ReLU's kink) or one of its 2 bs layer-2 values has ||v| - lam| < margin (the softshrink's): there a gradient computed in
    another precision may legitimately take the other branch."""
    z1r, z1i, z2r, z2i = pre
    hit = (z1r.abs() < margin) | (z1i.abs() < margin) | ((z2r.abs() - lam).abs() < margin) | ((z2i.abs() - lam).abs() < margin)
    return hit.any(dim=2)


def _layer_norm(s, gamma, beta, eps):
    mean = s.mean(dim=-1, keepdim=True)
    var = ((s - mean) ** 2).mean(dim=-1, keepdim=True)
    return (s - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def merge(f, l, x, gamma, beta, eps, sum_bias=None):
    """f, l [B, C, H, W], x [B, H, W, C] -> (stored sum, LayerNorm(sum)) in float64, both [B, H, W, C].  sum = f + l + x;
    sum_bias is added to the STORED sum only, not to the LayerNorm input.  gamma None -> (stored sum, None)."""
    s = (f.double() + l.double()).permute(0, 2, 3, 1) + x.double()
    n = _layer_norm(s, gamma, beta, eps) if gamma is not None else None
    return (s + sum_bias.double() if sum_bias is not None else s), n


def layernorm_to_nchw(x, gamma, beta, eps):
    """x [B, H, W, C] -> LayerNorm over C, channels-first [B, C, H, W], float64"""
    return _layer_norm(x.double(), gamma, beta, eps).permute(0, 3, 1, 2).contiguous()
