"""float64 reference of the window-attention operator (TEST INFRASTRUCTURE; plain torch on the CPU).

What dlwp_window_attn_f32 / dlwp_window_attn_bf16 take -- qkv [B, L, 3 heads d] as the qkv Linear wrote it, the qkv bias, the
bias table -- goes through the reference's own sequence of pad / roll / window_partition / attention / window_reverse / roll /
crop, built from the geometry helpers of oracle/restate/swin.py and oracle/restate/pangu.py (pinned to fixtures the real
reference classes produced).  Nothing here comes from the product: no descriptor, no index arithmetic of the kernels, and
no import of dlwp_benchmark_amd (training.window_attention_torch is one of the things this module checks).

operands="bf16" is this reference's own model of what bfloat16 MFMA operands cost: the scaled q, k, v and the un-normalised
probabilities exp(s - max) that enter `@ v` are rounded to bfloat16, everything else (accumulation, bias, mask, maximum, row
sum, normalisation) stays float64.
"""
import torch
import torch.nn.functional as F

from oracle.restate import pangu as _pangu
from oracle.restate import swin as _swin


def _round(t, operands):
    if operands == "fp64":
        return t
    if operands != "bf16":
        raise ValueError(f"unknown operands {operands!r}")
    return t.to(torch.bfloat16).to(torch.float64)


def _attend(q, k, v, add, operands):
    """softmax(q k^T + add) v over the last two dims; q already scaled.  add broadcasts against [..., N, N]."""
    q, k, v = _round(q, operands), _round(k, operands), _round(v, operands)
    s = q @ k.transpose(-2, -1) + add
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    return (_round(p, operands) @ v) / p.sum(dim=-1, keepdim=True)


def ref_swin(qkv, table, h, w, win, shift, heads, d, operands="fp64"):
    """swin_transformer.py:217-251 + :122-154 between the qkv and the proj Linear.  qkv [B, h w, 3 heads d], table
    [(2 wh - 1)(2 ww - 1), heads], win = (wh, ww) dividing (h, w), shift = (sh, sw) or (0, 0) -> [B, h w, heads d] float64."""
    b = qkv.shape[0]
    c = heads * d
    wh, ww = win
    n = wh * ww
    shifted = shift[0] > 0 or shift[1] > 0
    x = qkv.double().view(b, h, w, 3 * c)
    if shifted:
        x = torch.roll(x, shifts=(-shift[0], -shift[1]), dims=(1, 2))
    xw = _swin.window_partition(x, win).view(-1, n, 3, heads, d).permute(2, 0, 3, 1, 4)        # [3, B nW, heads, N, d]
    q, k, v = xw[0] * d ** -0.5, xw[1], xw[2]
    idx = _swin.relative_position_index(wh, ww)
    add = table.double()[idx.view(-1)].view(n, n, heads).permute(2, 0, 1).unsqueeze(0)         # [1, heads, N, N]
    if shifted:
        mask = _swin.shift_mask(h, w, win, shift).double()                                      # [nW, N, N]
        nw = mask.shape[0]
        add = (add.unsqueeze(0) + mask.view(1, nw, 1, n, n)).expand(b, nw, heads, n, n).reshape(b * nw, heads, n, n)
    o = _attend(q, k, v, add, operands).transpose(1, 2).reshape(-1, wh, ww, c)
    x = _swin.window_reverse(o, win, h, w)
    if shifted:
        x = torch.roll(x, shifts=(shift[0], shift[1]), dims=(1, 2))
    return x.reshape(b, h * w, c)


def ref_pangu(qkv, bias, table, grid, win, shift, heads, d, operands="fp64"):
    """panguweather.py:285-316 + :176-211 between the qkv and the proj Linear.  qkv [B, pl lat lon, 3 heads d], bias [3 heads d]
    (the zero-padded tokens enter the qkv Linear as zeros, so they leave it as the bias), table [rows, types, heads],
    shift = (spl, slat, slon); the block rolls only when all three are non-zero -> [B, pl lat lon, heads d] float64."""
    b = qkv.shape[0]
    c = heads * d
    pl, lat, lon = grid
    wpl, wlat, wlon = win
    n = wpl * wlat * wlon
    bias = bias.double()
    x = qkv.double().view(b, pl, lat, lon, 3 * c)
    pad = _pangu.get_pad3d(grid, win)
    x = F.pad((x - bias).permute(0, 4, 1, 2, 3), pad).permute(0, 2, 3, 4, 1) + bias
    _, plp, latp, lonp, _ = x.shape
    roll = bool(shift[0] and shift[1] and shift[2])
    types = (plp // wpl) * (latp // wlat)
    if roll:
        x = torch.roll(x, shifts=(-shift[0], -shift[1], -shift[1]), dims=(1, 2, 3))           # [sic] panguweather.py:291
    xw = _pangu.window_partition(x.contiguous(), win)                                          # [B nLon, nW, wpl, wlat, wlon, 3C]
    b_, nw_ = xw.shape[0], xw.shape[1]
    xw = xw.view(b_, nw_, n, 3, heads, d).permute(3, 0, 4, 1, 2, 5)                            # [3, B nLon, heads, nW, N, d]
    q, k, v = xw[0] * d ** -0.5, xw[1], xw[2]
    idx = _pangu.earth_position_index(win)
    add = table.double()[idx.view(-1)].view(n, n, types, heads).permute(3, 2, 0, 1).unsqueeze(0)   # [1, heads, nW, N, N]
    if roll:
        mask = _pangu.shift_window_mask((plp, latp, lonp), win, shift).double()                # [nLon, nW, N, N]
        nlon = mask.shape[0]
        add = (add.unsqueeze(0) + mask.view(1, nlon, 1, nw_, n, n)).expand(b, nlon, heads, nw_, n, n)
        add = add.reshape(b_, heads, nw_, n, n)
    o = _attend(q, k, v, add, operands).permute(0, 2, 3, 1, 4).reshape(b_, nw_, wpl, wlat, wlon, c)
    x = _pangu.window_reverse(o, win, plp, latp, lonp)
    if roll:
        x = torch.roll(x, shifts=tuple(shift), dims=(1, 2, 3))                                 # panguweather.py:310
    fr, to_, le = pad[4], pad[2], pad[0]
    x = x[:, fr:fr + pl, to_:to_ + lat, le:le + lon]
    return x.reshape(b, pl * lat * lon, c)
