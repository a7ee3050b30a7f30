"""linear_ring_kernel (csrc/linear.hip) at the row counts that select it.

The ring kernel only runs on large bf16-x calls -- the Pangu Linears of C5 at the benchmark's batch (M = 262 144 in layer 1,
65 536 in layer 2) -- while every other test stays below the threshold on linear_kernel.  Each case here runs the full-M call
on the ring kernel and checks it three ways:
  * bitwise against the same call cut into row slices small enough to run on linear_kernel ("bit-identical
    to linear_kernel (same products, same order)"), over every output element;
  * against F.linear of the bf16-rounded operands in float64, on a row sample that holds the first and the last 256-row tile
    and every tail row (the bound of test_linear_bf16_matches_bf16_rounded_operands);
  * with guard rows around `out`: rows before and after the view are bitwise untouched (the stores are clipped by the buffer
    descriptor's range check, not by branches).
The selection rule is restated in ring_selected() / ring_instance(); a CPU test asserts that every case is in the regime it
claims and that the cases reach every instance the dispatcher can pick."""
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_l2

DEV = "cuda:0"


def ring_selected(M, K, N, x_bf16, out_bf16):
    """lin::launch() (csrc/linear.hip): the ring kernel takes a bf16-x call (form 4: bf16 x, fp32 out; form 6: bf16 x and out)
    when K % 64 == 0, K >= 3 * 64, (form 4 or N % 8 == 0) and its 256 x 128 tiles fill the chip:
    ceil(M/256) * ceil(N/128) >= 1024, or >= 512 with K >= 768 (DLWP_LINEAR_RING / DLWP_LINEAR_RING_MIN_TILES unset)."""
    if not x_bf16:
        return False
    tiles = ((M + 255) // 256) * ((N + 127) // 128)
    fill = tiles >= 1024 or (2 * tiles >= 1024 and K >= 768)
    return K % 64 == 0 and K >= 3 * 64 and (not out_bf16 or N % 8 == 0) and fill


def ring_instance(N, out_bf16, resid):
    """the template arguments lin::launch() gives linear_ring_kernel<BN, OB16, S, RES>: BN = 96 where a 128-wide last tile
    would waste a quarter or more (narrow_r), OB16 = bf16 output, RES = residual operand (S = 3 stages)."""
    narrow = N % 128 != 0 and N % 128 <= 96 and (N % 96 == 0 or N < 128)
    return (96 if narrow else 128, bool(out_bf16), bool(resid))


L1, L2 = 262144, 65536      # C5 token rows at batch 8: 8 x 8 x 128 x 256 (layer 1), 8 x 8 x 64 x 128 (layer 2)

# name -> (M, K, N, act, bias, out_bf16, resid, ring expected)
CASES = {
    # the Pangu block's Linears in C5's bf16 form (models/pangu.py: LayerNorm / attention / fc1 hand over bf16 tensors)
    "l1_qkv": (L1, 192, 576, 0, True, True, False, True),
    "l1_fc1": (L1, 192, 768, 1, True, True, False, True),
    "l1_fc2": (L1, 768, 192, 0, True, False, True, True),
    "l1_proj": (L1, 192, 192, 0, True, False, True, True),
    "l2_qkv": (L2, 384, 1152, 0, True, True, False, True),
    "l2_fc1": (L2, 384, 1536, 1, True, True, False, True),
    "l2_fc2": (L2, 1536, 384, 0, True, False, True, True),       # 768 tiles: ring through the K >= 768 clause only
    "l2_proj": (L2, 384, 384, 0, True, False, True, False),      # 768 tiles, K = 384: stays on linear_kernel
    # shapes the model never produces
    "ragged_m_bn128_ob16": (L2 + 77, 384, 1152, 1, True, True, False, True),
    "ragged_n_bn128_resid": (L2 + 77, 384, 1000, 0, False, False, True, True),   # last tile 104 of 128 columns
    "ragged_n_bn96_ob16": (L1 + 77, 192, 88, 1, True, True, False, True),        # one tile, 88 of 96 columns
    "ragged_n_bn96_resid": (L1 + 77, 192, 40, 0, False, False, True, True),
    "bn96_plain": (L1 + 5, 192, 96, 0, False, False, False, True),
    "bn128_plain": (L2 + 77, 768, 640, 1, True, False, False, True),
    "k768_clause": (40000 + 13, 768, 768, 1, True, True, False, True),          # 942 tiles
}


def _slice_rows(N):
    """row slices in multiples of 256 (16-byte aligned views) with fewer than 512 tiles: linear_kernel, never the ring"""
    return 256 * max(1, 511 // ((N + 127) // 128))


def test_ring_cases_cover_every_instance():
    seen = set()
    for name, (M, K, N, act, bias, ob16, resid, ring) in CASES.items():
        assert ring_selected(M, K, N, True, ob16) == ring, name
        assert not ring_selected(_slice_rows(N), K, N, True, ob16), name
        assert not (ob16 and resid), name           # a bf16 output takes no residual (dlwp_linear_bf16_io)
        if ring:
            seen.add(ring_instance(N, ob16, resid))
            if ob16:
                seen.add(ring_instance(N, False, False))     # the fp32-output twin each bf16-output case runs
    assert {bn for bn, _, _ in seen} == {96, 128}
    assert {(bn, res) for bn, _, res in seen} == {(96, False), (96, True), (128, False), (128, True)}
    assert {ob for _, ob, _ in seen} == {False, True}
    assert seen == {(bn, ob, res) for bn in (96, 128) for ob, res in ((True, False), (False, False), (False, True))}
    assert any(ring and ((M + 255) // 256) * ((N + 127) // 128) < 1024 for M, K, N, *_, ring in CASES.values())
    assert any(M % 256 for M, *_ in CASES.values())


def _linear(k, n, bias, seed):
    torch.manual_seed(seed)
    m = torch.nn.Linear(k, n, bias=bias)
    with torch.no_grad():
        m.weight.mul_(3.0)
    return m.to(DEV)


HEAD, TAIL = 64, 300        # guard rows before / after the output (TAIL > 255: past any row a clipped last tile could reach)


def _guarded(M, N, dtype, fill=None):
    """a [HEAD + M + TAIL, N] buffer with sentinel rows around the [M, N] view the kernel writes"""
    buf = torch.full((HEAD + M + TAIL, N), -7.25, dtype=dtype, device=DEV)
    buf[:HEAD].view(torch.int16 if dtype == torch.bfloat16 else torch.int32).fill_(0x7FC1 if dtype == torch.bfloat16 else 0x7FC0DEAD)
    view = buf[HEAD:HEAD + M]
    if fill is not None:
        view.copy_(fill)
    guards = torch.cat([buf[:HEAD], buf[HEAD + M:]]).clone()
    return buf, view, guards


def _guards_intact(buf, M, guards):
    now = torch.cat([buf[:HEAD], buf[HEAD + M:]])
    it = torch.int16 if buf.dtype == torch.bfloat16 else torch.int32
    return torch.equal(now.view(it), guards.view(it))


def _sample_rows(M, g):
    """the first and last 256-row tile, every row of a partial last tile, and a random sample"""
    last = (M - 1) // 256 * 256
    rows = torch.cat([torch.arange(0, 256), torch.arange(last, M), torch.arange(max(0, last - 256), last),
                      torch.randint(0, M, (4096,), generator=g)])
    return torch.unique(rows).to(DEV)


def _want64(x, m, rows, act, resid):
    w = m.weight.bfloat16().double()
    want = F.linear(x[rows].double(), w, m.bias.double() if m.bias is not None else None)
    if act:
        want = F.gelu(want)
    if resid is not None:
        want = want + resid[rows].double()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_ring_linear_matches_linear_kernel_and_float64(name):
    from dlwp_benchmark_amd import ops

    for var in ("DLWP_LINEAR_RING", "DLWP_LINEAR_RING_MIN_TILES"):
        assert var not in os.environ, f"{var} changes the dispatch these cases are chosen for"
    M, K, N, act, bias, ob16, has_resid, ring = CASES[name]
    odt = torch.bfloat16 if ob16 else torch.float32
    m = _linear(K, N, bias, seed=K + N)
    g = torch.Generator(device=DEV).manual_seed(M + K + N)
    x = (torch.randn(M, K, device=DEV, generator=g) * 2.0 + 0.3).bfloat16()
    resid = torch.randn(M, N, device=DEV, generator=g) if has_resid else None

    with torch.no_grad():
        # the full call; a residual is added in place (out = resid, as the blocks do), into a guarded buffer either way
        buf, out, guards = _guarded(M, N, odt, fill=resid)
        got = ops.linear(x, m, act=act, resid=out if has_resid else None, out=out, precision="bf16")
        assert got.data_ptr() == out.data_ptr()
        torch.cuda.synchronize()
        assert _guards_intact(buf, M, guards), f"{name}: rows outside the output were written"

        # the same operation in row slices on linear_kernel: every element bitwise equal
        step = _slice_rows(N)
        parts = [ops.linear(x[a:a + step], m, act=act, resid=resid[a:a + step] if has_resid else None, precision="bf16",
                            out_dtype=odt) for a in range(0, M, step)]
        sliced = torch.cat(parts)
        diff = (got.float() != sliced.float()).sum().item()
        assert diff == 0, f"{name}: {diff} of {M * N} elements differ from linear_kernel"

        # float64 on a row sample
        rows = _sample_rows(M, torch.Generator().manual_seed(M))
        want = _want64(x, m, rows, act, resid)
        if ob16:
            # the bf16 output is the fp32 result rounded to nearest even: the fp32-output twin of the call (same instance
            # but OB16 = false) holds the fp32 bound, and rounds to the same bits
            buf32, out32, guards32 = _guarded(M, N, torch.float32)
            got32 = ops.linear(x, m, act=act, out=out32, precision="bf16")
            torch.cuda.synchronize()
            assert _guards_intact(buf32, M, guards32), f"{name}: rows outside the fp32 output were written"
            assert torch.equal(got, got32.bfloat16()), name
            err = rel_l2(got32[rows], want)
            err16 = rel_l2(got[rows], want)
            assert err16 <= 2.0 ** -8, (name, err16)
        else:
            err = rel_l2(got[rows], want)
        print(f"{name}: ring={ring} rel-L2 vs float64 {err:.3e}, bitwise equal to linear_kernel slices")
        assert err <= 1e-6, (name, err)
        # the sample is not dominated by the residual / bias: the GEMM part differs from a bf16-free one
        full = F.linear(x[rows].double(), m.weight.double(), m.bias.double() if bias else None)
        assert rel_l2(F.linear(x[rows].double(), m.weight.bfloat16().double(), m.bias.double() if bias else None), full) > 1e-4
