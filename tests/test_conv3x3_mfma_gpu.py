"""The matrix-pipe forms of pad(1) + Conv2d(3x3) (csrc/conv_mfma.hip: conv_mfma_kernel<Padded3x3<TW>, NF, NIMG>, forms "bf16x6" and
"bf16" of ops.conv3x3*) against float64, through the networks against the committed real-class goldens, and under graph replay.

Bounds: form "bf16x6" is held to the direct kernel's bounds of tests/test_conv3x3_variants_gpu.py (rel-L2 1e-6 cylinder / 2e-6
HEALPix, max-abs 1e-5 max(1, |want|)); form "bf16" to the project's bf16 bound 5e-3, and -- without an input activation -- to
2e-6 against the float64 convolution of the RNE-bf16-rounded operands: its only error is the operand rounding.

The launcher picks the tile (8 x 16, or 16 x 8 where that leaves fewer live 16-pixel fragments) and NF = 4 / 2 / 1
16-channel fragments per workgroup (the largest that still makes 512 workgroups); mfma_variant() asks the library which instance
it launches for a shape (dlwp_conv3x3_mfma_variant: the launcher's own rule, not a copy) and a CPU test asserts that the cases
reach both tiles and every NF."""
import ctypes
import json

import pytest
import torch
import torch.nn.functional as F

from helpers import load_golden, per_step_rel_l2, rel_l2
from test_conv3x3_variants_gpu import ACT, ACT_FN, _images, _rand, _reference

DEV = "cuda:0"
TOL = 1e-5          # tests/test_backbones_gpu.py
TOL_BF16 = 5e-3


def mfma_variant(n, H, W, cout):
    """(tile width, NF) the launcher of csrc/conv_mfma.hip takes for n images of H x W and cout output channels"""
    from dlwp_benchmark_amd import lib as L

    v = int(L.load().dlwp_conv3x3_mfma_variant(n, H, W, cout))
    assert v > 0
    return v // 16, v % 16


# name -> (hpx, images (HEALPix: samples of 12 faces), H, W, c0, c1, cout, pre_act, act, resid, bias)
CASES = {
    "cyl_13x37": (False, 2, 13, 37, 5, 0, 7, "none", "gelu", False, True),
    "cyl_20x40_split_slab": (False, 2, 20, 40, 13, 6, 45, "gelu", "tanh", True, True),     # segment boundary inside a K-slab
    "cyl_9x10": (False, 1, 9, 10, 33, 0, 17, "tanh", "silu", True, False),
    "cyl_8x64_aligned": (False, 2, 8, 64, 64, 64, 64, "none", "relu", False, True),
    "cyl_3x2": (False, 1, 3, 2, 3, 0, 3, "none", "none", False, True),                     # smaller than any tile
    "hpx_8x8": (True, 1, 8, 8, 3, 0, 6, "none", "gelu", False, True),
    "hpx_12x12_co170": (True, 1, 12, 12, 10, 5, 170, "relu", "none", True, False),
    "hpx_20x20": (True, 2, 20, 20, 40, 0, 34, "silu", "tanh", False, True),
    # beyond the listed cases: the workgroup shapes only many tiles reach (NF = 2 and NF = 4), few input channels
    "cyl_nf2": (False, 8, 64, 64, 3, 0, 64, "none", "gelu", False, True),
    "cyl_nf4": (False, 8, 64, 64, 2, 3, 120, "none", "none", True, True),
    "hpx_nf2_narrow": (True, 2, 20, 20, 3, 0, 100, "gelu", "relu", False, True),
    "hpx_nf4_narrow": (True, 2, 20, 20, 3, 2, 200, "none", "silu", True, False),
}


def test_cases_cover_every_instance():
    seen = {mfma_variant(_images(v[0], v[1]), v[2], v[3], v[6]) for v in CASES.values()}
    assert seen == {(tw, nf) for tw in (8, 16) for nf in (1, 2, 4)}, seen
    assert mfma_variant(8, 64, 64, 64) == (16, 2) and mfma_variant(8, 64, 64, 120) == (16, 4)
    assert mfma_variant(24, 20, 20, 100) == (8, 2) and mfma_variant(24, 20, 20, 200) == (8, 4)
    assert mfma_variant(12, 8, 8, 6) == (8, 1) and mfma_variant(1, 9, 10, 17) == (16, 1) and mfma_variant(1, 3, 2, 3) == (8, 1)


_MADE = {}


def _case(name):
    """inputs and the float64 reference of a case, made once"""
    if name not in _MADE:
        hpx, n, H, W, c0, c1, cout, pre, act, has_resid, has_bias = CASES[name]
        pre, act, imgs = ACT[pre], ACT[act], _images(hpx, n)
        g = torch.Generator(device=DEV).manual_seed(imgs * 1000 + cout)
        x0 = _rand(imgs, c0, H, W, g=g, scale=1.5)
        x1 = _rand(imgs, c1, H, W, g=g) if c1 else None
        w = _rand(cout, c0 + c1, 3, 3, g=g, scale=1.0 / (3.0 * (c0 + c1) ** 0.5))
        b = _rand(cout, g=g) if has_bias else None
        resid = _rand(imgs, cout, H, W, g=g) if has_resid else None
        with torch.no_grad():
            want = _reference(x0, x1, w, b, resid, pre, act, hpx)
        _MADE[name] = (x0, x1, w, b, resid, pre, act, hpx, want)
    return _MADE[name]


def _run(name, form):
    from dlwp_benchmark_amd import ops

    x0, x1, w, b, resid, pre, act, hpx, want = _case(name)
    with torch.no_grad():
        if pre or resid is not None:
            return ops.conv3x3(x0, w, b, act=act, x1=x1, pre_act=pre, resid=resid, hpx=hpx, form=form)
        return (ops.conv3x3_hpx if hpx else ops.conv3x3_cyl)(x0, w, b, act, x1=x1, form=form)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bf16x6_matches_float64(name):
    want, hpx = _case(name)[8], _case(name)[7]
    got = _run(name, "bf16x6")
    assert got.shape == want.shape and got.dtype == torch.float32
    err = rel_l2(got, want)
    print(f"{name} bf16x6: rel-L2 vs float64 {err:.3e}")
    assert err <= (2e-6 if hpx else 1e-6), (name, err)
    assert (got.double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item()), name
    assert torch.equal(_run(name, "bf16x6"), got), "rerun differs"


def _rounded_reference(x0, x1, w, b, resid, act, hpx):
    """float64 convolution of the RNE-bf16 operands: padded in float32 first (HEALPix corner means in fp32), then rounded"""
    from oracle.restate.healpix import healpix_pad

    x = x0 if x1 is None else torch.cat([x0, x1], 1)
    if hpx:
        xp = healpix_pad(x, 1)
    else:
        xp = F.pad(torch.cat([x[..., -1:], x, x[..., :1]], -1), (0, 0, 1, 1))
    y = F.conv2d(xp.bfloat16().double(), w.bfloat16().double(), b.double() if b is not None else None)
    if resid is not None:
        y = y + resid.double()
    return ACT_FN[act](y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bf16_form(name):
    x0, x1, w, b, resid, pre, act, hpx, want = _case(name)
    got = _run(name, "bf16")
    err = rel_l2(got, want)
    print(f"{name} bf16: rel-L2 vs float64 {err:.3e}")
    assert err <= TOL_BF16, (name, err)
    assert err > 1e-4, f"{name}: {err:.3e} is not a bf16-operand result"
    if pre == 0:
        with torch.no_grad():
            err_r = rel_l2(got, _rounded_reference(x0, x1, w, b, resid, act, hpx))
        print(f"{name} bf16: rel-L2 vs float64 on rounded operands {err_r:.3e}")
        assert err_r <= 2e-6, (name, err_r)
    assert torch.equal(_run(name, "bf16"), got), "rerun differs"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cyl_20x40_split_slab", "cyl_13x37", "hpx_12x12_co170", "hpx_8x8"])
def test_direct_through_the_keyword_is_the_default_path(name):
    from dlwp_benchmark_amd import ops

    x0, x1, w, b, resid, pre, act, hpx, _ = _case(name)
    with torch.no_grad():
        if pre or resid is not None:
            a = ops.conv3x3(x0, w, b, act=act, x1=x1, pre_act=pre, resid=resid, hpx=hpx)
        else:
            a = (ops.conv3x3_hpx if hpx else ops.conv3x3_cyl)(x0, w, b, act, x1=x1)
    assert torch.equal(_run(name, "direct"), a)


@pytest.mark.gpu
def test_pack_follows_the_weight():
    """the pack is re-derived after an in-place write and after invalidate_packed's epoch bump, and dies with its tensor"""
    from dlwp_benchmark_amd import ops

    g = torch.Generator(device=DEV).manual_seed(5)
    x, w = _rand(1, 5, 9, 12, g=g), _rand(7, 5, 3, 3, g=g, scale=0.2)
    with torch.no_grad():
        y1 = ops.conv3x3_cyl(x, w, None, form="bf16x6")
        buf = ops.conv3x3_weights(w).get(w)
        assert ops.conv3x3_weights(w).get(w) is buf
        w.mul_(2.0)
        y2 = ops.conv3x3_cyl(x, w, None, form="bf16x6")
        assert rel_l2(y2, 2.0 * y1.double()) <= 1e-6
        ops.bump_pack_epoch()
        assert ops.conv3x3_weights(w).get(w) is not buf
    n = ops.live_holders()
    del w
    assert ops.live_holders() == n - 1


def _unet_like(tag):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec
    from oracle.make_golden import MODEL_CASES, model_inputs

    family, cfg, (batch, frames), gain = MODEL_CASES[tag]
    g = load_golden(f"model_{tag}")
    sd, _ = fill_by_spec(json.loads(str(g["param_spec"])), gain=gain)
    cls = {"unet": M.UNet, "convlstm": M.ConvLSTM}[family]
    dev = lambda t: t.to(DEV) if t is not None else None
    c, p, x = [dev(t) for t in model_inputs(tag, cfg, batch, frames)]

    def make(**kw):
        model = cls(**cfg, **kw)
        model.load_state_dict(sd, strict=False)
        return model.to(DEV).eval()

    return make, (lambda m: m(constants=c, prescribed=p, prognostic=x)), torch.from_numpy(g["y"])


def _hpx_like(table, cls_name, tag):
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec
    from oracle.make_golden import hpx_inputs

    cfg, (batch, frames), hw = table[tag]
    g = load_golden(f"model_{tag}")
    sd, _ = fill_by_spec(json.loads(str(g["param_spec"])), gain=1.0)
    ins = [t.to(DEV) if t is not None else None for t in hpx_inputs(tag, cfg, batch, frames, hw)]

    def make(**kw):
        model = getattr(M, cls_name)(**cfg, **kw)
        model.load_state_dict(sd, strict=True)
        return model.to(DEV).eval()

    return make, (lambda m: m(*ins)), torch.from_numpy(g["y"])


DIFF_TAG = "diffmunethpx_h8_16"


def _diffusion():
    import dlwp_benchmark_amd.models as M
    from dlwp_benchmark_amd.weights import fill_by_spec
    from oracle.make_golden import DIFFUSION_CASES, DIFFUSION_SEED, diffusion_inputs
    from oracle.restate.ddpm import DDPMSchedulerRestated

    cls, cfg, (batch, frames), hw, betas, nsteps = DIFFUSION_CASES[DIFF_TAG]
    g = load_golden(f"model_{DIFF_TAG}")
    sd, _ = fill_by_spec(json.loads(str(g["param_spec"])), gain=0.7)
    c, p, x = [t.to(DEV) if t is not None else None for t in diffusion_inputs(DIFF_TAG, cls, cfg, batch, frames, hw)]

    def make(**kw):
        model = getattr(M, cls)(**cfg, **kw)
        model.load_state_dict(sd, strict=False)
        return model.to(DEV).eval()

    def run(m):
        sched = DDPMSchedulerRestated(betas, seed=7)
        sched.set_timesteps(nsteps)
        torch.manual_seed(DIFFUSION_SEED)
        return m(constants=c, prescribed=p, prognostic=x, noise_scheduler=sched)

    return make, run, torch.from_numpy(g["y"])


def _network_cases():
    from oracle.make_golden import HPX_MODEL_CASES, HPX_MUNET_CASES

    cases = [("unet", "unet_c1_64x64"), ("unet", "unet_h4_32x64"), ("unet", "convlstm_h8_32x64")]
    cases += [("unethpx", t) for t in HPX_MODEL_CASES] + [("munethpx", t) for t in HPX_MUNET_CASES]
    return cases + [("diffusion", DIFF_TAG)]


def _network(kind, tag):
    from oracle.make_golden import HPX_MODEL_CASES, HPX_MUNET_CASES

    if kind == "unet":
        return _unet_like(tag)
    if kind == "unethpx":
        return _hpx_like(HPX_MODEL_CASES, "UNetHPX", tag)
    if kind == "munethpx":
        return _hpx_like(HPX_MUNET_CASES, "MUNetHPX", tag)
    return _diffusion()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,tag", _network_cases())
def test_networks_match_the_reference_goldens(kind, tag):
    """set_conv_form("bf16x6") within the fp32 tolerance of the goldens, compute_precision="bf16" within the bf16 one"""
    make, run, want = _network(kind, tag)
    default = run(make()).clone()
    model = make().set_conv_form("bf16x6")
    assert {m.conv_form for m in model.modules() if "conv_form" in m.__dict__} == {"bf16x6"}
    got = run(model).clone()
    assert not torch.equal(got, default), "the bf16x6 network gave the direct kernel's bits: the form did not reach the op"
    assert got.shape == want.shape
    errs = per_step_rel_l2(got, want)
    print(f"{tag} bf16x6: per-step rel-L2 {['%.2e' % e for e in errs]}")
    assert max(errs) <= TOL, f"{tag}: per-step rel L2 {['%.2e' % e for e in errs]}"
    got16 = run(make(compute_precision="bf16"))
    assert not torch.equal(got16, default) and not torch.equal(got16, got), "the bf16 form did not reach the op"
    errs16 = per_step_rel_l2(got16, want)
    print(f"{tag} bf16: per-step rel-L2 {['%.2e' % e for e in errs16]}")
    assert max(errs16) <= TOL_BF16, f"{tag} bf16: per-step rel L2 {['%.2e' % e for e in errs16]}"


@pytest.mark.gpu
def test_graph_replay_and_form_change():
    make, run, _ = _unet_like("unet_c1_64x64")
    default = run(make()).clone()
    model = make().set_conv_form("bf16x6")
    eager = run(model).clone()
    assert not torch.equal(eager, default)
    model.set_step_graphs(True)
    assert torch.equal(run(model), eager)
    assert torch.equal(run(model), eager)          # replay of the cached graph
    model.set_conv_form("direct")                  # drops the capture: the next call runs (and captures) the direct kernel
    assert torch.equal(run(model), default)


@pytest.mark.gpu
def test_the_3x3_pack_is_the_kxk_pack_at_k3():
    """[17, 33, 3, 3] (a partial fragment and a partial slab): dlwp_conv3x3_mfma_pack_f32 and dlwp_conv2d_mfma_pack_f32(k 3, not
    transposed) write the same bytes"""
    from dlwp_benchmark_amd import lib as L

    lib = L.load()
    w = _rand(17, 33, 3, 3, g=torch.Generator(device=DEV).manual_seed(3))
    nbytes = int(lib.dlwp_conv3x3_mfma_packed_bytes(17, 33))
    assert nbytes == int(lib.dlwp_conv2d_mfma_packed_bytes(17, 33, 3)) == 3 * 9 * 2 * 2 * 1024
    a = torch.full((nbytes // 4,), -1, dtype=torch.int32, device=DEV)
    b = torch.full((nbytes // 4,), -2, dtype=torch.int32, device=DEV)
    L.launch("dlwp_conv3x3_mfma_pack_f32", w.device, w, 17, 33, a)
    L.launch("dlwp_conv2d_mfma_pack_f32", w.device, w, 17, 33, 3, 0, b)
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,variant", [(9, 10, (16, 1)), (20, 20, (8, 1))])
@pytest.mark.parametrize("form", ["bf16x6", "bf16"])
def test_cylinder_and_zero_padding_agree_bitwise_inside(H, W, variant, form):
    """One kernel body, two loaders: on output columns 1 .. W-2 the circular and the zero padding read the same cells, and the
    tile, the window and the tap order are the same (one planner), so pad(1) + 3x3 on the cylinder and Conv2d(3, 1, 1) agree
    bit for bit there.  9 x 10: fragment rows of 16; 20 x 20: two rows of 8."""
    from dlwp_benchmark_amd import ops
    from test_conv_aux_mfma_gpu import aux_variant

    assert mfma_variant(1, H, W, 17) == variant and aux_variant(False, 1, H, W, 17, 3, 1, 1) == variant
    g = torch.Generator(device=DEV).manual_seed(H * 100 + W)
    x, w, b = _rand(1, 33, H, W, g=g, scale=1.5), _rand(17, 33, 3, 3, g=g, scale=1.0 / (3.0 * 33 ** 0.5)), _rand(17, g=g)
    with torch.no_grad():
        cyl = ops.conv3x3_cyl(x, w, b, ACT["gelu"], form=form)
        zero = ops.conv2d(x, w, b, 1, 1, act=ACT["gelu"], form=form)
    assert cyl.shape == zero.shape == (1, 17, H, W)
    assert torch.equal(cyl[..., 1:W - 1], zero[..., 1:W - 1])
    assert not torch.equal(cyl[..., 0], zero[..., 0])        # the paddings themselves differ


@pytest.mark.gpu
def test_sizes_past_the_32_bit_offsets_are_unsupported():
    """rejected by the argument checks, before any launch: the tiny tensors are never read at the declared sizes"""
    from dlwp_benchmark_amd import lib as L

    lib = L.load()
    t = torch.zeros(64, device=DEV)
    assert lib.dlwp_conv3x3_mfma_packed_bytes(0, 4) == 0 and lib.dlwp_conv3x3_mfma_packed_bytes(4, 0) == 0
    null = ctypes.c_void_p(None)
    # 4 channels of 32768 x 32768: the channel-plane offset inside one sample reaches 2^32; and 2^20 x 2^20 weights: pack > 2 GiB
    for c0, cout, H, W in ((4, 4, 32768, 32768), (1 << 20, 1 << 20, 4, 4)):
        rc = lib.dlwp_conv3x3_mfma_f32(t.data_ptr(), c0, null, 0, t.data_ptr(), null, null, t.data_ptr(), 1, H, W, cout, 0, 0,
                                       null, 0, L.stream_ptr())
        assert rc == -2, rc      # DLWP_ERR_UNSUPPORTED
        with pytest.raises(L.DlwpError, match="status -2"):
            L.check(rc, "dlwp_conv3x3_mfma_f32")
    torch.cuda.synchronize()
