"""Times the spherical harmonic transforms, the Driscoll-Healy channel mix (csrc/sht.hip) and a whole SFNO step against their
torch compositions on the device (training.sht_torch / isht_torch / sph_mix_torch: torch.fft + einsum on the same fp32 tables;
the step: the same network with torch convolutions around them), at the shape of configs/model/sfno.yaml (32 x 64, embed 256,
batch 16) on both quadratures and at 64 x 128 / embed 64 / batch 8.

Per (op, shape) one JSON line:
  ms_hip / ms_torch   median over --reps of HIP-event brackets around --inner back-to-back calls, divided by --inner; the two are
                      alternated bracket by bracket in one process, after --warmup brackets of each
  bytes               what the op has to move once (fields 4 B, coefficients 8 B, weights 8 B; tables left out)
  gbytes_per_s_hip    bytes / ms_hip
  rel_l2              the two results against each other
`sph_mix` runs the cached degree-major pack of the weight (ops.sph_mix(..., owner=)), `sph_mix_parameter_layout` the kernel
that reads the parameter as it lies.  The step is timed with the 1x1 convolutions in both forms of
HipBackbone.set_aux_conv_form ("direct", "bf16x6").

Usage: python tools/bench_sht.py [--reps 15] [--inner 20] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("legendre-gauss", 32, 64, 256, 16), ("equiangular", 32, 64, 256, 16), ("legendre-gauss", 64, 128, 64, 8)]


def bracket(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    return e0, e1


def torch_step(model, x):
    """the network of models/sfno.py with torch operators (scale_factor 1: one grid per transform pair)"""
    from dlwp_benchmark_amd import sphere as S
    from dlwp_benchmark_amd import training as T

    net = model.sfno
    act = {1: F.gelu, 3: F.relu}[net.act]
    conv = lambda m, v: F.conv2d(v, m.weight, m.bias)
    y = conv(net.encoder["2"], act(conv(net.encoder["0"], x)))
    if net.pos_embed is not None:
        y = y + net.pos_embed
    last = len(net.blocks) - 1
    for i, blk in enumerate(net.blocks):
        fwd = net.trans_down if i == 0 else net.trans
        inv = net.itrans_up if i == last else net.itrans
        tf = S.device_tables(fwd.grid, fwd.nlat, fwd.nlon, net.modes, net.modes, x.device)
        ti = S.device_tables(inv.grid, inv.nlat, inv.nlon, net.modes, net.modes, x.device)
        c = T.sht_torch(y, tf)
        r = y if fwd.same_grid(inv) else T.isht_torch(c, ti)
        f = T.isht_torch(T.sph_mix_torch(c, torch.view_as_complex(blk.filter.filter.weight)), ti)
        z = act(f + conv(blk.inner_skip, r))
        if blk.use_mlp:
            z = conv(blk.mlp.fwd["2"], act(conv(blk.mlp.fwd["0"], z)))
        y = z + r
    if net.big_skip:
        y = torch.cat([y, x], dim=1)
    return conv(net.decoder["2"], act(conv(net.decoder["0"], y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sht: no GPU; a timing taken anywhere else says nothing")

    from dlwp_benchmark_amd import ops
    from dlwp_benchmark_amd import sphere as S
    from dlwp_benchmark_amd import training as T
    from dlwp_benchmark_amd.lib import DlwpError
    from dlwp_benchmark_amd.models import SFNO2DModule
    from dlwp_benchmark_amd.weights import fill_state_dict

    dev = torch.device("cuda:0")
    lines = []

    def rel(a, b):
        a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
        return float(torch.linalg.vector_norm(a.double() - b.double()) / torch.linalg.vector_norm(b.double()))

    def measure(op, shape, hip, tor, nbytes, **extra):
        diff = rel(hip(), tor())
        for _ in range(args.warmup):
            bracket(hip, args.inner)
            bracket(tor, args.inner)
        torch.cuda.synchronize()
        ev = {"hip": [], "torch": []}
        for _ in range(args.reps):
            ev["hip"].append(bracket(hip, args.inner))
            ev["torch"].append(bracket(tor, args.inner))
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) / args.inner for a, b in v] for k, v in ev.items()}
        ms_hip, ms_torch = statistics.median(ms["hip"]), statistics.median(ms["torch"])
        line = {"op": op, **shape, **extra, "ms_hip": round(ms_hip, 5), "ms_hip_min_max": [round(min(ms["hip"]), 5), round(max(ms["hip"]), 5)],
                "ms_torch": round(ms_torch, 5), "ms_torch_min_max": [round(min(ms["torch"]), 5), round(max(ms["torch"]), 5)],
                "speedup": round(ms_torch / ms_hip, 2), "bytes": nbytes, "gbytes_per_s_hip": round(nbytes / ms_hip / 1e6, 1),
                "rel_l2": diff, "reps": args.reps, "inner": args.inner}
        print(json.dumps(line), flush=True)
        lines.append(line)

    with torch.no_grad():
        for grid, nlat, nlon, embed, batch in SHAPES:
            modes = min(nlat, nlon // 2)
            shape = {"grid": grid, "nlat": nlat, "nlon": nlon, "embed": embed, "batch": batch, "modes": modes}
            tab = S.device_tables(grid, nlat, nlon, modes, modes, dev)
            gen = torch.Generator(device=dev).manual_seed(nlat)
            x = torch.randn(batch, embed, nlat, nlon, device=dev, generator=gen)
            c = ops.sht(x, grid, modes, modes)
            w = torch.view_as_complex(torch.randn(embed, embed, modes, 2, device=dev, generator=gen) / embed ** 0.5)
            planes = batch * embed
            field, spec = planes * nlat * nlon * 4, planes * modes * modes * 8
            measure("sht", shape, lambda: ops.sht(x, grid, modes, modes), lambda: T.sht_torch(x, tab), field + spec)
            measure("isht", shape, lambda: ops.isht(c, grid, nlat, nlon), lambda: T.isht_torch(c, tab), field + spec)
            wreal = torch.view_as_real(w)       # the "Parameter" the pack is cached on
            for op, fn in (("sph_mix", lambda: ops.sph_mix(c, w, owner=wreal)), ("sph_mix_parameter_layout", lambda: ops.sph_mix(c, w))):
                measure(op, shape, fn, lambda: T.sph_mix_torch(c, w), 2 * spec + embed * embed * modes * 8,
                        gflop=round(8 * batch * embed * embed * modes * (modes + 1) / 2 / 1e9, 3))
            model = SFNO2DModule(height=nlat, width=nlon, grid=grid, num_layers=4, scale_factor=1, embed_dim=embed, big_skip=True,
                                 pos_embed=True, use_mlp=True)
            fill_state_dict(model, std_fn=lambda n, s: 0.7 / s[0] ** 0.5 if n.endswith("filter.weight") else None)
            model = model.to(dev).eval()
            xin = torch.randn(batch, model.in_channels, nlat, nlon, device=dev, generator=gen)
            for form in ("direct", "bf16x6"):
                model.set_aux_conv_form(form)
                try:
                    measure("sfno_step", shape, lambda: model.one_step(xin), lambda: torch_step(model, xin), 0, aux_conv_form=form)
                except DlwpError as e:          # a convolution shape outside the matrix-pipe form's envelope: say so, go on
                    print(json.dumps({"op": "sfno_step", **shape, "aux_conv_form": form, "error": str(e)}), flush=True)
            del x, c, w, model
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
