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


--part backward (or all) adds the backwards, by the same method at the two legendre-gauss shapes:
  sht_backward, isht_backward                   ops.* against the backward of the torch form (training._grad_of_torch_form of
                                                sht_torch / isht_torch: what the Functions ran before they had kernels)
  sph_mix_dgrad {packed, in_place}              the two candidates of the input gradient: a per-call degree-major pack of the
                                                conjugate transpose + the packed kernel, or the weight read in place
  sph_mix_wgrad {packed, direct}                the two candidates of the weight gradient's store: degree-major scratch + transpose
                                                back, or straight into the parameter layout
  sfno_train_step                               forward + backward of the 4-block network (MLP, big skip, pos_embed), "hip": the HIP
                                                backwards of the three ops; "torch": `switch` "env" is DLWP_TRAIN_TORCH_BACKWARD=1
                                                (read at every call: the two alternate in one process; it also turns the
                                                convolutions into the plain composition), `switch` "three_ops" sends ONLY the
                                                three ops to their torch forms.  conv_dgrad: DLWP_CONV_DGRAD of the run
                                                ("hip": the bf16x6 matrix-pipe convolutions).  peak_mb_*: max_memory_allocated of one step.

Usage: python tools/bench_sht.py [--part forward|backward|all] [--reps 15] [--inner 20] [--warmup 3] [--out FILE]
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
    ap.add_argument("--part", default="all", choices=("forward", "backward", "all"))
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

    def peak_mb(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)

    def backward_part(grid, nlat, nlon, embed, batch):
        modes = min(nlat, nlon // 2)
        shape = {"grid": grid, "nlat": nlat, "nlon": nlon, "embed": embed, "batch": batch, "modes": modes}
        tab = S.device_tables(grid, nlat, nlon, modes, modes, dev)
        gen = torch.Generator(device=dev).manual_seed(nlat + 1)
        x = torch.randn(batch, embed, nlat, nlon, device=dev, generator=gen)
        gy = torch.randn(batch, embed, nlat, nlon, device=dev, generator=gen)
        c = ops.sht(x, grid, modes, modes)
        g = ops.sht(gy, grid, modes, modes)
        w = torch.view_as_complex(torch.randn(embed, embed, modes, 2, device=dev, generator=gen) / embed ** 0.5)
        planes = batch * embed
        field, spec, wbytes = planes * nlat * nlon * 4, planes * modes * modes * 8, embed * embed * modes * 8
        gflop = round(8 * batch * embed * embed * modes * (modes + 1) / 2 / 1e9, 3)
        torch_form = T._grad_of_torch_form
        measure("sht_backward", shape, lambda: ops.sht_backward(g, grid, nlat, nlon),
                lambda: torch_form(lambda t: T.sht_torch(t, tab), (x,), (True,), g)[0], field + spec)
        measure("isht_backward", shape, lambda: ops.isht_backward(gy, grid, modes, modes),
                lambda: torch_form(lambda t: T.isht_torch(t, tab), (c,), (True,), gy)[0], field + spec)
        for cand in ("packed", "in_place"):
            measure("sph_mix_dgrad", shape, lambda: ops.sph_mix_backward(c, w, g, True, False, dgrad=cand)[0],
                    lambda: torch_form(T.sph_mix_torch, (c, w), (True, False), g)[0], 2 * spec + wbytes, candidate=cand, gflop=gflop)
        for cand in ("packed", "direct"):
            measure("sph_mix_wgrad", shape, lambda: ops.sph_mix_backward(c, w, g, False, True, wgrad=cand)[1],
                    lambda: torch_form(T.sph_mix_torch, (c, w), (False, True), g)[1], 2 * spec + wbytes, candidate=cand, gflop=gflop)
        del x, gy, c, g, w
        model = SFNO2DModule(height=nlat, width=nlon, grid=grid, num_layers=4, scale_factor=1, embed_dim=embed, big_skip=True,
                             pos_embed=True, use_mlp=True)
        fill_state_dict(model, std_fn=lambda n, s: 0.7 / s[0] ** 0.5 if n.endswith("filter.weight") else None)
        model = model.to(dev).train()
        xin = torch.randn(batch, model.in_channels, nlat, nlon, device=dev, generator=gen)
        hip_or_none = T._hip_backward_or_none

        def step(torch_backward: str, three_ops_torch: bool = False):
            os.environ["DLWP_TRAIN_TORCH_BACKWARD"] = torch_backward
            T._hip_backward_or_none = (lambda run: None) if three_ops_torch else hip_or_none
            try:
                with torch.enable_grad():
                    model.zero_grad(set_to_none=True)
                    model.sfno(xin).square().mean().backward()
            finally:
                os.environ["DLWP_TRAIN_TORCH_BACKWARD"] = "0"
                T._hip_backward_or_none = hip_or_none
            return model.sfno.blocks[1].filter.filter.weight.grad

        for conv_dgrad in ("torch", "hip"):
            os.environ["DLWP_CONV_DGRAD"] = conv_dgrad
            for switch, tor in (("env", lambda: step("1")), ("three_ops", lambda: step("0", True))):
                try:
                    measure("sfno_train_step", shape, lambda: step("0"), tor, 0, switch=switch, conv_dgrad=conv_dgrad,
                            peak_mb_hip=peak_mb(lambda: step("0")), peak_mb_torch=peak_mb(tor))
                except DlwpError as e:
                    print(json.dumps({"op": "sfno_train_step", **shape, "switch": switch, "conv_dgrad": conv_dgrad, "error": str(e)}),
                          flush=True)
        os.environ.pop("DLWP_CONV_DGRAD", None)
        del model
        torch.cuda.empty_cache()

    with torch.no_grad():
        for grid, nlat, nlon, embed, batch in SHAPES:
            if args.part in ("backward", "all") and grid == "legendre-gauss":
                backward_part(grid, nlat, nlon, embed, batch)
            if args.part == "backward":
                continue
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
