"""Phase timeline of fno_trunk_kernel from a DLWP_TRUNK_TRACE dump (100 MHz s_memrealtime stamps).
usage: DLWP_TRUNK_TRACE=trunk_trace.txt python tools/trunk_trace.py trunk_trace.txt [--staged-seam]

The first four stamps of a step depend on the seam the kernel ran.  With a live lifting table the
workgroup votes: "step top" = previous projection done -> this step's top, "lift vote" = input row, domain test, flag,
"seam barrier" = wait for the workgroup's slowest wave (plus, after a vote for it, staging the exact MLP's weights and the
barrier behind that), "lift" = gather from the table or the exact MLP (and then the barrier that frees its weights).  --staged-seam names them for the seam that always stages the exact path's weights
(no live table: DLWP_FNO_LIFT_TABLE=0, more input channels, a rejected table):
"step top" = end-of-step barrier + LDS write, "lift staged" = barrier, "lift seg" = gather or MLP, "lift all waves" = barrier."""
import os
import sys

import numpy as np

staged_seam = "--staged-seam" in sys.argv[2:] or os.environ.get("DLWP_FNO_LIFT_TABLE", "1") == "0"
path = sys.argv[1]
if not os.path.exists(path) or os.environ.get("DLWP_TRUNK_TRACE"):
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import build_model
    from dlwp_benchmark_amd.synthetic import navier_stokes

    model, _ = build_model("cuda:0")
    prog = navier_stokes(32, 4, 64, 64, seed=1)[2].to("cuda:0")
    for _ in range(3):   # the first launch of a process pays cold instruction caches; look at the later ones
        model(prognostic=prog)
    torch.cuda.synchronize()
rows = [list(map(int, l.split())) for l in open(path)]
# the two hand-off stamps of a layer ("P2 done", "P3+sync") carry in bits 56-63 the poll issue that delivered the traced wave's
# block: 1 = the first poll, 0 = the wave had no block in that phase (the 100 MHz counter stays below bit 56)
POLL_SHIFT, TIME_MASK = 56, (1 << 56) - 1
names = ["start"]
if os.environ.get("DLWP_FNO_STEP", "1") != "0":
    names = ["step top", "lift vote", "seam barrier", "lift", "lift done", "trunk setup"]
    if staged_seam:
        names = ["step top", "lift staged", "lift seg", "lift all waves", "lift done", "trunk setup"]
for l in range(4):
    names += [f"L{l} y-ready", f"L{l} P1 done", f"L{l} barrier1", f"L{l} P2 done", f"L{l} barrier2", f"L{l} P3+sync",
              f"L{l} skip+idft"]
    if l < 3:
        names += [f"L{l} gelu", f"L{l} transpose", f"L{l} fwd dft"]
names += ["rows done", "proj done"]
for launch in sorted({r[0] for r in rows})[-int(os.environ.get('TRACE_LAUNCHES', '1')):]:
    raw = np.array([r[2:] for r in rows if r[0] == launch], dtype=np.uint64)
    polls = (raw >> np.uint64(POLL_SHIFT)).astype(np.int64)
    t = (raw & np.uint64(TIME_MASK)).astype(np.float64)
    t0 = t[:, 0].min()
    rel = (t - t0) / 100.0
    print(f"launch {launch}: {t.shape[0]} workgroups, span {rel.max():.2f} us; start skew max {rel[:, 0].max():.2f} us")
    prev = rel[:, 0]
    for k in range(1, t.shape[1]):
        d = rel[:, k] - rel[:, k - 1]
        print(f"  {names[k % len(names)]:>14}: at mean {rel[:, k].mean():6.2f} us | phase mean {d.mean():5.2f} min {d.min():5.2f} max {d.max():5.2f}")
    # polls per hand-off: over every stamped hand-off of the launch (waves without a block left out).  The kernel keeps the
    # count of the LAST block a wave polled in the phase: at shapes where a wave takes several P2 passes or P3 columns
    # (more than 16 modes per workgroup, more than 8 kept columns) the earlier blocks' counts are not in the figures
    print("  polls per hand-off (last block of the phase where a wave polls several):")
    for what in ("P2 done", "P3+sync"):
        cols = [k for k in range(1, t.shape[1]) if names[k % len(names)].endswith(what)]
        n = polls[:, cols]
        n = n[n > 0]
        if n.size:
            print(f"    {what:>7}: mean {n.mean():.2f} max {n.max()} first-poll share {100.0 * (n == 1).mean():.1f} % "
                  f"({n.size} hand-offs)")
