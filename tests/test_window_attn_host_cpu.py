"""The host layer of the window-attention forward family (csrc/window_attn_desc.hpp, select_path and the entry points of
csrc/window_attn.hip, the planners of csrc/window_attn2.hip / window_attn3.hip), without a GPU: only calls that end before
any HIP call -- dlwp_window_attn_workspace_bytes, and the run entry points with descriptors the argument checks refuse.

* coverage: the library's path selection equals the restated host rules of tests/test_window_attn_ref_cpu.py at every entry
  of its tables (the `_covered` assertion of tests/test_window_attn_fp64_gpu.py, made where no GPU is needed);
* sizes: workspace sizes pinned as numbers read off the library of the commit BEFORE the host layer was unified (one reading
  of the descriptor, one dispatch), never off the code under test;
* bad descriptors: each in a child process, so that a crash (the planners once divided by a zero extent before any check)
  shows as a signal exit; a clean error with the generic path's status and text is expected.
"""
import ctypes
import json
import os
import subprocess
import sys

import pytest

import test_window_attn_ref_cpu as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2          # DLWP_ERR_INVALID_ARGUMENT, DLWP_ERR_UNSUPPORTED (include/dlwp_hip.h)
ENTRIES = ("dlwp_window_attn_f32", "dlwp_window_attn_bf16", "dlwp_window_attn_bf16_io")


def _ws(spec, batch, bf16, form):
    from dlwp_benchmark_amd import lib as L

    dsc = spec.to_c()
    dsc.form = form
    return L.load().dlwp_window_attn_workspace_bytes(ctypes.byref(dsc), batch, bf16)


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
def _specs():
    return [(C.case_id(p), C.swin_spec(*p)) for p in C.SWIN_PARAMS] + [(C.case_id(p), C.pangu_spec(*p)[0]) for p in C.PANGU_PARAMS]


def test_workspace_query_selects_the_restated_path():
    for tag, spec in _specs():
        fast = C.path(spec) != "gen"
        assert (_ws(spec, C.BATCH, 0, 1) > 0) == fast, (tag, "bf16x6")
        assert (_ws(spec, C.BATCH, 1, -1) > 0) == fast, (tag, "bf16")
        assert _ws(spec, C.BATCH, 0, 0) == 0, (tag, "the fp32-MFMA form is the generic kernel")


# ---------------------------------------------------------------------------------------------------------------------
# sizes: (table, case, workspace bytes at batch 2 for bf16 = 0 with form 1, for bf16 = 1 with form -1), unshifted descriptors
# ---------------------------------------------------------------------------------------------------------------------
PINNED = [
    ("swin", (12, 64, 6, 32, 2, 48), 3_254_784, 1_092_096),          # SUB 1
    ("swin", (8, 32, 8, 32, 2, 8), 500_992, 173_312),                # SUB 2
    ("swin", (32, 64, 32, 64, 2, 24), 4_793_600, 1_647_872),         # SUB 4
    ("pangu", ((1, 16, 32), (2, 6, 12), 32), 79_488, 79_488),        # (RP, PP) = (1, 1)
    ("pangu", ((2, 12, 24), (2, 6, 12), 32), 52_992, 52_992),        # (2, 0)
    ("pangu", ((1, 8, 16), (1, 4, 8), 32), 3_840, 3_840),            # (1, 0)
]


@pytest.mark.parametrize("kind,case,x6,bf16", PINNED, ids=lambda v: C.case_id((v, False)) if isinstance(v, tuple) else None)
def test_workspace_sizes_are_the_earlier_library_s(kind, case, x6, bf16):
    spec = C.swin_spec(case, False) if kind == "swin" else C.pangu_spec(case, False)[0]
    assert (_ws(spec, 2, 0, 1), _ws(spec, 2, 1, -1)) == (x6, bf16)


def test_pinned_sizes_reach_every_sub_and_plane_plan():
    subs = {C.plan2(C.swin_spec(c, False)) for k, c, _, _ in PINNED if k == "swin"}
    planes = {C.plan3(C.pangu_spec(c, False)[0])[:2] for k, c, _, _ in PINNED if k == "pangu"}
    assert subs == {1, 2, 4} and planes == {(1, 1), (2, 0), (1, 0)}


# ---------------------------------------------------------------------------------------------------------------------
# bad descriptors
# ---------------------------------------------------------------------------------------------------------------------
BIG = 1 << 30
# 2-D, one 8 x 32 window, 2 heads of 8: the 2-D fast path covers it (PINNED, second row)
GOOD = dict(grid=[1, 8, 32], padded=[1, 8, 32], pad_lead=[0, 0, 0], window=[1, 8, 32], shift_fwd=[0, 0, 0], shift_back=[0, 0, 0],
            use_mask=0, mask_b1=[BIG] * 3, mask_b2=[BIG] * 3, bias_mode=0, heads=2, head_dim=8, scale=8 ** -0.5, form=1)
# 6 x 10 windows, 2 heads of 32: neither fast path covers it
PLAIN = dict(GOOD, grid=[1, 12, 20], padded=[1, 12, 20], window=[1, 6, 10], head_dim=32, scale=32 ** -0.5)

POSITIVE = (INVALID, "grid and window must be positive")
SMALLER = (INVALID, "padded grid smaller than grid + leading pad")
NOT_COVERED = (UNSUPPORTED, "window attention with bfloat16 tensors: descriptor not covered by the fast kernels")


def _multiple(padded, window):
    return (INVALID, "padded grid (%d,%d,%d) is not a multiple of the window (%d,%d,%d)" % (*padded, *window))


def _changed(base, **fields):
    d = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
    for k, v in fields.items():
        if isinstance(v, dict):
            for i, x in v.items():
                d[k][i] = x
        else:
            d[k] = v
    return d


def _bad_cases():
    """(id, descriptor or None, {entry: (status, last-error text)}): what the generic path's checks answer, in their order
    (check_desc in csrc/window_attn_desc.hpp).  With bfloat16 tensors a descriptor with all extents positive that the fast
    kernels decline is DLWP_ERR_UNSUPPORTED; one with a non-positive extent gets the generic path's answer."""
    cases = []
    for field in ("grid", "window", "padded"):
        for pos in range(3):
            for v in (0, -1):
                d = _changed(GOOD, **{field: {pos: v}})
                if field != "padded":
                    want = POSITIVE
                elif d["padded"][pos] % d["window"][pos]:          # (C: -1 % 8 = -1, -1 % 1 = 0; Python's sign differs, not its zero)
                    want = _multiple(d["padded"], d["window"])
                else:
                    want = SMALLER
                cases.append(("%s[%d]=%d" % (field, pos, v), d, {e: want for e in ENTRIES}))
    # grid = padded = (1, 0, 32): the 2-D planner's cover predicate let 0 % wlat == 0 through and reduced a roll modulo 0
    cases.append(("grid=padded=(1,0,32)", _changed(GOOD, grid={1: 0}, padded={1: 0}), {e: POSITIVE for e in ENTRIES}))
    d = _changed(GOOD, padded={2: 40})
    cases.append(("padded-not-a-multiple", d, dict({e: _multiple(d["padded"], d["window"]) for e in ENTRIES[:2]}, **{ENTRIES[2]: NOT_COVERED})))
    cases.append(("padded<grid+pad_lead", _changed(GOOD, pad_lead={1: 1}), dict({e: SMALLER for e in ENTRIES[:2]}, **{ENTRIES[2]: NOT_COVERED})))
    hd = (UNSUPPORTED, "head_dim 20: kernels are instantiated for 8, 16, 24, 32, 48, 64")
    cases.append(("head_dim=20", _changed(GOOD, head_dim=20), dict({e: hd for e in ENTRIES[:2]}, **{ENTRIES[2]: NOT_COVERED})))
    # form is read by dlwp_window_attn_f32 alone, which checks its range first; on a descriptor of the generic path, so that the
    # workspace query (which does not look at the range) answers 0 like for every other case
    cases.append(("form=2", _changed(PLAIN, form=2), {ENTRIES[0]: (INVALID, "form 2 not in {-1, 0, 1}")}))
    cases.append(("null-descriptor", None, {ENTRIES[0]: (INVALID, "null descriptor"), ENTRIES[1]: (INVALID, "null argument"),
                                            ENTRIES[2]: (INVALID, "null argument")}))
    return cases


# argv[1]: {"desc": fields or null, "entries": [...]} -> {"ws": [bf16 = 0, bf16 = 1], "clean": text, "runs": {entry: [status, text]}}
# The run entry points get non-null dummy tensors, batch 1 and NO workspace, and only after both workspace queries said 0.
CHILD = r"""
import ctypes, json, sys
from dlwp_benchmark_amd import lib as L
case = json.loads(sys.argv[1])
lib = L.load()
ref = None
if case["desc"] is not None:
    d = L.WAttnDesc()
    for k, v in case["desc"].items():
        if isinstance(v, list):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    ref = ctypes.byref(d)
out = {"ws": [lib.dlwp_window_attn_workspace_bytes(ref, 1, b) for b in (0, 1)], "runs": {}}
out["clean"] = lib.dlwp_last_error().decode()
if out["ws"] == [0, 0]:
    p = ctypes.c_void_p(4096)
    for name in case["entries"]:
        rc = getattr(lib, name)(ref, p, p, p, p, 1, None, 0, None)
        out["runs"][name] = [rc, lib.dlwp_last_error().decode()]
print(json.dumps(out))
"""


def run_child(desc, entries):
    env = dict(os.environ, PYTHONPATH=ROOT)          # the child imports dlwp_benchmark_amd.lib alone: ctypes, no torch
    r = subprocess.run([sys.executable, "-c", CHILD, json.dumps({"desc": desc, "entries": list(entries)})], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return r.returncode, (json.loads(r.stdout) if r.returncode == 0 else None), r.stderr


@pytest.mark.parametrize("case", _bad_cases(), ids=lambda c: c[0])
def test_bad_descriptor_is_a_clean_error(case):
    _, desc, want = case
    rc, got, err = run_child(desc, want)
    assert rc == 0, "the child ended with status %d (negative: a signal)\n%s" % (rc, err)
    assert got["ws"] == [0, 0]
    assert got["clean"] == "", "a workspace query left an error text behind"
    assert {e: tuple(v) for e, v in got["runs"].items()} == want


def test_an_uncovered_descriptor_leaves_no_error_text():
    rc, got, err = run_child(PLAIN, ())
    assert rc == 0, err
    assert got == {"ws": [0, 0], "clean": "", "runs": {}}
