"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/dlwp_hip.h
declares, and the product path fails loudly without a GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

from dlwp_benchmark_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dlwp_[a-z0-9_]+)\s*\(", src)))


def test_library_loads_and_exports_every_declared_symbol():
    lib = L.load()
    declared = _declared_symbols()
    assert declared, "no symbols parsed from include/dlwp_hip.h"
    for name in declared:
        assert hasattr(lib, name), f"libdlwp_hip.so does not export {name}"
    # the ctypes table covers the header exactly
    assert sorted(L.SIGNATURES) == declared
    assert lib.dlwp_version() >= 100


_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}
_STRUCTS = {"dlwp_fno2d_desc": "FNO2dDesc", "dlwp_wattn_desc": "WAttnDesc", "dlwp_mgn_mlp_desc": "MgnMlpDesc",
            "dlwp_gc_linear_args": "GcLinearArgs"}
_STRUCT_RE = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;"


def _header():
    src = open(os.path.join(ROOT, "include", "dlwp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*|^\s*#.*$", "", src, flags=re.M)      # and the preprocessor lines


def _c_class(decl: str):
    """"ptr" for anything with a `*`, else the ctypes type of the exact scalar type a C declaration names"""
    if "*" in decl:
        return "ptr"
    return _SCALARS[[w for w in decl.split() if w != "const"][0]]


def _ctypes_class(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    return t


def _header_prototypes():
    """{name: (class of the return type, [class of each parameter])}; an array parameter is a pointer"""
    src = re.sub(_STRUCT_RE, "", _header(), flags=re.S)
    src = re.sub(r"typedef\s+enum\s+\w+\s*\{.*?\}\s*\w+\s*;", "", src, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(dlwp_\w+)\s*\(([^()]*)\)\s*;", src):
        assert name not in out, f"{name} is declared twice"
        params = [p.strip() for p in params.split(",")]
        params = [] if params == ["void"] else params
        out[name] = (_c_class(ret), ["ptr" if "[" in p else _c_class(p) for p in params])
    return out


def _header_structs():
    """{struct: [(field, class or (class, length) for an array field)]} with `int32_t a, b;` as two fields"""
    out = {}
    for name, body in re.findall(_STRUCT_RE, _header(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            base = re.match(r"(.*?)(\w+)\s*(\[\d+\])?$", first, flags=re.S).group(1)
            for d in [first] + [base + m for m in more]:
                typ, field, length = re.match(r"(.*?)(\w+)\s*(?:\[(\d+)\])?$", d, flags=re.S).groups()
                fields.append((field, (_c_class(typ), int(length)) if length else _c_class(typ)))
        out[name] = fields
    return out


def test_signatures_match_the_header_type_by_type():
    """lib.SIGNATURES is a hand-kept mirror of include/dlwp_hip.h: a c_int32 where the header says int64_t, or a dropped
    argument, would load cleanly and corrupt a launch.  Every prototype's return and parameter types, in arity and position."""
    protos = _header_prototypes()
    assert len(protos) == len(L.SIGNATURES) and len(protos) > 100
    assert sorted(protos) == sorted(L.SIGNATURES)
    for name, (ret, params) in protos.items():
        res, args = L.SIGNATURES[name]
        assert _ctypes_class(res) == ret, f"{name}: return type {res} against the header's {ret}"
        assert [_ctypes_class(a) for a in args] == params, f"{name}: argument types differ from the header"


def test_structure_mirrors_match_the_header_field_by_field():
    """the four ctypes.Structure mirrors: the header's field names in its order, types classified like the prototypes'
    (an array field by its element class and its length)"""
    structs = _header_structs()
    assert sorted(structs) == sorted(_STRUCTS)
    for cname, pyname in _STRUCTS.items():
        mirror = [(f, (_ctypes_class(t._type_), t._length_) if issubclass(t, ctypes.Array) else _ctypes_class(t))
                  for f, t in getattr(L, pyname)._fields_]
        assert mirror == structs[cname], f"{pyname} differs from struct {cname}"


def test_error_reporting_without_gpu():
    lib = L.load()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert lib.dlwp_device_count() < 0
    assert b"hipGetDeviceCount" in lib.dlwp_last_error()


def test_product_path_refuses_cpu_tensors():
    from dlwp_benchmark_amd.models import FNO2DModule

    m = FNO2DModule(constant_channels=0, prescribed_channels=0, prognostic_channels=1, context_size=1).eval()
    with pytest.raises(L.DlwpError, match="no CPU fallback"):
        m(prognostic=torch.zeros(1, 3, 1, 64, 64))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "dlwp_benchmark_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f"{f} imports oracle"


def test_state_dicts_match_reference_layout():
    """Product modules expose exactly the reference's state-dict keys / shapes / dtypes (recorded
    from the real reference classes in the golden fixtures): checkpoints load unchanged."""
    import json

    import dlwp_benchmark_amd.models as M
    from helpers import load_golden
    from oracle.make_golden import MODEL_CASES

    names = {"swin": "SwinTransformer", "pangu": "PanguWeather", "afno": "FourCastNet", "unet": "UNet",
             "convlstm": "ConvLSTM"}
    checked = 0
    for tag, (family, cfg, _, _) in MODEL_CASES.items():
        if not hasattr(M, names[family]):
            continue
        g = load_golden(f"model_{tag}")
        want = {k: (tuple(s), d) for k, s, d in json.loads(str(g["state_spec"]))}
        m = getattr(M, names[family])(**cfg)
        got = {k: (tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in m.state_dict().items()}
        assert got == want, (tag, sorted(set(want) ^ set(got))[:6])
        checked += 1
    assert checked >= 3
    from oracle.make_golden import HPX_MODEL_CASES

    for tag, (cfg, _, _) in HPX_MODEL_CASES.items():
        g = load_golden(f"model_{tag}")
        want = {k: (tuple(s), d) for k, s, d in json.loads(str(g["state_spec"]))}
        got = {k: (tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in M.UNetHPX(**cfg).state_dict().items()}
        assert got == want, (tag, sorted(set(want) ^ set(got))[:6])
    from oracle.make_golden import HPX_MUNET_CASES, HPX_SWIN_CASES

    for tag, (cfg, _, _) in HPX_MUNET_CASES.items():
        g = load_golden(f"model_{tag}")
        want = {k: (tuple(s), d) for k, s, d in json.loads(str(g["state_spec"]))}
        got = {k: (tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in M.MUNetHPX(**cfg).state_dict().items()}
        assert got == want, (tag, sorted(set(want) ^ set(got))[:6])
    for tag, (cfg, _, _) in HPX_SWIN_CASES.items():
        g = load_golden(f"model_{tag}")
        want = {k: (tuple(s), d) for k, s, d in json.loads(str(g["state_spec"]))}
        got = {k: (tuple(v.shape), str(v.dtype).replace("torch.", ""))
               for k, v in M.SwinTransformerHPX(**cfg).state_dict().items()}
        assert got == want, (tag, sorted(set(want) ^ set(got))[:6])


def test_healpix_gather_table_reproduces_reference_padding():
    """Host logic of the HEALPix row: the gather table (dlwp_benchmark_amd/healpix.py), applied with plain
    indexing on the CPU, reproduces the real reference HEALPixPadding outputs bit for bit."""
    import torch

    from dlwp_benchmark_amd import weights as W
    from dlwp_benchmark_amd.healpix import pad_table
    from helpers import load_golden
    from oracle.make_golden import HPX_PAD_CASES

    for tag, (b, c, h, w, p) in HPX_PAD_CASES.items():
        x = W.normal(f"golden/hpxpad/{tag}/x", (b * 12, c, h, w), 1.0)
        t = pad_table(h, w, p).long()
        assert t.shape == (12, (h + 2 * p) * (w + 2 * p), 2) and int(t[..., 0].min()) >= 0 and int(t.max()) < 12 * h * w
        xs = x.reshape(b, 12, c, h * w).permute(0, 2, 1, 3).reshape(b, c, 12 * h * w)
        ia, ib = t[..., 0].reshape(-1), t[..., 1].reshape(-1)
        va, vb = xs[:, :, ia], xs[:, :, ib.clamp(min=0)]
        y = torch.where(ib >= 0, 0.5 * va + 0.5 * vb, va)
        y = y.reshape(b, c, 12, h + 2 * p, w + 2 * p).permute(0, 2, 1, 3, 4).reshape(b * 12, c, h + 2 * p, w + 2 * p)
        assert torch.equal(y, torch.from_numpy(load_golden(f"healpix_pad_{tag}")["y"])), tag
