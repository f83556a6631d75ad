"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/lgs_engine.h declares (no compute calls without a GPU), and the product path fails loudly."""
import ctypes
import os
import re
import struct

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lgs_[a-z0-9_]+)\s*\(", txt)))


def header_abi_version():
    txt = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    return int(re.search(r"#define\s+LGS_ABI_VERSION\s+(\d+)", txt).group(1))


def test_documented_build_entry_point_runs():
    """`python -c "import __graft_entry__ as g; g.build()"` is what README.md / INTEGRATION.md print and what the driver
    calls: it must run (round 3 shipped it with a stale ABI literal and nothing called it)."""
    import __graft_entry__ as g
    path = g.build()
    assert os.path.exists(path) and path.endswith("liblgs_engine.so")
    assert os.path.exists(os.path.join(ROOT, "oracle", "liboracle.so"))


def test_library_exports_every_declared_symbol():
    from languagegroundedsemseg_amd import build, engine
    path = build.build()
    L = ctypes.CDLL(path)
    syms = declared_symbols()
    assert len(syms) >= 19
    for s in syms:
        assert hasattr(L, s), "missing export " + s
    assert sorted(engine.EXPORTS) == syms, "engine.EXPORTS out of sync with the header"
    assert engine.lib().lgs_abi_version() == engine.ABI_VERSION == header_abi_version()


def declared_prototypes():
    """-> {name: (return kind, [param kinds])} parsed from the header; kinds: ptr / int / i64 / f32 / f64"""
    txt = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)

    def kind(decl):
        decl = decl.strip()
        if "*" in decl:
            return "ptr"
        base = re.sub(r"\b(const|unsigned|signed)\b", " ", decl).split()
        assert base, decl
        t = base[0]
        return {"int": "int", "int64_t": "i64", "float": "f32", "double": "f64", "int32_t": "int"}[t]

    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \t\n\*]*?)\b(lgs_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        ret = re.split(r"[;{}]", ret)[-1]
        if "typedef" in ret or "struct" in ret:
            continue
        plist = [] if params in ("", "void") else [kind(x) for x in params.split(",")]
        protos[name] = (kind(ret), plist)
    return protos


def _ctype_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents") or issubclass(t, ctypes._Pointer):
        return "ptr"
    return {ctypes.c_int: "int", ctypes.c_int64: "i64", ctypes.c_float: "f32", ctypes.c_double: "f64", ctypes.c_int32: "int"}[t]


def test_ctypes_signatures_match_the_header_prototypes():
    """arity and argument classes (pointer / int / int64 / float) of every binding in engine.py against the C prototypes:
    a drifted argtype (e.g. an `int` row stride bound as int64) passes garbage in the upper register half silently"""
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    protos = declared_prototypes()
    assert sorted(protos) == declared_symbols(), "prototype parser missed a declaration"
    for name, (ret, params) in protos.items():
        f = getattr(L, name)
        assert f.argtypes is not None, "engine.py binds %s without argtypes" % name
        got = [_ctype_kind(t) for t in f.argtypes]
        assert got == params, "%s: engine.py argtypes %s != header %s" % (name, got, params)
        assert _ctype_kind(f.restype) == ret, "%s: restype %s != header %s" % (name, _ctype_kind(f.restype), ret)


def declared_struct(name):
    """-> [(member, kind)] of `typedef struct name {...} name;` in the header; kinds: ptr / int / i64 / f32, or the type name of a
    nested struct"""
    txt = open(os.path.join(ROOT, "include", "lgs_engine.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S).group(1)
    members = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"((?:const\s+)?\w+)\s+(.*)", decl, flags=re.S).groups()
        base = base.replace("const", "").strip()
        for item in rest.split(","):
            item = item.strip()
            kind = "ptr" if item.startswith("*") else {"int": "int", "int64_t": "i64", "float": "f32"}.get(base, base)
            members.append((item.lstrip("* "), kind))
    return members


def test_ctypes_structs_match_the_header_structs():
    """member names, order and kinds of the structs the host packs by position (the block arguments, their nested norm
    parameters, the pack descriptor) against the header, and the struct-module formats derived from the ctypes classes against
    the ctypes layouts: a member added on one side only shifts every later value of a positional pack_into"""
    from languagegroundedsemseg_amd import engine
    classes = {"lgs_bn_params": engine.BnParams, "lgs_block_fwd": engine.BlockFwd, "lgs_block_bwd": engine.BlockBwd,
               "lgs_pack_desc": engine.PackDesc}
    nested = {cls: name for name, cls in classes.items()}
    for name, cls in classes.items():
        got = [(f, nested[t] if t in nested else _ctype_kind(t)) for f, t in cls._fields_]
        assert got == declared_struct(name), name
    assert [len(c._fields_) for c in classes.values()] == [7, 31, 58, 14]
    for cls, packer in ((engine.BlockFwd, engine.BLOCK_FWD_PACK), (engine.BlockBwd, engine.BLOCK_BWD_PACK)):
        assert packer.format == "@" + engine.struct_format(cls) and packer.size == ctypes.sizeof(cls)
    for cls in classes.values():
        assert struct.calcsize("@" + engine.struct_format(cls)) == ctypes.sizeof(cls), cls


def test_integration_stub_signatures_match_the_header():
    """the ctypes stub printed in INTEGRATION.md is held to the same check (it once declared an int as int64)"""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    protos = declared_prototypes()
    names = {"vp": "ptr", "i64": "i64", "ci": "int", "cf": "f32"}
    found = 0
    for m in re.finditer(r"L\.(lgs_[a-z0-9_]+)\.argtypes\s*=\s*\[([^\]]*)\]", txt):
        name, args = m.group(1), m.group(2)
        kinds = []
        for a in [x.strip() for x in args.split(",") if x.strip()]:
            kinds.append("ptr" if a.startswith("ctypes.POINTER") else names[a])
        assert kinds == protos[name][1], "INTEGRATION.md stub of %s: %s != header %s" % (name, kinds, protos[name][1])
        found += 1
    assert found >= 5


def test_error_reporting_without_gpu():
    from languagegroundedsemseg_amd import engine
    L = engine.lib()
    # null arguments are rejected before any HIP call
    rc = L.lgs_manager_map_size(None, 0, None, None)
    assert rc != 0
    assert b"bad key" in L.lgs_last_error() or b"lgs_manager_map_size" in L.lgs_last_error()
    with pytest.raises(RuntimeError):
        engine.check(rc)


def test_product_path_has_no_cpu_fallback():
    import MinkowskiEngine as ME
    assert ME.get_backend().name == "hip"
    coords = torch.tensor([[0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP"):
        ME.SparseTensor(torch.zeros(2, 3), coords)


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "languagegroundedsemseg_amd")
    for d in (pkg, os.path.join(ROOT, "MinkowskiEngine")):
        for base, _, files in os.walk(d):
            for f in files:
                if f.endswith(".py"):
                    src = open(os.path.join(base, f)).read()
                    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(base, f)
                    assert "from .. import oracle" not in src and "import oracle" not in src.replace("# oracle", "")


def test_integration_stub_names_the_current_abi_version():
    """INTEGRATION.md once said `lgs_abi_version() == 10` two versions after the header had moved on"""
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    named = [int(v) for v in re.findall(r"lgs_abi_version\(\) == (\d+)", txt)]
    assert named and all(v == header_abi_version() for v in named), named
