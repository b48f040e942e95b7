"""The C-ABI library loads without a GPU and exports every symbol include/isegmi.h declares; host-only
entry points (weight packing, descriptor validation, error reporting) behave; nothing computes on a GPU here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "isegmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(isegmi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from isegmi import _ffi
    lib = _ffi.lib()
    syms = declared_symbols()
    assert len(syms) >= 40
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.isegmi_version() == 1


def test_missing_library_fails_loudly(monkeypatch):
    from isegmi import _ffi
    monkeypatch.setattr(_ffi, "_lib", None)
    monkeypatch.setattr(_ffi, "LIB_PATH", "/nonexistent/libisegmi.so")
    with pytest.raises(_ffi.IsegmiError, match="no CPU fallback"):
        _ffi.lib()


def test_pack_weights_layout_and_validation():
    from isegmi import _ffi
    d = _ffi.make_conv_desc(1, 8, 8, 32, 5, 1, 1)
    w = np.arange(5 * 32, dtype=np.float32).reshape(5, 1, 1, 32)
    p = _ffi.pack_conv_weights(d, w).reshape(128, 32)   # Cout padded to 128 rows
    assert not p[5:].any()
    # inside each group of 8 consecutive k: [k0 k2 k4 k6 | k1 k3 k5 k7]
    assert list(p[1, :8]) == [32, 34, 36, 38, 33, 35, 37, 39]
    assert sorted(p[3]) == list(range(96, 128))
    stem = _ffi.make_conv_desc(1, 32, 32, 4, 64, 7, 7, 2, 3)
    ps = _ffi.pack_conv_weights(stem, np.ones((64, 7, 7, 4), np.float32)).reshape(128, 7, 32)
    assert ps[0].sum() == 7 * 28 and ps[0, 0].sum() == 28  # 28 real taps + 4 zero pads per kernel row
    assert _ffi.conv_out_hw(stem) == (16, 16)
    bad = _ffi.make_conv_desc(1, 8, 8, 24, 5, 1, 1)  # Cin not a multiple of 32
    with pytest.raises(_ffi.IsegmiError, match="Cin"):
        _ffi.conv_out_hw(bad)
    assert b"Cin" in _ffi.lib().isegmi_last_error()


def test_no_device_is_an_error_not_a_fallback():
    from isegmi import _ffi
    if _ffi.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_ffi.IsegmiError):
        _ffi.DeviceBuffer((16,))


# ---------------------------------------------------------------------------------------------------------------------------------------
# The ctypes declaration of the ABI (isegmi/_abi.py) against include/isegmi.h, and every call site against the declaration.
PKG_DIR = os.path.join(ROOT, "instancesegmentation-jittor_amd", "isegmi")
_BY_VALUE = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_FIELD = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
HANDLE_ONLY = {"isegmi_engine", "isegmi_comm"}
_STRUCT = r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;"
_FORWARD = r"typedef\s+struct\s+(\w+)\s+(\w+)\s*;"


def _header():
    """include/isegmi.h without comments -> (text, {macro: int})"""
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "isegmi.h")).read(), flags=re.S)
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(\w+)\s+(\d+)\s*$", src, flags=re.M)}
    return src, macros


def _ctype_of(decl, is_return=False):
    """The one mechanical rule of _abi.py's docstring; raises on anything it cannot classify."""
    decl = " ".join(decl.split())
    if "*" in decl:
        if re.fullmatch(r"const char ?\*( ?\w+)?", decl):
            return C.c_char_p
        assert not is_return, "pointer return other than const char*: " + decl
        return C.c_void_p
    tokens = decl.split()
    if len(tokens) != (1 if is_return else 2) or tokens[0] not in _BY_VALUE:
        raise AssertionError("cannot classify %r" % decl)
    return _BY_VALUE[tokens[0]]


def header_prototypes():
    src, _ = _header()
    src = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("#"))
    src = re.sub(_STRUCT, " ", src, flags=re.S)
    src = re.sub(_FORWARD, " ", src)
    out = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.replace('extern "C" {', " ").split())
        if stmt in ("", "}"):
            continue
        m = re.fullmatch(r"(.*?)\b(isegmi_\w+) ?\((.*)\)", stmt)
        assert m, "not a prototype: %r" % stmt
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in out, name
        out[name] = (_ctype_of(ret, True), [] if params == "void" else [_ctype_of(p) for p in params.split(",")])
    return out


def test_signature_table_matches_the_header():
    from isegmi import _abi
    protos = header_prototypes()
    assert len(protos) >= 140 and sorted(protos) == declared_symbols()
    assert sorted(_abi.SIGNATURES) == sorted(protos), (set(_abi.SIGNATURES) ^ set(protos))
    wrong = {n: (_abi.SIGNATURES[n], protos[n]) for n in protos if (_abi.SIGNATURES[n][0], list(_abi.SIGNATURES[n][1])) != protos[n]}
    assert not wrong, wrong


def header_structs():
    """{struct name: [(field, ctypes type)]} in declaration order; raises on a field it cannot classify."""
    src, macros = _header()
    out = {}
    for m in re.finditer(_STRUCT, src, flags=re.S):
        assert m.group(1) == m.group(3), m.group(0)[:60]
        fields = []
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            if "*" in decl:
                base, names = C.c_void_p, decl[decl.rindex("*") + 1:]
            else:
                tname, _, names = decl.partition(" ")
                assert tname in _FIELD, "cannot classify field %r of %s" % (decl, m.group(1))
                base = _FIELD[tname]
            for nm in names.split(","):
                f = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", nm.strip())
                assert f, "cannot classify field %r of %s" % (decl, m.group(1))
                n = f.group(2)
                fields.append((f.group(1), base if n is None else base * (int(n) if n.isdigit() else macros[n])))
        out[m.group(1)] = fields
    return out


def test_structures_match_the_header():
    from isegmi import _abi, _ffi
    src, _ = _header()
    structs = header_structs()
    forward = {m.group(1) for m in re.finditer(_FORWARD, src)}
    assert forward == HANDLE_ONLY and len(structs) == 9
    assert sorted(_abi.STRUCTS) == sorted(structs)
    for name, fields in structs.items():
        cls = _abi.STRUCTS[name]
        assert getattr(_ffi, cls.__name__) is cls          # _ffi re-exports the mirrors
        assert list(cls._fields_) == fields, name
        off = align = 0
        for _, t in fields:
            elem = getattr(t, "_type_", t) if hasattr(t, "_length_") else t
            a = C.sizeof(elem)
            align = max(align, a)
            off = -(-off // a) * a + C.sizeof(t)
        assert C.sizeof(cls) == -(-off // align) * align, name


def _python_files():
    for top in (PKG_DIR, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")):
        for d, _, names in os.walk(top):
            for n in sorted(names):
                if n.endswith(".py"):
                    yield os.path.join(d, n)
    yield os.path.join(ROOT, "bench.py")


def _starred_len(node):
    """How many arguments `*node` contributes, when the source says so: a list / tuple display, or a comprehension over one."""
    import ast
    if isinstance(node, (ast.List, ast.Tuple)) and not any(isinstance(e, ast.Starred) for e in node.elts):
        return len(node.elts)
    if isinstance(node, (ast.ListComp, ast.GeneratorExp)) and len(node.generators) == 1 and not node.generators[0].ifs:
        it = node.generators[0].iter
        if isinstance(it, ast.Call) and isinstance(it.func, ast.Name) and it.func.id == "range" and len(it.args) == 1 and isinstance(it.args[0], ast.Constant):
            return int(it.args[0].value)
        return _starred_len(it)
    return None


def call_sites():
    """-> (checked [(where, name, positional count)], unchecked [where]) of every `<expr>.isegmi_*(...)` call in the project's Python."""
    import ast
    checked, unchecked = [], []
    for path in _python_files():
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("isegmi_")):
                continue
            where = "%s:%d %s" % (os.path.relpath(path, ROOT), node.lineno, node.func.attr)
            assert not node.keywords, where + ": keyword argument in a C call"
            n = 0
            for a in node.args:
                k = _starred_len(a.value) if isinstance(a, ast.Starred) else 1
                if k is None:
                    n = None
                    break
                n += k
            if n is None:
                unchecked.append(where)
            else:
                checked.append((where, node.func.attr, n))
    return checked, unchecked


def test_call_sites_match_the_table():
    from isegmi import _abi
    checked, unchecked = call_sites()
    bad = ["%s: %d arguments, %s" % (w, n, "declared %d" % len(_abi.SIGNATURES[name][1]) if name in _abi.SIGNATURES else "not in the table")
           for w, name, n in checked if name not in _abi.SIGNATURES or n != len(_abi.SIGNATURES[name][1])]
    msg = "\n".join(bad) + "\nunchecked (starred, not countable): " + ", ".join(unchecked)
    assert not bad, msg
    assert len(checked) >= 250 and len(unchecked) * 10 <= len(checked) + len(unchecked), msg


def test_declared_means_strict():
    from isegmi import _ffi
    lib = _ffi.lib()
    set_device = lib.isegmi_set_device      # by name: the arity test below reads every direct call in this file too
    with pytest.raises(TypeError):
        set_device()
    with pytest.raises(C.ArgumentError):
        set_device(1.5)
    assert lib.isegmi_op_roi_table_bytes(2, 1000, 7, 7) == 2 * 1000 * 29 * 16
    big = lib.isegmi_op_roi_table_bytes(1 << 15, 1 << 12, 7, 7)
    assert type(big) is int and big == (1 << 27) * 29 * 16 > 1 << 31
    assert isinstance(lib.isegmi_last_error(), bytes)


def test_missing_symbol_is_named(monkeypatch):
    from isegmi import _abi, _ffi
    monkeypatch.setattr(_ffi, "_lib", None)
    monkeypatch.setitem(_abi.SIGNATURES, "isegmi_no_such_entry_point", (C.c_int, []))
    with pytest.raises(_ffi.IsegmiError, match="isegmi_no_such_entry_point"):
        _ffi.lib()


@pytest.mark.parametrize("case", ["d_out", "d_rois", "fixed_level"])
def test_roi_align_refuses_null_and_level_before_any_launch(case):
    """Host-side argument arrays are valid, the device pointers are made-up addresses that nothing dereferences: the launcher returns before it reads
    d_feats[level] or launches (no HIP allocation, no kernel)."""
    from isegmi import _ffi
    lib = _ffi.lib()
    nlevels, fake = 1, 0x10000
    feats = (C.c_void_p * nlevels)(fake)
    Hs, Ws, scales = (C.c_int32 * nlevels)(8), (C.c_int32 * nlevels)(8), (C.c_float * nlevels)(0.25)
    a = dict(d_rois=fake, d_out=fake, fixed_level=-1)
    a[case] = nlevels if case == "fixed_level" else None
    rc = lib.isegmi_op_roi_align(feats, Hs, Ws, scales, nlevels, a["d_rois"], fake, 1, 4, 32, 7, 7, 2, 0, 2, a["fixed_level"], a["d_out"], None, None)
    assert rc != 0
    err = lib.isegmi_last_error()
    assert b"roi_align args" in err and b"fixed_level < nlevels" in err, err


@pytest.mark.parametrize("sampling", [0, -1])
def test_roi_align_f16_refuses_an_adaptive_grid_before_any_launch(sampling):
    """No fp16 kernel has the adaptive grid (their sample loops run iy < g): with sampling <= 0 every RoI would pool to 0 / 0.  Only this entry point used to
    refuse it, inside its unnamed "args" check; now the launcher -- the entry the engines call -- does, and names the reason.  Device pointers are made-up
    addresses that nothing dereferences."""
    from isegmi import _ffi
    lib = _ffi.lib()
    fake = 0x10000
    feats = (C.c_void_p * 1)(fake)
    Hs, Ws, scales = (C.c_int32 * 1)(8), (C.c_int32 * 1)(8), (C.c_float * 1)(0.25)
    rc = lib.isegmi_op_roi_align_f16(feats, Hs, Ws, scales, 1, fake, fake, 1, 4, 64, 7, 7, sampling, 1, 2, fake, None)
    assert rc != 0
    err = lib.isegmi_last_error()
    assert b"roi_align_f16: a fixed sampling grid only" in err and b"g > 0" in err, err


ENGINE_SHARED = ("_create", "set_param", "_set_conv_krsc", "_set_conv_grouped", "_set_tensor", "sync", "stream", "fetch", "timings", "memory",
                 "conv_stats", "_buffer_info", "input_buffer", "upload_async", "_u8_staging", "_preprocess_u8", "mark_step", "wait_mark", "step_times",
                 "rle_device", "coco_record_bytes", "pack_coco_records", "download_async", "download_fence", "download_wait", "close", "__del__")
# the deliberate overrides: a box-only R-CNN engine (and RetinaNet with it) refuses rle_device by name; Pose2Seg.close also frees its staging buffers
ENGINE_OVERRIDES = {("MaskRCNN", "rle_device"), ("RetinaNet", "rle_device"), ("Pose2Seg", "close")}


def test_one_engine_base():
    import ast
    from isegmi.engine import Engine
    from isegmi.maskrcnn import MaskRCNN
    from isegmi.pose2seg import Pose2Seg
    from isegmi.retinanet import RetinaNet
    from isegmi.yolact import Yolact
    for cls in (Yolact, MaskRCNN, RetinaNet, Pose2Seg):
        assert issubclass(cls, Engine)
        for name in ENGINE_SHARED:
            own = getattr(cls, name) is not getattr(Engine, name)
            assert own == ((cls.__name__, name) in ENGINE_OVERRIDES), (cls.__name__, name)
    tree = ast.parse(open(os.path.join(PKG_DIR, "maskrcnn.py")).read())
    imported = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names] + \
               [(n.module or "") for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
    assert not [m for m in imported if "yolact" in m], imported
