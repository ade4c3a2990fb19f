"""CPU-side checks of the drop-in boundary: the shared library loads, exports every symbol that
include/icer_hip.h declares, and the pure-host entry points behave like the reference's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from icer_compression_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions(header="icer_hip.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(icerx?_[a-z0-9_]+)\s*\(", src)))


def _prototypes(header):
    """name -> (return type, [parameter declarations]) of every function the header declares"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(icerx?_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = [p.strip() for p in params.split(",")]
        protos[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return protos


_INTEGERS = (C.c_int, C.c_uint, C.c_int8, C.c_uint8, C.c_int16, C.c_uint16, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64)
_C_WIDTH = {"int": 4, "unsigned": 4, "enum icer_filter_types": 4, "uint8_t": 1, "uint32_t": 4, "int32_t": 4}
_RETURNS = {"int": C.c_int, "void": None, "size_t": C.c_size_t, "uint64_t": C.c_uint64, "const char *": C.c_char_p}


def _is_pointer(ctype):
    return isinstance(ctype, type) and issubclass(ctype, (C._Pointer, C.c_void_p, C.c_char_p, np.ctypeslib._ndptr))


def _parameter_fits(decl, ctype):
    """one C parameter declaration against the ctype the table gives it"""
    if "*" in decl or "[" in decl:
        return _is_pointer(ctype)
    c_type = " ".join(w for w in re.sub(r"\w+$", "", decl).split() if w != "const")       # (without the parameter's name)
    exact = {"size_t": C.c_size_t, "uint64_t": C.c_uint64, "double": C.c_double}
    if c_type in exact:
        return ctype is exact[c_type]
    return ctype in _INTEGERS and C.sizeof(ctype) <= _C_WIDTH[c_type]


def _table_problems(header, table):
    problems = []
    for name, (ret, params) in _prototypes(header).items():
        if name not in table:
            problems.append(f"{name}: no entry")
            continue
        restype, argtypes = table[name]
        if restype is not _RETURNS[ret]:
            problems.append(f"{name}: returns {ret}, declared {restype}")
        if len(argtypes) != len(params):
            problems.append(f"{name}: {len(params)} parameters, {len(argtypes)} declared")
            continue
        problems += [f"{name}: parameter {k} `{decl}` declared {ctype}" for k, (decl, ctype) in enumerate(zip(params, argtypes))
                     if not _parameter_fits(decl, ctype)]
    return problems


@pytest.mark.parametrize("header,table,count", [("icer_hip.h", "ENCODER", 48), ("icer_hip_dec.h", "DECODER", 46)])
def test_declaration_table_matches_the_header(header, table, count):
    """icer_compression_amd/_abi.py against the prototypes: an entry for every function, the parameter count, and per parameter and
    return the kind and width of its C type (an undeclared or narrower one is passed or returned as a 32-bit int, silently)"""
    from icer_compression_amd import _abi
    table = getattr(_abi, table)
    protos = _prototypes(header)
    assert sorted(protos) == _declared_functions(header) and len(protos) == count
    assert _table_problems(header, table) == []
    # the check itself: a deleted entry and a size_t declared c_int are both found
    name = next(n for n, (_, params) in protos.items() if any(p.startswith("size_t ") for p in params))
    k = next(k for k, p in enumerate(protos[name][1]) if p.startswith("size_t "))
    narrowed = list(table[name][1])
    narrowed[k] = C.c_int
    assert _table_problems(header, {**table, name: (table[name][0], narrowed)}) == [f"{name}: parameter {k} `{protos[name][1][k]}` declared {C.c_int}"]
    assert _table_problems(header, {n: e for n, e in table.items() if n != name}) == [f"{name}: no entry"]


def test_library_exports_every_declared_symbol():
    lib = api.load_library()
    names = _declared_functions()
    assert {"icer_init", "icer_init_output_struct", "icer_compress_image_uint16", "icer_compress_image_yuv_uint16",
            "icerx_encoder_create", "icerx_encode_device"} <= set(names)
    for n in names:
        assert hasattr(lib, n), n


def test_decoder_library_exports_every_declared_symbol_and_has_no_cpu_fallback():
    """include/icer_hip_dec.h <-> libicer_hip_dec.so (the decoder)"""
    from icer_compression_amd import decoder
    lib = decoder.load_library()
    names = _declared_functions("icer_hip_dec.h")
    assert {"icer_get_image_dimensions", "icer_decompress_image_uint16", "icer_decompress_image_yuv_uint16",
            "icer_decompress_image_uint8", "icer_decompress_image_yuv_uint8", "icerx_decoder_create", "icerx_decode_host",
            "icerx_decode_device"} <= set(names)
    for n in names:
        assert hasattr(lib, n), n
    # host-only entry point: size fields of the first CRC-valid packet (icer_compress.c:541-566)
    from oracle.binding import Oracle
    rc, stream, _ = Oracle().compress([np.arange(40 * 24, dtype=np.uint16).reshape(24, 40) % 200], 2, 0, 3, 1 << 16)
    assert decoder.icer_get_image_dimensions(stream) == (0, 40, 24)
    assert decoder.icer_get_image_dimensions(b"\x00" * 9 + stream) == (0, 40, 24)
    assert decoder.icer_get_image_dimensions(stream[:27])[0] == decoder.ICER_DECODER_OUT_OF_DATA
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        rc, w, h, _ = decoder.decompress(stream, 1, 2, 0, 3)
        assert rc == api.ICER_FATAL_ERROR and b"no usable HIP device" in lib.icerx_decoder_last_error()


def test_plain_c_decode_program_links(tmp_path):
    """tests/c_abi/dropin_decode_example.c: the reference's decode call sequence against include/icer_hip_dec.h and
    libicer_hip_dec.so.  Without a GPU the image call must fail loudly (exit code 10); with one, the images must equal the
    decoder oracle's."""
    import subprocess
    from oracle.binding import Oracle
    from icer_compression_amd import synth
    from icer_compression_amd.build import build_decoder_library
    exe = str(tmp_path / "dropin_decode_example")
    libdir = os.path.dirname(build_decoder_library())
    subprocess.check_call(["gcc", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_abi", "dropin_decode_example.c"),
                           "-L", libdir, "-licer_hip_dec", "-Wl,-rpath," + libdir, "-o", exe])
    orc = Oracle()
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    for planes, st, f, sg in [([synth.gray_frame(160, 120, 5, 1)], 3, 0, 5), (list(synth.color_frame_yuv(96, 64, 7)), 2, 1, 3)]:
        rc, stream, _ = orc.compress(planes, st, f, sg, 1 << 20)
        (tmp_path / "in.bin").write_bytes(stream)
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(len(planes)), str(st), str(f), str(sg), str(tmp_path / "out.raw")],
                           capture_output=True, text=True)
        if not has_gpu:
            assert r.returncode == 10 and "rc=-10" in r.stdout and "no usable HIP device" in r.stderr, r.stdout + r.stderr
            continue
        h, w = planes[0].shape
        want = orc.decompress(stream, len(planes), st, f, sg)
        assert r.returncode == 0 and f"rc=0 w={w} h={h}" in r.stdout, r.stdout + r.stderr
        got = np.fromfile(tmp_path / "out.raw", "<u2").reshape(len(planes), h * w)
        assert all(np.array_equal(got[c], want[3][c]) for c in range(len(planes)))


def test_output_struct_layout_and_init():
    # icer.h:307-312: four 8-byte fields
    assert C.sizeof(api.icer_output_data_buf_typedef) == 32
    assert api.icer_init() == api.ICER_RESULT_OK
    out = api.icer_output_data_buf_typedef()
    buf = np.zeros(1000, np.uint8)
    assert api.icer_init_output_struct(out, buf, 1000, 501) == api.ICER_OUTPUT_BUF_TOO_SMALL     # icer_util.c:39
    assert api.icer_init_output_struct(out, buf, 1000, 500) == api.ICER_RESULT_OK
    assert (out.size_used, out.size_allocated) == (0, 500)
    assert out.data_start == buf.ctypes.data and out.rearrange_start == buf.ctypes.data + 500


def test_geometry_is_refused_like_the_reference_before_touching_the_gpu():
    lib = api.load_library()
    h = C.c_void_p()
    # final LL thinner than 3 -> ICER_TOO_MANY_STAGES (icer_wavelet.c:63-68)
    assert lib.icerx_encoder_create(C.byref(h), 0, 32, 32, 1, 5, 0, 4, 1) == api.ICER_TOO_MANY_STAGES
    assert lib.icerx_encoder_create(C.byref(h), 0, 64, 64, 2, 2, 0, 4, 1) == api.ICER_INVALID_INPUT


def test_no_cpu_fallback():
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    rc, stream, _ = api.compress([np.zeros((64, 64), np.uint16)], 2, 0, 4, 1 << 16)
    assert rc == api.ICER_FATAL_ERROR and stream == b""
    assert b"no usable HIP device" in api.load_library().icerx_last_error()
