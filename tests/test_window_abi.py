"""include/icer_hip_dec_window.h (the window decode's prototypes, included by icer_hip_dec.h) against the one declaration
table of the package, with the checks of tests/test_abi.py; the product library exports every one of them, and a C program
that includes icer_hip_dec.h alone sees them.  CPU only."""
import os
import subprocess

from tests.test_abi import ROOT, _declared_functions, _prototypes, _table_problems

HEADER = "icer_hip_dec_window.h"
NAMES = ["icerx_decode_host_window", "icerx_decode_device_window", "icerx_decode_device_window_display",
         "icerx_decode_window_workspace_bytes", "icerx_decode_device_window_async", "icerx_decode_window_display_workspace_bytes",
         "icerx_decode_device_window_display_async", "icerx_decompress_window"]


def test_window_prototypes_are_declared_once_in_the_table():
    from icer_compression_amd import _abi
    protos = _prototypes(HEADER)
    assert sorted(protos) == sorted(NAMES) == _declared_functions(HEADER)
    assert _table_problems(HEADER, _abi.DECODER) == []
    assert not set(NAMES) & set(_prototypes("icer_hip_dec.h")), "declared twice"


def test_library_exports_the_window_calls():
    from icer_compression_amd import _abi, decoder
    lib = decoder.load_library()
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes == list(_abi.DECODER[n][1]), n


def test_the_decoder_header_brings_the_window_calls(tmp_path):
    src = tmp_path / "uses_window.c"
    src.write_text('#include "icer_hip_dec.h"\nint main(void) { return icerx_decode_window_workspace_bytes(0, 0, 0, 0) != 0 || '
                   '(void *)icerx_decompress_window == 0 || (void *)icerx_decode_device_window_display_async == 0; }\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_window_header_refuses_to_be_included_alone(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "icer_hip_dec_window.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "include icer_hip_dec.h" in r.stderr, r.stderr
