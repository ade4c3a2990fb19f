"""include/icer_hip_dec_session.h (the decode sessions' prototypes, included by icer_hip_dec.h) against the one declaration table
of the package, with the checks of tests/test_abi.py; the product library exports every one of them, and a C program that
includes icer_hip_dec.h alone sees them.  CPU only."""
import os
import subprocess

from tests.test_abi import ROOT, _declared_functions, _prototypes, _table_problems

HEADER = "icer_hip_dec_session.h"
NAMES = ["icerx_session_create", "icerx_session_destroy", "icerx_session_reset", "icerx_session_feed_host", "icerx_session_feed_device",
         "icerx_session_feed_device_display", "icerx_session_planes_held", "icerx_session_stats"]


def test_session_prototypes_are_declared_once_in_the_table():
    from icer_compression_amd import _abi
    protos = _prototypes(HEADER)
    assert sorted(protos) == sorted(NAMES) == _declared_functions(HEADER)
    assert _table_problems(HEADER, _abi.DECODER) == []
    assert not set(NAMES) & set(_prototypes("icer_hip_dec.h")), "declared twice"


def test_library_exports_the_session_calls():
    from icer_compression_amd import _abi, decoder
    lib = decoder.load_library()
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes == list(_abi.DECODER[n][1]), n


def test_the_decoder_header_brings_the_session_calls(tmp_path):
    src = tmp_path / "uses_session.c"
    src.write_text('#include "icer_hip_dec.h"\nint main(void) { icerx_session *s = 0; return icerx_session_reset(s, -1) != 0 || '
                   '(void *)icerx_session_feed_device_display == 0 || (void *)icerx_session_stats == 0; }\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_session_header_refuses_to_be_included_alone(tmp_path):
    src = tmp_path / "alone.c"
    src.write_text('#include <stddef.h>\n#include <stdint.h>\n#include "icer_hip_dec_session.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "include icer_hip_dec.h" in r.stderr, r.stderr


def test_python_session_wraps_every_call():
    from icer_compression_amd import decoder
    for method in ("feed_host", "feed_device", "feed_torch", "reset", "planes_held", "stats", "close"):
        assert callable(getattr(decoder.Session, method)), method
