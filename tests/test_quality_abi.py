"""include/icer_hip_sidecar.h and include/icer_hip_dec_quality.h (the prototypes of the distortion sidecar and of the
quality-driven re-cuts, included by icer_hip.h and icer_hip_dec.h) against the one declaration table of the package, with the
checks of tests/test_abi.py; the product libraries export every one of them, and a C program that includes icer_hip_dec.h alone
sees them.  CPU only."""
import os
import subprocess

import pytest

from tests.test_abi import ROOT, _declared_functions, _prototypes, _table_problems

PARTS = {
    "icer_hip_sidecar.h": ("icer_hip.h", "ENCODER", ["icerx_distortion_sidecar_entries", "icerx_get_distortion_sidecar_device"]),
    "icer_hip_dec_quality.h": ("icer_hip_dec.h", "DECODER", [
        "icerx_recutter_create_quality", "icerx_recut_sidecar_entries", "icerx_recut_target_threshold", "icerx_recut_target_workspace_bytes",
        "icerx_recut_device_target_async", "icerx_recut_budget_workspace_bytes", "icerx_recut_device_budget_async"]),
}


@pytest.mark.parametrize("header", list(PARTS))
def test_prototypes_are_declared_once_in_the_table(header):
    from icer_compression_amd import _abi
    whole, table, names = PARTS[header]
    protos = _prototypes(header)
    assert sorted(protos) == sorted(names) == _declared_functions(header)
    assert _table_problems(header, getattr(_abi, table)) == []
    assert not set(names) & set(_prototypes(whole)), "declared twice"


def test_libraries_export_the_calls():
    from icer_compression_amd import _abi, api, decoder
    for lib, table, names in ((api.load_library(), _abi.ENCODER, PARTS["icer_hip_sidecar.h"][2]),
                              (decoder.load_library(), _abi.DECODER, PARTS["icer_hip_dec_quality.h"][2])):
        for n in names:
            assert hasattr(lib, n) and getattr(lib, n).argtypes == list(table[n][1]), n


def test_the_decoder_header_brings_both_parts(tmp_path):
    src = tmp_path / "uses_quality.c"
    src.write_text('#include "icer_hip_dec.h"\nint main(void) { return icerx_recut_sidecar_entries(0) != icerx_distortion_sidecar_entries(0) || '
                   '(void *)icerx_recut_device_target_async == 0 || (void *)icerx_recut_device_budget_async == 0 || '
                   '(void *)icerx_get_distortion_sidecar_device == 0 || (void *)icerx_recutter_create_quality == 0; }\n')
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


@pytest.mark.parametrize("header", list(PARTS))
def test_a_part_refuses_to_be_included_alone(tmp_path, header):
    src = tmp_path / "alone.c"
    src.write_text(f'#include <stddef.h>\n#include <stdint.h>\n#include "{header}"\nint main(void) {{ return 0; }}\n')
    r = subprocess.run(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and f"include {PARTS[header][0]}" in r.stderr, r.stderr
