"""The workspace a caller must hand the six calls on stored masters (icerx_recut_workspace_bytes, _cuts_, _roi_, _target_, _budget_
and icerx_combine_workspace_bytes) is part of what callers see: the sizes are pinned here, on the CPU build of decoder.hip against
tests/emu/hip_mock_async.h (as tests/test_recut_mock.py builds it).  Two geometries, a plain and a quality recutter, n in {1, 3},
two cuts.  The literals were taken by running these same calls on the build of the commit before the recutter's calls were put
on one call record and one driver; a layout change that moves one of them is a change callers have to be told about.  CPU only."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N_CUTS = 2

# (recutter arguments, {n: (data_bytes, recut, cuts, roi, target, budget, combine)}); a plain recutter has no target or budget call: 0
CASES = {
    "gray16": (dict(w=64, h=48, channels=1, stages=2, segments=2, bits=16, max_reduce=1),
               {1: (1007, 12032, 14592, 20224, 0, 0, 13056), 3: (3007, 28928, 36096, 51968, 0, 0, 32512)}),
    "yuv8_quality": (dict(w=128, h=96, channels=3, stages=3, segments=5, bits=8, max_reduce=2, filt=0),
                     {1: (1007, 46080, 67584, 110336, 88064, 105472, 59392), 3: (3007, 131072, 195328, 322304, 256256, 307712, 170496)}),
}


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_recut_sizes") / "libdecoder_mock_recut_sizes.so")
    subprocess.check_call(["g++", "-x", "c++", "-O0", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                           "-DICER_HOST_MOCK", "-DICER_WAVE_EMU", "-include", os.path.join(HERE, "emu", "hip_mock_async.h"),
                           "-o", lib_path, os.path.join(ROOT, "icer_compression_amd", "csrc", "decoder.hip")])
    return decoder.bind(lib_path)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n", [1, 3])
def test_workspace_sizes_are_the_recorded_ones(mock_lib, name, n):
    from icer_compression_amd import decoder
    kw, expected = CASES[name]
    r = decoder.Recutter(lib=mock_lib, **kw)
    try:
        data_bytes = expected[n][0]
        got = (r.workspace_bytes(n, data_bytes, N_CUTS), r.cuts_workspace_bytes(n, data_bytes, N_CUTS), r.roi_workspace_bytes(n, data_bytes, N_CUTS),
               r.target_workspace_bytes(n, data_bytes, N_CUTS), r.budget_workspace_bytes(n, data_bytes, N_CUTS),
               r.combine_workspace_bytes(n, data_bytes))
    finally:
        r.close()
    print(name, n, got)
    assert got == expected[n][1:]
