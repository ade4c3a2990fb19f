"""Decode sessions (include/icer_hip_dec_session.h; csrc/decoder_session.hpp) end to end on the CPU: decoder.hip compiled by g++
against tests/emu/hip_mock_async.h as tests/test_display_mock.py builds it, driven through decoder.Session -- icerx_session_feed_device
on host arrays (the mock's device memory) and icerx_session_feed_host -- against tests/session_model.py.  The scenarios are those
of tests/session_cases.py, which tests/test_gpu_session.py runs on the GPU; here they also run with ICER_DEC_WAVE=0, where every
chain takes the thread-per-chain kernel.  CPU only."""
import subprocess

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import session_cases as sc
from tests import session_model as sm
from tests.test_display_mock import DECODER_HIP, MOCK_FLAGS


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


@pytest.fixture(scope="module")
def mock_lib(tmp_path_factory):
    from icer_compression_amd import decoder
    lib_path = str(tmp_path_factory.mktemp("mock_session") / "libdecoder_mock_session.so")
    subprocess.check_call(["g++"] + MOCK_FLAGS + ["-O2", "-fPIC", "-shared", "-o", lib_path, DECODER_HIP])
    return decoder.bind(lib_path)


class Rig:
    """sessions of the mock build; host=True feeds through icerx_session_feed_host"""

    def __init__(self, lib, orc, host=False):
        self.lib, self.orc, self.host, self.keep = lib, orc, host, []

    def open(self, name, n_slots=1, reduce=0, reconstruct=0, display=False):
        from icer_compression_amd import decoder
        g, _ = sc.CASES[name]
        rw, rh = red.reduced_size(g.w, g.h, reduce)
        dec = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits, lib=self.lib, reduce=reduce, reconstruct=reconstruct)
        ses = decoder.Session(dec, n_slots, rw * rh)
        self.keep.append(dec)
        return ses, sm.SessionModel(self.orc, g.channels, g.stages, g.filt, g.segments, rw * rh, g.bits, reduce, reconstruct, n_slots)

    def feed(self, ses, feeds, slots=None, display=False, sizes=None):
        n, ch, stride = len(feeds), ses.channels, ses.frame_stride
        if self.host and not display:
            rc, res = ses.feed_host(feeds, slots, sizes)
            assert rc == 0
            # (feed_host hands out zeroed planes: a frame that delivers nothing must leave them zero)
            rows = [np.concatenate(r[3]) for r in res]
            for k, r in enumerate(res):
                if r[0] in (sm.INVALID_INPUT, sm.QUOTA) or r[1] * r[2] == 0:
                    assert not rows[k].any()
                    rows[k] = np.full_like(rows[k], sc.SENT if rows[k].dtype == np.uint8 else sc.SENT * 0x0101)
            return [r[0] for r in res], [r[1] for r in res], [r[2] for r in res], rows
        dt = np.uint8 if display or ses.bits == 8 else np.uint16
        out = np.full(n * ch * stride + 64, sc.SENT if dt == np.uint8 else sc.SENT * 0x0101, dt)
        lens = [len(f) for f in feeds]
        offs = [sum(lens[:k]) + 3 for k in range(n)]
        blob = np.frombuffer(b"\x5b\x60\x00" + b"".join(feeds) + b"\x5b" * 5, np.uint8).copy()
        keep = blob.copy()
        rc, rcs, ws, hs = ses.feed_device(n, blob.ctypes.data, offs, lens, out.ctypes.data, slots, sizes, display)
        assert rc == 0 and np.array_equal(blob, keep)
        assert (out[n * ch * stride:] == out[-1]).all(), "written behind the n rows"
        return rcs, ws, hs, [out[k * ch * stride: (k + 1) * ch * stride] for k in range(n)]


@pytest.fixture(params=["", "0"], ids=["planes", "threads"])
def dec_wave(request, monkeypatch):
    monkeypatch.setenv("ICER_DEC_WAVE", request.param)
    return request.param


@pytest.mark.parametrize("name", list(sc.CASES))
def test_ladder_of_three_steps(mock_lib, expected, oracle, dec_wave, name):
    ses, mod = sc.run_ladder(Rig(mock_lib, oracle), expected, oracle, name)
    resumed, threads, planes, _ = ses.stats()
    assert planes > 0 and (resumed > 0 if dec_wave == "" else (resumed == 0 and threads > 0)), (name, ses.stats())


def test_the_gpu_cases_resume_chains_in_the_wave_per_plane_kernel(mock_lib, expected, oracle, monkeypatch):
    """the routing of every case of tests/test_gpu_session.py, checked where it can be without a GPU"""
    monkeypatch.delenv("ICER_DEC_WAVE", raising=False)
    for name in sc.CASES:
        ses, _ = sc.run_ladder(Rig(mock_lib, oracle), expected, oracle, name)
        assert ses.stats()[0] > 0, name


def test_ladder_through_the_host_call(mock_lib, expected, oracle, dec_wave):
    sc.run_ladder(Rig(mock_lib, oracle, host=True), expected, oracle, "gray16_A4")


@pytest.mark.parametrize("options", [dict(reduce=1), dict(reconstruct=3), dict(display=True), dict(reduce=1, reconstruct=3)],
                         ids=["reduce1", "recon3", "display", "reduce1_recon3"])
def test_decoder_options(mock_lib, expected, oracle, dec_wave, options):
    sc.run_ladder(Rig(mock_lib, oracle), expected, oracle, "gray16_A4", **options)


def test_yuv_display_and_reconstruction(mock_lib, expected, oracle):
    sc.run_ladder(Rig(mock_lib, oracle), expected, oracle, "yuv8", reconstruct=3)


def test_roi_cut_then_quota_cut(mock_lib, expected, oracle, dec_wave):
    sc.run_roi_then_quota(Rig(mock_lib, oracle), expected)


def test_slots_reset_size_mismatch_duplicate(mock_lib, expected, oracle, dec_wave):
    sc.run_slots(Rig(mock_lib, oracle), expected)
    sc.run_slots(Rig(mock_lib, oracle, host=True), expected)


def test_damaged_packet_in_an_increment(mock_lib, expected, oracle, dec_wave):
    sc.run_damaged_increment(Rig(mock_lib, oracle), expected)


def test_a_plane_that_fails_stops_its_chain_for_good(mock_lib, expected, oracle, dec_wave):
    """the packet: a header's data_length cut to one bit, both CRCs recomputed; the decoder oracle stops the chain there"""
    sc.run_failing_plane(Rig(mock_lib, oracle), expected, oracle)


def test_refused_arguments(mock_lib, oracle):
    rig = Rig(mock_lib, oracle)
    ses, _ = rig.open("gray16_A4", n_slots=2)
    out = np.zeros(2 * ses.frame_stride, np.uint16)
    blob = np.zeros(8, np.uint8)
    for slots in ([0, 0], [0, 2], [-1, 1]):
        assert ses.feed_device(2, blob.ctypes.data, [0, 0], [0, 0], out.ctypes.data, slots)[0] == sm.INVALID_INPUT
    assert ses.feed_device(3, blob.ctypes.data, [0] * 3, [0] * 3, out.ctypes.data)[0] == sm.INVALID_INPUT
    assert ses.feed_device(1, blob.ctypes.data, [0], [0], None)[0] == sm.INVALID_INPUT
    assert ses.planes_held(5, 0, 1, 1, 0) == -2 and ses.planes_held(0, 0, 9, 1, 0) == -2 and ses.stats() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        ses.reset(7)
