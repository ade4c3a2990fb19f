"""Decode sessions on the GPU (include/icer_hip_dec_session.h; csrc/decoder_session.hpp, the resume variants of
csrc/decoder_planes.hpp and decoder_core.hpp) through decoder.Session.feed_torch.  Per case of tests/session_cases.py a lossless
master is re-cut to three nested quotas by Recutter.recut, the increments are formed by Recutter.combine (combine_torch) and fed
in order: after every step image, size and rc are the decoder oracle's for that cut, and the counts show that chains were resumed
in the wave-per-plane kernel.  Once each, against tests/session_model.py (the scenarios tests/test_session_mock.py runs on the
CPU): an ROI cut then a quota cut, a subset of slots, reset, size mismatch, a duplicate, a damaged packet inside an increment,
reconstruction k = 3, display output, reduce = 1.  The plain decode of the same streams on the same decoder object equals the
oracle before and after a session ran."""
import numpy as np
import pytest

from icer_compression_amd import decoder
from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import session_cases as sc
from tests import session_model as sm
from tests.decoder_batch_cases import oracle_decode
from tests.test_gpu_recut import torch                      # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


class Rig:
    def __init__(self, torch, orc):
        self.torch, self.orc, self.keep = torch, orc, []

    def open(self, name, n_slots=1, reduce=0, reconstruct=0, display=False):
        g, _ = sc.CASES[name]
        rw, rh = red.reduced_size(g.w, g.h, reduce)
        dec = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits, reduce=reduce, reconstruct=reconstruct)
        self.keep.append(dec)
        return decoder.Session(dec, n_slots, rw * rh), \
            sm.SessionModel(self.orc, g.channels, g.stages, g.filt, g.segments, rw * rh, g.bits, reduce, reconstruct, n_slots)

    def feed(self, ses, feeds, slots=None, display=False, sizes=None):
        torch = self.torch
        n, ch, stride = len(feeds), ses.channels, ses.frame_stride
        lens = [len(f) for f in feeds]
        offs = [sum(lens[:k]) + 3 for k in range(n)]                 # (odd offsets, junk around the feeds)
        data = torch.from_numpy(np.frombuffer(b"\x5b\x60\x00" + b"".join(feeds) + b"\x5b" * 5, np.uint8).copy()).cuda()
        keep = data.clone()
        narrow = display or ses.bits == 8
        out = torch.full((n + 1, ch, stride), sc.SENT if narrow else sc.SENT * 0x0101, dtype=torch.uint8 if narrow else torch.int16, device="cuda")
        rcs, ws, hs = ses.feed_torch(data, lens, out[:n], offsets=offs, slots=slots, sizes=sizes, display=display)
        torch.cuda.synchronize()
        assert torch.equal(data, keep), "the feeds were modified on the device"
        host = out.cpu().numpy().view(np.uint8 if narrow else np.uint16)
        assert (host[n] == host[n, 0, 0]).all() and host[n, 0, 0] == (sc.SENT if narrow else sc.SENT * 0x0101), "written past the n rows"
        return rcs, ws, hs, [host[k].reshape(-1) for k in range(n)]


def plain_decode_equals_the_oracle(torch, orc, dec, g, streams):
    n, stride = len(streams), g.w * g.h
    blob, offs, lens = dec._pack(streams)
    data = torch.from_numpy(blob).cuda()
    out = torch.zeros((n, g.channels, stride), dtype=torch.int16 if g.bits == 16 else torch.uint8, device="cuda")
    rc, rcs, ws, hs = dec.decode_device(n, data.data_ptr(), offs, lens, out.data_ptr(), stride)
    torch.cuda.synchronize()
    assert rc == 0
    host = out.cpu().numpy().view(np.uint16 if g.bits == 16 else np.uint8)
    for k, s in enumerate(streams):
        want = oracle_decode(orc, s, g.channels, g.stages, g.filt, g.segments, stride, g.bits)
        assert (rcs[k], ws[k], hs[k]) == want[:3], (k, rcs[k], ws[k], hs[k], want[:3])
        for c in range(g.channels):
            assert np.array_equal(host[k, c, : g.w * g.h], want[3][c][: g.w * g.h]), (k, c)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_recut_ladder_fed_as_increments(torch, expected, oracle, name):
    g, spec = sc.CASES[name]
    rc, master = expected(g, spec, ebc.quota(g, "lossless"))[:2]
    assert rc == 0
    L = len(master)
    r = decoder.Recutter(g.w, g.h, g.channels, g.stages, g.segments, bits=g.bits)
    cuts = [row[0][1] for row in r.recut([master], [L // 6, L // 3, (2 * L) // 3])]
    assert cuts == sc.ladder(expected, name)[2], "the re-cuts are not the oracle's cuts"
    incs = [cuts[0]] + [r.combine([cuts[i]], [cuts[i + 1]], decoder.COMBINE_DIFFERENCE)[0][1] for i in range(2)]
    assert [len(x) for x in incs[1:]] == [len(cuts[i + 1]) - len(cuts[i]) for i in range(2)]
    rig = Rig(torch, oracle)
    ses, _ = rig.open(name)
    dec = rig.keep[-1]
    plain_decode_equals_the_oracle(torch, oracle, dec, g, cuts)
    for i, inc in enumerate(incs):
        got = rig.feed(ses, [inc])
        want = oracle_decode(oracle, cuts[i], g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
        assert want[0] == 0
        sc.check_step(g, got, 0, want, (name, "step", i))
    resumed, threads, planes, dropped = ses.stats()
    assert resumed >= 1 and dropped == 0 and planes == len(list(red.walk(cuts[2]))), (name, ses.stats())
    plain_decode_equals_the_oracle(torch, oracle, dec, g, cuts)
    ses.close()
    r.close()


def test_ladder_against_the_model_with_an_empty_feed(torch, expected, oracle):
    ses, _ = sc.run_ladder(Rig(torch, oracle), expected, oracle, "gray16_A4")
    assert ses.stats()[0] >= 1


def test_roi_cut_then_quota_cut(torch, expected, oracle):
    sc.run_roi_then_quota(Rig(torch, oracle), expected)


def test_slots_reset_size_mismatch_duplicate(torch, expected, oracle):
    sc.run_slots(Rig(torch, oracle), expected)


def test_damaged_packet_in_an_increment(torch, expected, oracle):
    sc.run_damaged_increment(Rig(torch, oracle), expected)


def test_a_plane_that_fails_stops_its_chain_for_good(torch, expected, oracle):
    sc.run_failing_plane(Rig(torch, oracle), expected, oracle)


@pytest.mark.parametrize("options", [dict(reconstruct=3), dict(display=True), dict(reduce=1)], ids=["recon3", "display", "reduce1"])
def test_decoder_options(torch, expected, oracle, options):
    ses, _ = sc.run_ladder(Rig(torch, oracle), expected, oracle, "gray16_A4", **options)
    assert ses.stats()[0] >= 1


def test_threads_only_routing(torch, expected, oracle, monkeypatch):
    """ICER_DEC_WAVE=0: every chain resumes in the thread-per-chain kernel"""
    monkeypatch.setenv("ICER_DEC_WAVE", "0")
    ses, _ = sc.run_ladder(Rig(torch, oracle), expected, oracle, "yuv8")
    assert ses.stats()[0] == 0 and ses.stats()[1] > 0
