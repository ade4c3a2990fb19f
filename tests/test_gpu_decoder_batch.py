"""The batch decoder (icerx_decode_host / icerx_decode_device, decode_batch in icer_compression_amd/csrc/decoder.hip) on the
GPU with many frames per call, frame by frame against the decoder oracle (and the reference decoder where it is built and
defined; tests/decoder_batch_cases.py builds the batches and their expected results):
  1. every filter, gray and YUV, 16 and 8 bits, sizes that share a width, each size at non-adjacent positions
     (the inverse transform's size groups), lossless and quota-cut streams, into host buffers and device buffers
  2. streams that stop early in the same batches: empty, truncated, a flipped payload byte, re-ordered, dropped and
     duplicated packets, a frame larger than the stride (rc -5), a frame too small for the segment grid (rc -3)
  3. every kernel choice, ICER_DEC_WAVE unset (chosen by load) and 0 / 1 / 2, and a batch past the load threshold
  4. the raised-LDS planes kernel (a chain 2048 wide) next to chains a few samples wide in one call
  5. more packets than the header kernel's first capacity (its second pass)
  6. one decoder object across calls of different sizes
  7. a hand-built blob: junk between streams, offsets out of order, shared bytes, zero-length entries, ws / hs in-values
The same cases, scaled down, run on the CPU mock-runtime build in tests/test_emu_decoder.py.
"""
import os

import numpy as np
import pytest

from oracle.binding import Oracle
from tests import decoder_batch_cases as dbc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.fixture(scope="module")
def dec():
    from icer_compression_amd import decoder
    decoder.load_library()
    return decoder


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _set_wave(value):
    if value is None:
        os.environ.pop("ICER_DEC_WAVE", None)
    else:
        os.environ["ICER_DEC_WAVE"] = value


@pytest.fixture(params=[None, "0", "1", "2"], ids=["by-load", "thread-per-chain", "wave-per-chain", "wave-per-plane"])
def kernel(request):
    """ICER_DEC_WAVE (read per call): unset = the kernel chosen by load, as library users get it; or pinned"""
    old = os.environ.get("ICER_DEC_WAVE")
    _set_wave(request.param)
    yield request.param
    _set_wave(old)


@pytest.fixture(params=[None, "1", "2"], ids=["by-load", "wave-per-chain", "wave-per-plane"])
def kernel_wide(request):
    old = os.environ.get("ICER_DEC_WAVE")
    _set_wave(request.param)
    yield request.param
    _set_wave(old)


def device_io(torch):
    def to_dev(a):
        t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
        torch.cuda.synchronize()
        return t.data_ptr(), t
    return to_dev, lambda t: t.cpu().numpy()


def run(dec, torch, b, label):
    d = dec.Decoder(b.channels, b.stages, b.filt, b.segments, bits=b.bits)
    try:
        dbc.decode_host(d, b, label)
        dbc.decode_device(d, b, *device_io(torch), label)
    finally:
        d.close()


_BATCHES = {}


def cached(key, make):
    if key not in _BATCHES:
        _BATCHES[key] = make()
    return _BATCHES[key]


@pytest.mark.timeout(240)
@pytest.mark.parametrize("filt", range(7))
def test_batch_filters_channels_bits(dec, orc, torch, kernel, filt):
    """cases 1-3: per filter, gray / YUV x 16 / 8 bits, one batch of 20 streams each, through both entry points"""
    for ch in (1, 3):
        for bits in (16, 8):
            b = cached(("mixed", filt, ch, bits), lambda: dbc.mixed_batch(orc, ch, bits, filt))
            run(dec, torch, b, f"filt {filt} ch {ch} bits {bits} mode {kernel}")


@pytest.mark.timeout(420)
def test_batch_past_the_load_threshold(dec, orc, torch, kernel):
    """case 3: enough chains that the unset choice (n_eligible > 12 * compute units: lane-per-plane kernel) changes its
    mind.  The test cannot see which chains were eligible (ChainDesc::fast), so the chain count from the packet headers
    is a bound, not a proof."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count

    def make():
        specs = [((1024, 1024, "noise", 1), dbc.LOSSLESS), ((1024, 1024, "smooth", 2), dbc.LOSSLESS),
                 ((1024, 1024, "noise", 3), dbc.CUT)]
        probe = dbc.Batch(orc, 1, 16, 1, 4, 32, [(s, q, None) for s, q in specs], check_reference=False)
        per = min(dbc.chains_in(s, 1) for s in probe.streams)
        reps = (2 * 12 * n_cus + per - 1) // per // len(specs) + 1
        return dbc.Batch(orc, 1, 16, 1, 4, 32, [(s, q, None) for _ in range(reps) for s, q in specs])
    b = cached(("load", n_cus), make)
    chains = sum(dbc.chains_in(s, 1) for s in b.streams)
    assert chains >= 2 * 12 * n_cus, (chains, n_cus)
    run(dec, torch, b, f"load mode {kernel}")


@pytest.mark.timeout(300)
def test_wide_and_narrow_chains_in_one_call(dec, orc, torch, kernel_wide):
    """case 4: one stage, one segment: a 4096 x 256 frame has chains 2048 wide, whose planes-kernel LDS is above the 48 KiB
    a launch gets without asking; frames a few samples wide have chains a few samples wide (several ring-size classes of
    the lane-per-plane kernel)"""
    wide, narrow = (4096, 256), [(6, 180), (9, 150), (7, 96), (12, 200), (5, 64), (40, 130)]
    widest = dbc.widest_segment(orc, *wide, 1, 1)
    assert widest >= 2048 and dbc.pw_lds_bytes(widest, 16) > 48 * 1024, widest
    assert max(dbc.widest_segment(orc, w, h, 1, 1) for w, h in narrow[:5]) <= 6

    def make():
        entries = [((4096, 256, "noise", 9), dbc.LOSSLESS, None)]
        for i, (w, h) in enumerate(narrow):
            entries.append(((w, h, "noise", 20 + i), dbc.LOSSLESS if i % 2 == 0 else dbc.CUT, None))
        entries.insert(4, ((4096, 256, "smooth", 10), dbc.CUT, None))
        return dbc.Batch(orc, 1, 16, 0, 1, 1, entries)
    b = cached("wide", make)
    assert set(b.rcs()) == {0}
    run(dec, torch, b, f"wide mode {kernel_wide}")


@pytest.mark.timeout(120)
def test_second_header_pass(dec, orc, torch, kernel):
    """case 5: more packets than count_headers_kernel's first capacity (asserted by the builder)"""
    run(dec, torch, cached("headers", lambda: dbc.header_pass_batch(orc, frames=6)), f"headers mode {kernel}")


@pytest.mark.timeout(180)
@pytest.mark.parametrize("bits", [16, 8])
def test_decoder_reused_across_calls(dec, orc, torch, bits):
    """case 6: one decoder object (filter D): a large call, a smaller call of other sizes and content, the large one
    again -- stale tmp / work / cands / pos contents would show"""
    large, small = cached(("reuse", bits), lambda: dbc.reuse_batches(orc, bits))
    d = dec.Decoder(1, large.stages, large.filt, large.segments, bits=bits)
    try:
        for k, b in enumerate((large, small, large, small, large)):
            dbc.decode_device(d, b, *device_io(torch), f"call {k}")
            dbc.decode_host(d, b, f"call {k}")
    finally:
        d.close()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("ch,bits", [(1, 16), (3, 8), (3, 16)])
def test_blob_layout(dec, orc, torch, ch, bits):
    """case 7: icerx_decode_device / icerx_decode_host on a hand-built blob, with ws / hs in-values"""
    layout = cached(("layout", ch, bits), lambda: dbc.Layout(orc, dbc.mixed_batch(orc, ch, bits, 4, seed=5)))
    d = dec.Decoder(ch, layout.batch.stages, layout.batch.filt, layout.batch.segments, bits=bits)
    try:
        for device in (True, False):
            dbc.layout_call(d, layout, device, *device_io(torch), f"device={device}")
    finally:
        d.close()
