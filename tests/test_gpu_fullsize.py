"""The launch shapes that exist only at full size (csrc/launch_plan.hpp), through every filter, against the reference build's digests
(tests/golden/golden.json from make_golden.py, fullsize_batch_golden.json from make_fullsize_batch_golden.py).  No ICER_HIP_* variable
is set: every launch is the production one, and every test asserts that it had the shape its row is there for.

  row (what plan_launch picks)                                                       goldens
  lone gray frame cut into sub-ranges (PipeKernel::Lone, list kernel Four, splice)   split_*: filters D E F Q, 12-bit D E, 4001 x 3003
  lone gray frame left whole (PipeKernel::Large, no list kernel)                     whole_2048_filtD, whole_2048_12bit_filtQ
  lone YUV frame, lossless (list kernel One beside PipeKernel::Large)                yuv_2048_lossless_filt{A,E,Q}, yuv_4096_lossless_filtD
  batch, lossless (PipeKernel::Batch, position-major, two parts)                     gray8_2048_filt{B,D,F,Q}, yuv3_2048_filt{C,E} (one part)
  progressive (window coder Four alone)                                              prog_4096_yuv_quota70000_filtB, prog_4096_gray_quota1000000_filtF
  few / many segments at 4096^2 (very long / very many units)                        seg4_4096_filt{A,F}, seg32_4096_filtQ
  the GPU decoder at these sizes                                                     every stream above, both decode kernels, both batch calls

A lone frame goes through icerx_encode_host and through icerx_encode_device (they differ in part planning); a batch through
icerx_encode_device, the pipelined host batch from page-locked memory, and a rate ladder whose largest quota is the lossless one.
Everything is byte or digest equality; the inputs are synthesised once per module (a 4096^2 frame costs more host time than its
encode costs GPU time)."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from icer_compression_amd import api, synth
from tests import test_gpu_decoder_async as tda
from tests import test_gpu_encoder_batch as tb
from tests import test_gpu_ladder as tl

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# golden name -> the shape its launch must have
SPLIT, WHOLE, YUV, PROGRESSIVE = "split", "whole", "yuv", "progressive"
LONE = {
    "split_4096_filtD": SPLIT, "split_4096_filtE": SPLIT, "split_4096_filtF": SPLIT, "split_4096_filtQ": SPLIT,
    "split_4096_12bit_filtD": SPLIT, "split_4096_12bit_filtE": SPLIT, "split_4001x3003_filtE": SPLIT,
    # 4 segments: level-1 units of 16 384 chunks.  plan.hpp auto_split_chunks counts, per piece size p, min(chunks / p, 8) pieces for every
    # unit of at least 2 p chunks in bit planes 0 .. 4, until they fit 2 x 256 compute units: 1 024: 480 + 240, 1 536 / 2 048: 480 + 120,
    # 3 072: 300 -- pieces of 3 072 chunks, a split launch
    "seg4_4096_filtA": SPLIT, "seg4_4096_filtF": SPLIT,
    # 32 segments: level-1 units of 409 x 320 .. 342 x 384 samples = 2 045 .. 2 052 chunks.  Only those of 2 048 chunks and more make two
    # pieces of 1 024, few enough for the budget: pieces of 1 024 chunks, and again a split launch -- of units that are barely long
    # enough beside equally long ones that stay whole (plan.hpp built on the host: 432 sub-range workgroups, as with 4 segments)
    "seg32_4096_filtQ": SPLIT,
    # 2048 x 2048 with 16 segments: no unit reaches 2 x 1 024 chunks, the frame is coded whole
    "whole_2048_filtD": WHOLE, "whole_2048_12bit_filtQ": WHOLE,
    "yuv_2048_lossless_filtA": YUV, "yuv_2048_lossless_filtE": YUV, "yuv_2048_lossless_filtQ": YUV, "yuv_4096_lossless_filtD": YUV,
    "prog_4096_yuv_quota70000_filtB": PROGRESSIVE, "prog_4096_gray_quota1000000_filtF": PROGRESSIVE,
}
BATCHES = ["gray8_2048_filtB", "gray8_2048_filtD", "gray8_2048_filtF", "gray8_2048_filtQ", "yuv3_2048_filtC", "yuv3_2048_filtE"]
# the variables tests/test_gpu_stress.py pops, and every other knob of the encoder and the decoder
KNOBS = ["ICER_HIP_CODER", "ICER_HIP_PIPE_WAVES", "ICER_HIP_HYBRID", "ICER_HIP_HYBRID_FRAMES", "ICER_HIP_SPLIT", "ICER_HIP_LIST_WAVES",
         "ICER_STRESS_BATCH", "ICER_DEC_WAVE"]


@pytest.fixture(autouse=True)
def production_settings(monkeypatch):
    for name in KNOBS + [k for k in os.environ if k.startswith("ICER_HIP_")]:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def batch_golden():
    with open(os.path.join(ROOT, "tests", "golden", "fullsize_batch_golden.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def dec():
    from icer_compression_amd import decoder
    decoder.load_library()
    return decoder


_INPUTS, _STREAMS = {}, {}       # synthesised once per module; the GPU encoder's streams, once they equalled the goldens


def cached(key, make):
    if key not in _INPUTS:
        _INPUTS[key] = make()
    return _INPUTS[key]


def lone_planes(g):
    """(channels, h, w) uint16, by the rule of tests/golden/make_golden.py planes_of"""
    kind, w, h, seed, mode = g["kind"], g["w"], g["h"], g["seed"], g["mode"]
    if kind == "yuv":
        return cached((kind, w, h, seed), lambda: np.stack(synth.color_frame_yuv(w, h, seed)))
    make = synth.gray_frame_12bit if kind == "gray12" else synth.gray_frame
    return cached((kind, w, h, seed, mode), lambda: make(w, h, seed, mode)[None])


def batch_frames(c):
    """(n, h, w) or (n, 3, h, w) uint16, by the rule of tests/golden/make_fullsize_batch_golden.py frame_planes"""
    def frame(k):
        g = dict(kind={"noise": "gray"}.get(c["content"][k], c["content"][k]), w=c["w"], h=c["h"], seed=c["base_seed"] + k,
                 mode=0 if c["content"][k] == "noise" else 1)
        p = lone_planes(g)
        return p if c["channels"] == 3 else p[0]
    return cached(("batch", c["channels"], tuple(c["content"])), lambda: np.ascontiguousarray(np.stack([frame(k) for k in range(len(c["content"]))])))


def digest(rc, stream):
    return (rc, len(stream), "%08x" % zlib.crc32(stream), hashlib.sha256(stream).hexdigest()[:16])


def planes_digest(planes):
    hsh = hashlib.sha256()
    for p in planes:
        hsh.update(np.ascontiguousarray(p).tobytes())
    return hsh.hexdigest()[:16]


def check_shape(enc, shape, what):
    li, st = enc.launch_info(), enc.stats()
    if shape == SPLIT:
        assert li["split"] and li["sub_range_workgroups"] > 0 and li["pipeline_waves"] == 8 and li["window_coder_beside"], (what, li)
    elif shape == WHOLE:
        assert not li["split"] and li["sub_range_workgroups"] == 0 and li["pipeline_waves"] == 11 and not li["window_coder_beside"], (what, li)
    elif shape == YUV:
        assert li["window_coder_beside"] and not li["split"] and li["sub_range_workgroups"] == 0 and li["pipeline_waves"] == 11, (what, li)
    else:
        assert li["pipeline_waves"] == 0 and not li["split"], (what, li)
    assert enc.parts() == 1, (what, enc.parts())
    assert st["unit_timeouts"] == 0 and st["fallback_batches"] == 0, (what, st)


def encode_lone(g, entry, shape, what):
    """the frame of golden `g` through icerx_encode_host ("host") or icerx_encode_device ("device": into sentinel-filled buffers, the input
    tensor compared afterwards -- tests/test_gpu_encoder_batch.py encode); -> (rc, stream) after the launch-shape checks"""
    planes = lone_planes(g)
    enc = api.Encoder(g["w"], g["h"], planes.shape[0], g["stages"], g["filt"], g["segments"], max_frames=1)
    try:
        if entry == "host":
            (rc, stream), = enc.encode_host(planes[None], g["quota"])
        else:
            (rc, stream), = tb.encode(enc, None, "sync", planes[None], g["quota"])
        check_shape(enc, shape, what)
    finally:
        enc.close()
    return rc, stream


# ---- lone frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", list(LONE))
def test_lone_frame(golden, name, entry):
    g = golden[name]
    assert (g["quota"] < g["w"] * g["h"] * (3 if g["kind"] == "yuv" else 1) // 2) == (LONE[name] == PROGRESSIVE)
    rc, stream = encode_lone(g, entry, LONE[name], f"{name} {entry}")
    print(name, entry, digest(rc, stream))
    assert digest(rc, stream) == (g["rc"], g["size"], g["crc32"], g["sha256_16"]), name
    _STREAMS[name] = stream


def gpu_stream(golden, name):
    """the GPU encoder's stream of a lone-frame golden, proven equal to the reference's"""
    if name not in _STREAMS:
        g = golden[name]
        rc, stream = encode_lone(g, "host", LONE[name], name)
        assert digest(rc, stream) == (g["rc"], g["size"], g["crc32"], g["sha256_16"]), name
        _STREAMS[name] = stream
    return _STREAMS[name]


def check_lone_decode(dec, golden, name):
    g = golden[name]
    planes = lone_planes(g)
    drc, w, h, back = dec.decompress(gpu_stream(golden, name), planes.shape[0], g["stages"], g["filt"], g["segments"])
    print(name, (drc, w, h, planes_digest(back)))
    assert (drc, w, h, planes_digest(back)) == (g["decoded_rc"], g["decoded_w"], g["decoded_h"], g["decoded_sha256_16"]), name
    same = all(np.array_equal(b.reshape(h, w), p) for b, p in zip(back, planes))
    assert same == g["decoded_is_input"], name


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(LONE))
def test_lone_frame_decodes(dec, golden, name):
    """libicer_hip_dec.so (its own choice of kernel) on the GPU encoder's stream: the reference decoder's digest, and the input where the
    reference gives the input back (lossless, but 12-bit content: 9 bit planes are coded)"""
    check_lone_decode(dec, golden, name)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["split_4096_filtE", "yuv_2048_lossless_filtQ"])
def test_lone_frame_decodes_wave_per_chain(dec, golden, monkeypatch, name):
    monkeypatch.setenv("ICER_DEC_WAVE", "1")
    check_lone_decode(dec, golden, name)


# ---- batches ------------------------------------------------------------------------------------------------------------------------
def check_batch_frames(got, b, what):
    for k, (rc, stream) in enumerate(got):
        print(what, k, digest(rc, stream)[:3])
        assert list(digest(rc, stream)[:3]) == b["frames"][k], f"{what}: frame {k}"


def batch_encoder(c, n):
    return api.Encoder(c["w"], c["h"], c["channels"], c["stages"], c["filter"], c["segments"], max_frames=n)


def check_batch_launch(enc, n, what):
    assert enc.parts() == (2 if n == 8 else 1), (what, enc.parts())
    li, st = enc.launch_info(), enc.stats()
    assert li["window_coder_beside"] and not li["split"] and li["pipeline_waves"] == 8, (what, li)
    assert st["unit_timeouts"] == 0 and st["fallback_batches"] == 0, (what, st)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", BATCHES)
def test_batch_device(batch_golden, name):
    """icerx_encode_device: in two parts on two streams for the batches of eight; the input tensor is not modified, nothing is written
    beyond the frames' rows (tests/test_gpu_encoder_batch.py encode)"""
    b = batch_golden[name]
    c, frames = b["config"], batch_frames(b["config"])
    enc = batch_encoder(c, len(frames))
    try:
        got = tb.encode(enc, None, "sync", frames, c["quota"])
        check_batch_launch(enc, len(frames), name)
    finally:
        enc.close()
    check_batch_frames(got, b, name)
    _STREAMS[name] = [s for _, s in got]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", BATCHES)
def test_batch_from_pinned_host_memory(batch_golden, name):
    """api.compress_batch(..., devices=[0]): the pipelined host batch, frames and output page-locked"""
    b = batch_golden[name]
    c, frames = b["config"], batch_frames(b["config"])
    n, q = len(frames), c["quota"]
    keep = frames.copy()
    out = np.full((n + 1, q + 5), tb.SENT, np.uint8)
    sizes, rcs = np.full(n + 1, tb.SENT_SIZE, np.uint64), np.full(n + 1, tb.SENT_RC, np.int32)
    before = api.process_stats()
    assert api.pin_host(frames) and api.pin_host(out)
    try:
        rc = api.compress_batch(frames, c["stages"], c["filter"], c["segments"], q, out, sizes, rcs, devices=[0])
        assert rc == 0, api.load_library().icerx_last_error()
    finally:
        api.load_library().icerx_batch_release()
        api.unpin_host(frames)
        api.unpin_host(out)
    after = api.process_stats()
    assert np.array_equal(frames, keep), "the input frames were modified"
    assert (out[n] == tb.SENT).all() and int(sizes[n]) == tb.SENT_SIZE and int(rcs[n]) == tb.SENT_RC
    assert all((out[k, int(sizes[k]):] == tb.SENT).all() for k in range(n))
    check_batch_frames([(int(rcs[k]), out[k, : int(sizes[k])].tobytes()) for k in range(n)], b, name)
    assert after["unit_timeouts"] == before["unit_timeouts"] and after["fallback_batches"] == before["fallback_batches"], (before, after)


@pytest.mark.timeout(400)
@pytest.mark.parametrize("name", BATCHES)
def test_batch_ladder(batch_golden, name):
    """a ladder of three quotas, the largest the lossless one: its row against the golden, the other rows against separate calls"""
    b = batch_golden[name]
    c, frames = b["config"], batch_frames(b["config"])
    quotas = [1_000_000, c["quota"], 70_000 * c["channels"]]
    enc = batch_encoder(c, len(frames))
    try:
        t = tl.device_frames(frames)
        got = tl.ladder(enc, t, quotas)
        check_batch_launch(enc, len(frames), name)
        check_batch_frames(got[1], b, name + " ladder")
        tl.check_against_separate(enc, t, [quotas[0], quotas[2]], [got[0], got[2]], name)
        assert enc.stats()["unit_timeouts"] == 0 and enc.stats()["fallback_batches"] == 0, enc.stats()
    finally:
        enc.close()


@pytest.mark.timeout(400)
@pytest.mark.parametrize("name", BATCHES)
def test_batch_decodes(dec, batch_golden, name):
    """the batch's streams (the GPU encoder's, equal to the reference's) in one icerx_decode_host call and one stream-ordered
    decode_torch call: every frame against the reference decoder's digest, and against its input where the reference gives it back"""
    import torch
    b = batch_golden[name]
    c, frames = b["config"], batch_frames(b["config"])
    n, ch, stride = len(frames), c["channels"], c["w"] * c["h"]
    if name not in _STREAMS:
        enc = batch_encoder(c, n)
        try:
            got = tb.encode(enc, None, "sync", frames, c["quota"])
        finally:
            enc.close()
        check_batch_frames(got, b, name)
        _STREAMS[name] = [s for _, s in got]
    streams = _STREAMS[name]
    inputs = frames.reshape(n, ch, stride)

    def check(k, rc, w, h, planes, what):
        drc, sha, is_input = b["decoded"][k]
        assert (rc, w, h, planes_digest(planes)) == (drc, c["w"], c["h"], sha), f"{name} {what}: frame {k}"
        assert all(np.array_equal(planes[j], inputs[k, j]) for j in range(ch)) == is_input, f"{name} {what}: frame {k}"

    d = dec.Decoder(ch, c["stages"], c["filter"], c["segments"])
    try:
        rc, res = d.decode_host(streams, stride)
        assert rc == 0, name
        for k, (rk, wk, hk, pk) in enumerate(res):
            check(k, rk, wk, hk, pk, "decode_host")
        blob, offs, lens = d._pack(streams)
        rcs, ws, hs, out = tda.decode_async(torch, d, blob, list(offs), list(lens), stride)
        out = out.reshape(n, ch, stride)
        for k in range(n):
            check(k, rcs[k], ws[k], hs[k], list(out[k]), "decode_torch")
    finally:
        d.close()
