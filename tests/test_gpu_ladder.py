"""The rate ladder (icerx_encode_device_ladder, include/icer_hip.h): one call codes a batch once and cuts it at several byte
quotas.  Every (frame, quota) must equal the oracle and a separate icerx_encode_device (or _s8) call at that quota -- on mixed
batches of every kind, on the full-size launches (a lone frame cut into sub-ranges, a batch in two parts, a YUV frame in
progressive mode), across a slot-bound retry and on long-lived encoders whose calls alternate with single and asynchronous
ones.  The caller's buffers keep their promises: the input is not modified, nothing is written beyond the Q * n rows and
entries, nor behind a stream in its row; and a refused call writes nothing at all."""
import ctypes as C

import numpy as np
import pytest

from icer_compression_amd import api, synth
from tests import encoder_batch_cases as ebc
from tests import test_gpu_encoder_batch as tb

pytestmark = pytest.mark.gpu

SENT, SENT_SIZE, SENT_RC = tb.SENT, tb.SENT_SIZE, tb.SENT_RC


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


def device_frames(frames):
    import torch
    return torch.from_numpy(frames.view(np.int16) if frames.dtype == np.uint16 else frames).to(torch.device("cuda", 0))


def ladder(enc, t, quotas, stride=None):
    """icerx_encode_device_ladder on the cuda tensor `t` into Q * n + 1 rows / entries filled with a sentinel (stride odd by
    default: rows start at every byte alignment).  Returns res[q][f] = (rc, stream) after checking the buffer promises."""
    import torch
    n, Q = t.shape[0], len(quotas)
    stride = stride or max(quotas) + 5
    keep = t.clone()
    out = torch.full((Q * n + 1, stride), SENT, dtype=torch.uint8, device=t.device)
    sizes = torch.full((Q * n + 1,), SENT_SIZE, dtype=torch.int64, device=t.device)
    rcs = torch.full((Q * n + 1,), SENT_RC, dtype=torch.int32, device=t.device)
    enc.encode_ladder_ptrs(t.data_ptr(), n, quotas, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(),
                           torch.cuda.current_stream(t.device).cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(t, keep), "the input frames were modified on the device"
    out, sizes, rcs = out.cpu().numpy(), sizes.cpu().numpy(), rcs.cpu().numpy()
    assert (out[Q * n] == SENT).all(), "bytes written past the Q * n rows of the output"
    assert int(sizes[Q * n]) == SENT_SIZE and int(rcs[Q * n]) == SENT_RC, "sizes / rcs written past Q * n entries"
    res = []
    for q, quota in enumerate(quotas):
        row = []
        for f in range(n):
            k = q * n + f
            s = int(sizes[k])
            assert 0 <= s <= quota, (q, f, s, quota)
            assert (out[k, s:] == SENT).all(), f"quota {q} frame {f}: bytes written behind its stream of {s} bytes"
            row.append((int(rcs[k]), out[k, :s].tobytes()))
        res.append(row)
    return res


def separate(enc, t, quota):
    """one icerx_encode_device (or _s8) call at `quota`: [(rc, stream)] per frame"""
    import torch
    n = t.shape[0]
    stride = quota + 5
    out = torch.full((n, stride), SENT, dtype=torch.uint8, device=t.device)
    sizes = torch.zeros(n, dtype=torch.int64, device=t.device)
    rcs = torch.zeros(n, dtype=torch.int32, device=t.device)
    args = (enc.handle, t.data_ptr(), n, quota, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(),
            torch.cuda.current_stream(t.device).cuda_stream)
    rc = enc.lib.icerx_encode_device_s8(*args) if enc.sample_bits == 8 else enc.lib.icerx_encode_device(*args)
    assert rc == 0, enc.lib.icerx_last_error()
    torch.cuda.synchronize()
    sz, rr, host = sizes.cpu().numpy(), rcs.cpu().numpy(), out.cpu().numpy()
    return [(int(rr[f]), host[f, : int(sz[f])].tobytes()) for f in range(n)]


def check_against_separate(enc, t, quotas, got, what):
    for q, quota in enumerate(quotas):
        want = separate(enc, t, quota)
        for f, (w, g) in enumerate(zip(want, got[q])):
            assert g == w, f"{what}: quota {quota} frame {f}: rc {g[0]} / {len(g[1])} bytes, separate call rc {w[0]} / {len(w[1])} " \
                           f"bytes, first difference at {ebc.first_difference(g[1], w[1])}"


def class_ladder(g, rng):
    """one quota of every class, shuffled, and one of them twice"""
    qs = [ebc.quota(g, c) for c in ebc.QUOTA_CLASSES]
    qs.append(qs[int(rng.integers(0, len(qs)))])
    rng.shuffle(qs)
    return [int(q) for q in qs]


# ---- mixed-content batches against the oracle and separate calls -----------------------------------------------------------
MIXED = {
    "gray": (tb.GRAY, tb.GRAY_BATCHES[::5]),
    "yuv": (tb.YUV, tb.YUV_BATCHES[::4]),
    "s8": (ebc.Geometry(256, 192, 1, 3, 0, 6, bits=8),
           [[(k, i) for i, k in enumerate(ebc.KINDS8)], [("noise6", 0), ("full8", 1), ("smooth6", 2), ("blank8", 3), ("noise6", 4)]]),
    "yuv8": (ebc.Geometry(128, 96, 3, 3, 0, 5, bits=8), [[(k, i) for i, k in enumerate(ebc.KINDS8)] + [("smooth6", 9)]]),
}


@pytest.mark.timeout(400)
@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_content_ladder(expected, name):
    g, batches = MIXED[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=9, sample_bits=g.bits)
    for b, specs in enumerate(batches):
        quotas = class_ladder(g, rng)
        t = device_frames(ebc.batch(g, specs))
        got = ladder(enc, t, quotas)
        for q, quota in enumerate(quotas):
            for f, spec in enumerate(specs):
                ebc.check_frame(*got[q][f], expected(g, spec, quota), f"{name} batch {b}: quota {quota} frame {f} {spec}")
        check_against_separate(enc, t, quotas, got, f"{name} batch {b}")
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


# ---- full-size launches against separate calls -------------------------------------------------------------------------------
@pytest.mark.timeout(400)
def test_lone_4096_frame_ladder_is_split():
    import torch
    w = h = 4096
    enc = api.Encoder(w, h, 1, 5, 0, 10, max_frames=1)
    t = synth.gray_frames_torch(1, w, h, synth.DEFAULT_SEED, torch.device("cuda", 0))
    quotas = [2 * w * h + 100_000, 5_000_000, 1_000_000, 70_000]
    got = ladder(enc, t, quotas)
    assert enc.launch_info()["split"], enc.launch_info()
    assert got[0][0][0] == 0, got[0][0][0]                                 # (the first quota holds the lossless stream)
    check_against_separate(enc, t, quotas, got, "4096^2 gray")
    enc.close()


@pytest.mark.timeout(400)
def test_batch_of_eight_2048_frames_ladder_in_two_parts():
    import torch
    w = h = 2048
    enc = api.Encoder(w, h, 1, 4, 0, 16, max_frames=8)
    t = synth.gray_frames_torch(8, w, h, 77, torch.device("cuda", 0))
    quotas = [1_000_000, 2 * w * h + 100_000, 70_000, 300_000]
    got = ladder(enc, t, quotas)
    assert enc.parts() == 2, enc.parts()
    check_against_separate(enc, t, quotas, got, "8 x 2048^2")
    enc.close()


@pytest.mark.timeout(400)
def test_yuv_4096_ladder_all_progressive():
    w = h = 4096
    enc = api.Encoder(w, h, 3, 5, 0, 10, max_frames=1)
    planes = np.stack(synth.color_frame_yuv(w, h, synth.DEFAULT_SEED))[None]
    t = device_frames(np.ascontiguousarray(planes))
    quotas = [100_000, 140_000, 70_000]
    got = ladder(enc, t, quotas)
    assert enc.launch_info()["pipeline_waves"] == 0, enc.launch_info()       # progressive: the window coder alone
    check_against_separate(enc, t, quotas, got, "4096^2 YUV")
    enc.close()


# ---- a ladder of one quota is the ordinary call ------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_single_quota_ladder_equals_encode_device(expected):
    g = tb.GRAY
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=9)
    for cls in ("lossless", "cut", "progressive", "tiny28"):
        q = ebc.quota(g, cls)
        for specs in (tb.GRAY_BATCHES[0], tb.GRAY_BATCHES[-1]):
            t = device_frames(ebc.batch(g, specs))
            got = ladder(enc, t, [q], stride=q + 5)
            assert got[0] == separate(enc, t, q), cls
            for f, spec in enumerate(specs):
                ebc.check_frame(*got[0][f], expected(g, spec, q), f"{cls} frame {f} {spec}")
    enc.close()


# ---- slot-bound retry ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_ladder_slot_retry(expected, monkeypatch):
    """slots of 1 bit per sample: the noise frame outgrows them, the batch is redone with larger slots and every quota's
    streams are cut again"""
    monkeypatch.setenv("ICER_HIP_SLOT_BPP", "1")
    g = ebc.Geometry(256, 256, 1, 1, 0, 1)
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=4)
    assert enc.info()["slot_bits_per_pixel"] == 1
    specs = [("blank", 0), ("flat", 0), ("noise8", 0), ("dot", 0)]
    quotas = [ebc.quota(g, c) for c in ("cut", "lossless", "tiny60", "progressive")]
    t = device_frames(ebc.batch(g, specs))
    got = ladder(enc, t, quotas)
    assert enc.stats()["slot_retries"] >= 1 and enc.info()["slot_bits_per_pixel"] > 1, (enc.stats(), enc.info())
    for q, quota in enumerate(quotas):
        for f, spec in enumerate(specs):
            ebc.check_frame(*got[q][f], expected(g, spec, quota), f"retry: quota {quota} frame {f} {spec}")
    check_against_separate(enc, t, quotas, got, "after the retry")
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


# ---- long-lived encoders: ladders between single and asynchronous calls ------------------------------------------------------
SEQUENCES = {
    "gray4": (ebc.Geometry(512, 384, 1, 2, 3, 2), 4, "128", ebc.KINDS16),
    "yuv3": (ebc.Geometry(256, 192, 3, 3, 1, 5), 3, None, ebc.KINDS16 + (("smooth", "overflow", "smooth"),)),
    "s8x4": (ebc.Geometry(512, 384, 1, 2, 0, 2, bits=8), 4, "128", ebc.KINDS8),
}
CALLS = 30


@pytest.mark.timeout(420)
@pytest.mark.parametrize("name", list(SEQUENCES))
def test_long_lived_encoder_with_ladders(expected, monkeypatch, name):
    g, mf, split, kinds = SEQUENCES[name]
    if split:
        monkeypatch.setenv("ICER_HIP_SPLIT", split)
    rng = np.random.default_rng(1000 + sum(map(ord, name)))
    enc = api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=mf, sample_bits=g.bits)
    entries = ("ladder", "s8") if g.bits == 8 else ("ladder", "sync", "async")
    classes = list(ebc.QUOTA_CLASSES)
    ladders = 0
    for call in range(CALLS):
        n = int(rng.integers(1, mf + 1))
        entry = entries[call % len(entries)] if call % 3 else "ladder"
        specs = [(kinds[int(rng.integers(0, len(kinds)))], int(rng.integers(0, 2))) for _ in range(n)]
        frames = ebc.batch(g, specs)
        if entry == "ladder":
            quotas = [ebc.quota(g, classes[int(i)]) for i in rng.integers(0, len(classes), int(rng.integers(1, 6)))]
            got = ladder(enc, device_frames(frames), quotas)
            for q, quota in enumerate(quotas):
                for f, spec in enumerate(specs):
                    ebc.check_frame(*got[q][f], expected(g, spec, quota), f"{name} call {call} ladder {quotas}: quota {quota} frame {f} {spec}")
            ladders += 1
        else:
            q = ebc.quota(g, classes[int(rng.integers(0, len(classes)))])
            tb.check(expected, g, specs, q, tb.encode(enc, g, entry, frames, q), f"{name} call {call} ({entry}, n={n})")
    assert ladders >= CALLS // 3
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()


# ---- refused calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_invalid_ladder_calls_write_nothing():
    import torch
    g = tb.GRAY
    enc = api.Encoder(g.w, g.h, 1, g.stages, g.filt, g.segments, max_frames=3)
    dev = torch.device("cuda", 0)
    t = device_frames(ebc.batch(g, [("smooth", 0), ("noise8", 0), ("sparse", 0)]))
    keep = t.clone()
    quotas = [ebc.quota(g, "cut"), ebc.quota(g, "lossless")]
    Q, n, stride = len(quotas), 3, max(quotas) + 5
    out = torch.full((Q * n, stride), SENT, dtype=torch.uint8, device=dev)
    sizes = torch.full((Q * n,), SENT_SIZE, dtype=torch.int64, device=dev)
    rcs = torch.full((Q * n,), SENT_RC, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    L = enc.lib

    def call(handle=enc.handle, frames=t.data_ptr(), nf=n, qs=quotas, nq=None, o=out.data_ptr(), s=stride, sz=sizes.data_ptr(),
             rc=rcs.data_ptr()):
        arr = None if qs is None else (C.c_size_t * max(len(qs), 1))(*qs)
        return L.icerx_encode_device_ladder(handle, frames, nf, arr, len(qs) if nq is None else nq, o, s, sz, rc, st)

    cases = {
        "no quotas": dict(nq=0), "17 quotas": dict(qs=[quotas[0]] * 17), "negative count": dict(nq=-1),
        "null encoder": dict(handle=None), "null frames": dict(frames=None), "null quotas": dict(qs=None, nq=2),
        "null out": dict(o=None), "null sizes": dict(sz=None), "null rcs": dict(rc=None),
        "no frames": dict(nf=0), "too many frames": dict(nf=4),
        "stride below the largest quota": dict(s=min(quotas) + 5),
    }
    for what, kw in cases.items():
        assert call(**kw) == api.ICER_INVALID_INPUT, what
    # an asynchronous encode pending on the encoder
    side = torch.full((n, stride), SENT, dtype=torch.uint8, device=dev)
    s_sizes, s_rcs = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    enc.encode_device_async_ptrs(t.data_ptr(), n, quotas[0], side.data_ptr(), stride, s_sizes.data_ptr(), s_rcs.data_ptr(), st)
    assert call() == api.ICER_INVALID_INPUT, "pending asynchronous encode"
    enc.wait()
    torch.cuda.synchronize()
    assert (out == SENT).all().item() and (sizes == SENT_SIZE).all().item() and (rcs == SENT_RC).all().item(), "a refused call wrote"
    assert torch.equal(t, keep)
    assert call() == 0                                        # (and the same arguments are accepted once nothing is pending)
    torch.cuda.synchronize()
    assert not (sizes == SENT_SIZE).any().item()
    enc.close()
