"""icerx_recut_device_async / decoder.Recutter on the GPU (icer_compression_amd/csrc/recut.hpp): stored streams re-cut to
smaller byte quotas.  Every (frame, quota) must equal the oracle's stream at that quota and a separate icerx_encode_device
(or _s8) call -- on mixed batches encoded on the device at the lossless quota, from a cut master, on a multi-segment frame of
several thousand units -- and chain into the asynchronous decode without the host.  Damaged masters are cut at the first
unit, in priority order, that lost its packet; bad frames leave their neighbours alone; the caller's buffers keep their
promises and a refused call writes nothing.  (The same source runs on the CPU in tests/test_emu_recut.py and
tests/test_recut_mock.py.)"""
import numpy as np
import pytest

from icer_compression_amd import api, decoder, synth
from tests import encoder_batch_cases as ebc
from tests import test_gpu_ladder as tl

pytestmark = pytest.mark.gpu

SENT, SENT_SIZE, SENT_RC = tl.SENT, tl.SENT_SIZE, tl.SENT_RC
HEADER = 28
QUOTA_EXCEEDED, OUT_OF_DATA, INVALID_INPUT, FATAL = -5, -7, -11, -10
ABORTED = ("overflow", "full8")                          # kinds whose encode returns ICER_INTEGER_OVERFLOW: an empty master

YUV = ebc.Geometry(256, 192, 3, 3, 1, 5)
GRAY = ebc.Geometry(512, 384, 1, 2, 3, 2)
GRAY8 = ebc.Geometry(256, 192, 1, 3, 0, 6, bits=8)
YUV8 = ebc.Geometry(128, 96, 3, 3, 0, 5, bits=8)
MIXED = {
    "yuv": (YUV, [("smooth", 0), ("noise8", 1), ("blank", 0), ("overflow", 7), ("sparse", 1), (("sparse", "dot", "wide"), 2)]),
    "gray": (GRAY, [("noise8", 0), ("flat", 1), ("blank", 2), ("wide", 3), ("overflow", 7), ("smooth", 4), ("dot", 5)]),
    "gray8": (GRAY8, [("blank8", 0), ("noise6", 1), ("smooth6", 2), ("full8", 3), ("noise6", 4)]),
    "yuv8": (YUV8, [("noise6", 0), ("blank8", 1), ("smooth6", 2), ("full8", 3), ("smooth6", 4)]),
}


@pytest.fixture(scope="module")
def expected(oracle):
    return ebc.Expected(oracle)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    decoder.load_library()
    return torch


def encoder(g, n):
    return api.Encoder(g.w, g.h, g.channels, g.stages, g.filt, g.segments, max_frames=n, sample_bits=g.bits)


def recutter(g):
    return decoder.Recutter(g.w, g.h, g.channels, g.stages, g.segments, bits=g.bits)


def encode_masters(torch, enc, t, quota):
    """icerx_encode_device (or _s8) at `quota`: the device buffers as the encoder leaves them -> (out (n, stride), sizes, rcs)"""
    n, stride = t.shape[0], quota + 5                    # (odd: masters start at every byte alignment)
    out = torch.full((n, stride), SENT, dtype=torch.uint8, device=t.device)
    sizes = torch.zeros(n, dtype=torch.int64, device=t.device)
    rcs = torch.zeros(n, dtype=torch.int32, device=t.device)
    args = (enc.handle, t.data_ptr(), n, quota, out.data_ptr(), stride, sizes.data_ptr(), rcs.data_ptr(),
            torch.cuda.current_stream(t.device).cuda_stream)
    rc = enc.lib.icerx_encode_device_s8(*args) if enc.sample_bits == 8 else enc.lib.icerx_encode_device(*args)
    assert rc == 0, enc.lib.icerx_last_error()
    return out, sizes, rcs


def recut(torch, r, data, lens, quotas, offsets=None, stream_stride=None):
    """recut_torch into Q * n + 1 rows / entries filled with a sentinel (stride odd: rows start at every byte alignment).
    Returns res[q][f] = (rc, stream) after checking the buffer promises."""
    n, Q = int(lens.shape[0]), len(quotas)
    stride = (max(quotas) + 5) | 1
    keep = data.clone()
    out = torch.full((Q * n + 1, stride), SENT, dtype=torch.uint8, device=data.device)
    sizes = torch.full((Q * n + 1,), SENT_SIZE, dtype=torch.int64, device=data.device)
    rcs = torch.full((Q * n + 1,), SENT_RC, dtype=torch.int32, device=data.device)
    r.recut_torch(data, lens, quotas, out[: Q * n], sizes[: Q * n], rcs[: Q * n], offsets=offsets, stream_stride=stream_stride)
    torch.cuda.synchronize()
    assert torch.equal(data, keep), "the masters were modified on the device"
    return read_rows(out, sizes, rcs, n, quotas)


def read_rows(out, sizes, rcs, n, quotas):
    Q = len(quotas)
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


def blob_of(torch, rng, streams):
    """the streams in one device blob at odd offsets with junk between them -> (data, offsets, lens)"""
    parts, offsets, at = [], [], 0
    for s in streams:
        gap = int(rng.integers(1, 40))
        gap += (at + gap + 1) % 2
        parts.append(rng.integers(0, 256, gap).astype(np.uint8).tobytes())
        at += gap
        offsets.append(at)
        parts.append(s)
        at += len(s)
    parts.append(b"\x5b" * 9)
    data = torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).cuda()
    return data, torch.tensor(offsets, dtype=torch.int64, device="cuda"), torch.tensor([len(s) for s in streams], dtype=torch.int64, device="cuda")


# ---- 1. mixed batches encoded on the device at the lossless quota ---------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_batches_recut_from_lossless_masters(torch, expected, name):
    g, specs = MIXED[name]
    aborted = [f for f, (kind, _) in enumerate(specs) if kind in ABORTED]
    assert len(aborted) <= 1 and 5 <= len(specs) <= 9
    rng = np.random.default_rng(sum(map(ord, name)))
    enc, r = encoder(g, len(specs)), recutter(g)
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, enc_rcs = encode_masters(torch, enc, t, ebc.quota(g, "lossless"))
    quotas = tl.class_ladder(g, rng)                      # every quota class, shuffled, one of them twice
    got = recut(torch, r, masters, sizes, quotas)          # (the encoder's d_out / out_stride / d_sizes as they are)
    assert [int(x) for x in enc_rcs.cpu()] == [-1 if f in aborted else 0 for f in range(len(specs))]
    for q, quota in enumerate(quotas):
        want = tl.separate(enc, t, quota)
        for f, spec in enumerate(specs):
            if f in aborted:                               # an aborted frame has an empty master
                assert got[q][f] == (OUT_OF_DATA, b""), (name, quota, spec)
                continue
            ebc.check_frame(*got[q][f], expected(g, spec, quota), f"{name}: quota {quota} frame {f} {spec}")
            assert got[q][f] == want[f], f"{name}: quota {quota} frame {f} {spec} differs from a separate encode"
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()
    r.close()


# ---- 2. a cut master ---------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_cut_master_recut(torch, expected):
    g = GRAY
    specs = [("noise8", 0), ("wide", 1), ("smooth", 2), ("blank", 3), ("sparse", 4)]
    mq = ebc.quota(g, "cut")
    enc, r = encoder(g, len(specs)), recutter(g)
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, enc_rcs = encode_masters(torch, enc, t, mq)
    master_rcs = [int(x) for x in enc_rcs.cpu()]
    assert QUOTA_EXCEEDED in master_rcs and set(master_rcs) <= {0, QUOTA_EXCEEDED}
    host, sz = masters.cpu().numpy(), sizes.cpu().numpy()
    quotas = [ebc.quota(g, c) for c in ("tiny60", "lossless", "cut", "progressive", "tiny27")] + [mq + 1, mq - 1]
    got = recut(torch, r, masters, sizes, quotas)
    for q, quota in enumerate(quotas):
        for f, spec in enumerate(specs):
            if quota > mq and master_rcs[f] == QUOTA_EXCEEDED:          # beyond a cut master's own quota: the master itself
                assert got[q][f] == (QUOTA_EXCEEDED, host[f, : int(sz[f])].tobytes()), (quota, spec)
            else:
                ebc.check_frame(*got[q][f], expected(g, spec, quota), f"cut master: quota {quota} frame {f} {spec}")
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()
    r.close()


# ---- 3. several thousand units, a header's length to more than a KiB -----------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_multi_segment_1024_frame(torch):
    g = ebc.Geometry(1024, 1024, 1, 4, 0, 32)
    enc, r = encoder(g, 1), recutter(g)
    t = synth.gray_frames_torch(1, g.w, g.h, 4321, torch.device("cuda", 0))
    masters, sizes, enc_rcs = encode_masters(torch, enc, t, ebc.quota(g, "lossless"))
    assert int(enc_rcs[0]) == 0
    quotas = [150_000, ebc.quota(g, "lossless"), 40_000, 600_000]
    got = recut(torch, r, masters, sizes, quotas)
    tl.check_against_separate(enc, t, quotas, got, "1024^2 gray, 32 segments")
    # (several thousand units, so the walk loops many times over its 64 lanes; from little more than a header to more than a
    # KiB -- a unit of this geometry has at most 8192 samples, so none reaches tens of KiB)
    stream = got[1][0][1]
    lens, at = [], 0
    while at < len(stream):
        lens.append(HEADER + (int.from_bytes(stream[at + 16: at + 20], "little") + 7) // 8)
        at += lens[-1]
    assert at == len(stream) and len(lens) > 640 and min(lens) <= HEADER + 8 and max(lens) >= 1024, (len(lens), min(lens), max(lens))
    assert enc.stats()["unit_timeouts"] == 0
    enc.close()
    r.close()


# ---- 4. encoder -> re-cut -> decoder on one stream ---------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["yuv", "gray8"])
def test_chain_encode_recut_decode_without_the_host(torch, name):
    g, specs = MIXED[name]
    specs = [s for s in specs if s[0] not in ABORTED]
    n = len(specs)
    quotas = [ebc.quota(g, "progressive"), ebc.quota(g, "cut")]
    Q = len(quotas)
    enc, r = encoder(g, n), recutter(g)
    d = decoder.Decoder(g.channels, g.stages, g.filt, g.segments, bits=g.bits)
    dt = torch.int16 if g.bits == 16 else torch.uint8
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            t = tl.device_frames(ebc.batch(g, specs))
            masters, sizes, _ = encode_masters(torch, enc, t, ebc.quota(g, "lossless"))
            out = torch.zeros((Q, n, max(quotas) + 3), dtype=torch.uint8, device="cuda")
            cut_sizes = torch.zeros((Q, n), dtype=torch.int64, device="cuda")
            cut_rcs = torch.zeros((Q, n), dtype=torch.int32, device="cuda")
            r.recut_torch(masters, sizes, quotas, out, cut_sizes, cut_rcs)
            planes = torch.full((Q, n, g.channels, g.w * g.h), 0x5A, dtype=dt, device="cuda")
            rcs = torch.full((Q, n), 77, dtype=torch.int32, device="cuda")
            ws, hs = torch.zeros((Q, n), dtype=torch.int64, device="cuda"), torch.zeros((Q, n), dtype=torch.int64, device="cuda")
            for q in range(Q):                               # (a quota's block goes into the decoder as it is)
                d.decode_torch(out[q], cut_sizes[q], planes[q], rcs[q], ws[q], hs[q])
        st.synchronize()
        assert ws.cpu().tolist() == [[g.w] * n] * Q and hs.cpu().tolist() == [[g.h] * n] * Q
        for q, quota in enumerate(quotas):                   # against decoding the separately encoded streams
            want_streams = tl.separate(enc, t, quota)
            res = d.decode_host([s for _, s in want_streams], g.w * g.h)[1]
            for f in range(n):
                for c in range(g.channels):
                    got = planes[q, f, c].cpu().numpy()
                    got = got.view(np.uint16) if g.bits == 16 else got
                    assert int(rcs[q, f]) == res[f][0] and np.array_equal(got, res[f][3][c]), (name, quota, f, c)
    finally:
        d.close()
        enc.close()
        r.close()


# ---- 5. damaged masters and bad frames ----------------------------------------------------------------------------------------------
def packets_of(stream):
    """[(offset, length, (level, subband, lsb, segment), bits)] of a well-formed gray stream, in stream order"""
    res, at = [], 0
    while at < len(stream):
        assert stream[at: at + 2] == b"\x5b\x60"
        bits = int.from_bytes(stream[at + 16: at + 20], "little")
        n = HEADER + (bits + 7) // 8
        res.append((at, n, (stream[at + 4], stream[at + 5], stream[at + 7] & 15, stream[at + 6]), bits))
        at += n
    return res


def gray_priority_order(stages, segments, planes=9):
    """(level, subband, lsb, segment) of a gray frame's units in priority order (csrc/plan.hpp make_packets: stable sort by
    priority down, then subband up; segments in turn)"""
    LL, HL, LH, HH = 0, 1, 2, 3
    pk = []
    for st in range(1, stages + 1):
        for lsb in range(planes):
            pk += [(st, HL, lsb, (1 << st) << lsb), (st, LH, lsb, (1 << st) << lsb), (st, HH, lsb, (((1 << st) // 2) << lsb) + 1)]
    pk += [(stages, LL, lsb, (2 << stages) << lsb) for lsb in range(planes)]
    pk.sort(key=lambda p: (-p[3], p[1]))
    return [(lv, sb, lsb, sg) for lv, sb, lsb, _ in pk for sg in range(segments)]


def recut_in_python(stream, lost, order, quota):
    """the documented rule on a well-formed master whose packet of unit `lost` cannot be used: (rc, stream)"""
    pk = {key: (off, n, bits) for off, n, key, bits in packets_of(stream)}
    used, kept = 0, set()
    for key in order:
        if key == lost or key not in pk:
            break
        bits = pk[key][2]
        if used + HEADER > quota or (bits > 0 and (bits >> 3) + used + HEADER >= quota):
            break
        used += pk[key][1]
        kept.add(key)
    body = b"".join(stream[off: off + n] for off, n, key, _ in packets_of(stream) if key in kept)
    assert len(body) == used
    return (0 if len(kept) == len(order) else QUOTA_EXCEEDED), body


@pytest.mark.timeout(300)
def test_damaged_masters_and_bad_frames(torch, expected):
    g = ebc.Geometry(256, 192, 1, 3, 0, 6)
    other = ebc.Geometry(128, 192, 1, 3, 0, 6)
    mq = ebc.quota(g, "lossless")
    specs = [("smooth", 0), ("noise8", 1), ("sparse", 2), ("noise8", 3)]
    good = [expected(g, s, mq) for s in specs]
    assert all(rc == 0 for rc, _, _ in good)
    order = gray_priority_order(g.stages, g.segments)
    assert sorted(order) == sorted(key for _, _, key, _ in packets_of(good[1][1]))
    # frame 1: a payload byte of a mid-priority packet flipped; frame 2: a header byte
    lost = {}
    damaged = {}
    for f, in_header in ((1, False), (2, True)):
        s = bytearray(good[f][1])
        pk = {key: (off, n, bits) for off, n, key, bits in packets_of(good[f][1])}
        mid = next(key for key in order[len(order) // 3:] if pk[key][2] >= 64)
        off, n, _ = pk[mid]
        s[off + (9 if in_header else HEADER + (n - HEADER) // 2)] ^= 0x10
        lost[f], damaged[f] = mid, bytes(s)
    rng = np.random.default_rng(3)
    junk = rng.integers(0, 256, 5000).astype(np.uint8).tobytes()
    alien = expected(other, ("smooth", 0), ebc.quota(other, "lossless"))[1]
    streams = [good[0][1], damaged[1], damaged[2], junk, alien, good[3][1]]
    data, offsets, lens = blob_of(torch, rng, streams)
    # a seventh frame addressed outside the blob
    offsets = torch.cat([offsets, torch.tensor([data.numel() - 10], dtype=torch.int64, device="cuda")])
    lens = torch.cat([lens, torch.tensor([11], dtype=torch.int64, device="cuda")])
    quotas = [mq, ebc.quota(g, "cut"), ebc.quota(g, "progressive"), 60]
    r = recutter(g)
    got = recut(torch, r, data, lens, quotas, offsets=offsets)
    cut_by_damage = 0
    for q, quota in enumerate(quotas):
        for f in (0, 5):                                     # the neighbours are unaffected
            ebc.check_frame(*got[q][f], expected(g, specs[0 if f == 0 else 3], quota), f"neighbour {f} at quota {quota}")
        for f in (1, 2):
            want = recut_in_python(good[f][1], lost[f], order, quota)
            assert got[q][f] == want, (quota, f, got[q][f][0], len(got[q][f][1]), want[0], len(want[1]))
            cut_by_damage += want[1] != expected(g, specs[f], quota)[1]
        assert [got[q][f] for f in (3, 4, 6)] == [(OUT_OF_DATA, b""), (INVALID_INPUT, b""), (INVALID_INPUT, b"")], quota
    assert cut_by_damage >= 2                                # (the damage, not the quota, decided some of the cuts)
    r.close()


# ---- 6. refused calls, two calls in flight -----------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_refused_calls_write_nothing(torch, expected):
    g = GRAY8
    specs = [("smooth6", 0), ("noise6", 1), ("blank8", 2)]
    mq = ebc.quota(g, "lossless")
    data, offsets, lens = blob_of(torch, np.random.default_rng(1), [expected(g, s, mq)[1] for s in specs])
    keep = data.clone()
    quotas = [ebc.quota(g, "cut"), mq]
    n, Q, stride = len(specs), len(quotas), mq + 5
    out = torch.full((Q * n, stride), SENT, dtype=torch.uint8, device="cuda")
    sizes = torch.full((Q * n,), SENT_SIZE, dtype=torch.int64, device="cuda")
    rcs = torch.full((Q * n,), SENT_RC, dtype=torch.int32, device="cuda")
    r = recutter(g)
    need = r.workspace_bytes(n, data.numel(), Q)
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        a = dict(n=n, d_data=data.data_ptr(), data_bytes=data.numel(), d_offsets=offsets.data_ptr(), stream_stride=0,
                 d_lens=lens.data_ptr(), quotas=quotas, d_out=out.data_ptr(), out_stride=stride, d_sizes=sizes.data_ptr(),
                 d_rcs=rcs.data_ptr(), d_workspace=work.data_ptr(), workspace_bytes=need, stream=st)
        a.update(kw)
        return r.recut_device_async_ptrs(**a)

    cases = {
        "no quotas": dict(n_quotas=0), "17 quotas": dict(quotas=[60] * 17), "negative quota count": dict(n_quotas=-1),
        "no frames": dict(n=0), "negative frames": dict(n=-1), "too many frames": dict(n=65536),
        "null quotas": dict(quotas=None, n_quotas=2), "null data": dict(d_data=None), "null lens": dict(d_lens=None),
        "null out": dict(d_out=None), "null sizes": dict(d_sizes=None), "null rcs": dict(d_rcs=None), "null workspace": dict(d_workspace=None),
        "stride below the largest quota": dict(out_stride=mq - 1), "workspace too small": dict(workspace_bytes=need - 1),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID_INPUT, what
    assert call(data_bytes=0xFFFFFFFF - 64) == FATAL
    torch.cuda.synchronize()
    assert (out == SENT).all().item() and (sizes == SENT_SIZE).all().item() and (rcs == SENT_RC).all().item(), "a refused call wrote"
    assert torch.equal(data, keep)
    assert call() == 0                                       # (and the same arguments are accepted)
    torch.cuda.synchronize()
    assert not (sizes == SENT_SIZE).any().item()
    for q, quota in enumerate(quotas):
        for f, spec in enumerate(specs):
            k = q * n + f
            ebc.check_frame(int(rcs[k]), out[k, : int(sizes[k])].cpu().numpy().tobytes(), expected(g, spec, quota), f"quota {quota} frame {f}")
    r.close()


@pytest.mark.timeout(300)
def test_two_calls_in_flight_on_two_streams(torch, expected):
    """one recutter, two streams, a workspace each (recut_torch keeps one per stream)"""
    g = YUV
    specs = [("smooth", 0), ("noise8", 1), (("sparse", "dot", "wide"), 2)]
    mq = ebc.quota(g, "lossless")
    quotas = [ebc.quota(g, "cut"), 60, ebc.quota(g, "progressive"), mq]
    n, Q, stride = len(specs), len(quotas), (mq + 5) | 1
    r = recutter(g)
    runs = []
    for k, st in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        order = list(range(n)) if k == 0 else list(reversed(range(n)))
        with torch.cuda.stream(st):
            data, offsets, lens = blob_of(torch, np.random.default_rng(k), [expected(g, specs[f], mq)[1] for f in order])
            out = torch.full((Q * n + 1, stride), SENT, dtype=torch.uint8, device="cuda")
            sizes = torch.full((Q * n + 1,), SENT_SIZE, dtype=torch.int64, device="cuda")
            rcs = torch.full((Q * n + 1,), SENT_RC, dtype=torch.int32, device="cuda")
            torch.cuda._sleep(int(10e-3 * 2.1e9))
            r.recut_torch(data, lens, quotas, out[: Q * n], sizes[: Q * n], rcs[: Q * n], offsets=offsets)
        runs.append((order, out, sizes, rcs, data))
    assert len(r._workspaces) >= 2
    torch.cuda.synchronize()
    for order, out, sizes, rcs, _ in runs:
        got = read_rows(out, sizes, rcs, n, quotas)
        for q, quota in enumerate(quotas):
            for k, f in enumerate(order):
                ebc.check_frame(*got[q][k], expected(g, specs[f], quota), f"two streams: quota {quota} frame {f}")
    r.close()
