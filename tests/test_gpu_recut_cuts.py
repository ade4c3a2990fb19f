"""icerx_recut_device_cuts_async / decoder.Recutter.recut_cuts_torch on the GPU (icer_compression_amd/csrc/recut.hpp):
stored masters cut by resolution as well as by byte quota.  A cut (reduce r, quota Q) of a master M is defined as the
existing re-cut at Q of the derived stream M_r (tests/reduced_model.derive) by a plain recutter made for the geometry at
1/2^r size: that, run on the device by Recutter.recut_torch on host-derived masters, is the expected value.  Masters are
encoded on the device: mixed batches of odd image sizes, and one frame of several thousand units.  Generous cuts are
derive(M, r) itself, chain into the decoder made for stages - r without the host and give what the reduced decode of the
masters gives.  (The same source runs on the CPU in tests/test_recut_cuts_mock.py.)"""
import numpy as np
import pytest

from icer_compression_amd import decoder, synth
from tests import encoder_batch_cases as ebc
from tests import reduced_model as rm
from tests import test_gpu_ladder as tl
from tests import test_gpu_recut as tg
from tests.decoder_batch_cases import oracle_decode
from tests.test_gpu_recut import expected, torch             # noqa: F401  (fixtures)
from tests.test_recut_cuts_mock import check_packets, mixed_cuts, reduced_geometry

pytestmark = pytest.mark.gpu

SENT, SENT_SIZE, SENT_RC = tg.SENT, tg.SENT_SIZE, tg.SENT_RC
QUOTA_EXCEEDED, OUT_OF_DATA, INVALID_INPUT = tg.QUOTA_EXCEEDED, tg.OUT_OF_DATA, tg.INVALID_INPUT

YUV = ebc.Geometry(250, 187, 3, 3, 1, 5)
GRAY8 = ebc.Geometry(250, 187, 1, 3, 0, 6, bits=8)
MIXED = {
    "yuv": (YUV, [("smooth", 0), ("noise8", 1), ("blank", 0), ("overflow", 7), ("sparse", 1), (("sparse", "dot", "wide"), 2)]),
    "gray8": (GRAY8, [("blank8", 0), ("noise6", 3), ("smooth6", 2), ("full8", 3), ("noise6", 4)]),
}


def recutter(g, max_reduce=None):
    return decoder.Recutter(g.w, g.h, g.channels, g.stages, g.segments, bits=g.bits,
                            max_reduce=g.stages - 1 if max_reduce is None else max_reduce)


def recut_cuts(torch, r, data, lens, cuts, offsets=None, stream_stride=None):
    """recut_cuts_torch into len(cuts) * n + 1 rows / entries filled with a sentinel (stride odd: rows start at every byte
    alignment).  Returns res[c][f] = (rc, stream) after checking the buffer promises."""
    n, Q = int(lens.shape[0]), len(cuts)
    quotas = [q for _, q in cuts]
    stride = (max(quotas) + 5) | 1
    keep = data.clone()
    out = torch.full((Q * n + 1, stride), SENT, dtype=torch.uint8, device=data.device)
    sizes = torch.full((Q * n + 1,), SENT_SIZE, dtype=torch.int64, device=data.device)
    rcs = torch.full((Q * n + 1,), SENT_RC, dtype=torch.int32, device=data.device)
    r.recut_cuts_torch(data, lens, cuts, out[: Q * n], sizes[: Q * n], rcs[: Q * n], offsets=offsets, stream_stride=stream_stride)
    torch.cuda.synchronize()
    assert torch.equal(data, keep), "the masters were modified on the device"
    return tg.read_rows(out, sizes, rcs, n, quotas)


def by_definition(torch, g, streams, cuts, rng):
    """want[c][f] = (rc, stream): Recutter.recut_torch of a plain recutter for the geometry at 1/2^r size on derive(M, r),
    prepared on the host and uploaded; one call per reduce"""
    want = [None] * len(cuts)
    for r in sorted({c[0] for c in cuts}):
        idx = [i for i, c in enumerate(cuts) if c[0] == r]
        derived = [rm.derive(s, r) if r else s for s in streams]
        plain = tg.recutter(reduced_geometry(g, r))
        data, offsets, lens = tg.blob_of(torch, rng, derived)
        got = tg.recut(torch, plain, data, lens, [cuts[i][1] for i in idx], offsets=offsets)
        plain.close()
        for j, i in enumerate(idx):
            want[i] = got[j]
    return want


def host_streams(masters, sizes):
    host, sz = masters.cpu().numpy(), sizes.cpu().numpy()
    return [host[f, : int(sz[f])].tobytes() for f in range(host.shape[0])]


def check_cuts(got, want, cuts, what):
    for c, cut in enumerate(cuts):
        for f in range(len(want[c])):
            ebc.check_frame(*got[c][f], want[c][f], f"{what}: cut {cut} frame {f}")
            check_packets(got[c][f][1], f"{what}: cut {cut} frame {f}")


# ---- 1. mixed batches encoded on the device: the definition, the derived stream itself, reduce 0 ---------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_batches_cut_by_resolution(torch, oracle, name):
    g, specs = MIXED[name]
    aborted = [f for f, (kind, _) in enumerate(specs) if kind in tg.ABORTED]
    assert len(aborted) == 1 and 5 <= len(specs) <= 6
    rng = np.random.default_rng(sum(map(ord, name)))
    enc, r = tg.encoder(g, len(specs)), recutter(g)
    assert r.max_reduce == g.stages - 1
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, enc_rcs = tg.encode_masters(torch, enc, t, ebc.quota(g, "lossless"))
    assert [int(x) for x in enc_rcs.cpu()] == [-1 if f in aborted else 0 for f in range(len(specs))]
    streams = host_streams(masters, sizes)
    # the definition, from the encoder's buffers as they are (rows of a stride) and from a blob of odd offsets
    cuts = mixed_cuts(g, streams, rng)
    want = by_definition(torch, g, streams, cuts, rng)
    check_cuts(recut_cuts(torch, r, masters, sizes, cuts), want, cuts, f"{name}, rows")
    data, offsets, lens = tg.blob_of(torch, rng, streams)
    check_cuts(recut_cuts(torch, r, data, lens, cuts, offsets=offsets), want, cuts, f"{name}, odd offsets")
    for c in range(len(cuts)):
        assert want[c][aborted[0]] == (OUT_OF_DATA, b""), "an aborted frame has an empty master"
    # generous cuts: derive(M, r) itself, whose plain decode at stages - r is the reduced decode of M
    generous = [(red, max(len(rm.derive(s, red)) for s in streams) + 1) for red in range(g.stages)]
    got = recut_cuts(torch, r, masters, sizes, generous)
    for c, (red, _) in enumerate(generous):
        rw, rh = rm.reduced_size(g.w, g.h, red)
        for f in range(len(specs)):
            if f in aborted:
                assert got[c][f] == (OUT_OF_DATA, b"")
                continue
            ebc.check_frame(*got[c][f], (0, rm.derive(streams[f], red)), f"{name}: generous cut at r {red} frame {f}")
            have = oracle_decode(oracle, got[c][f][1], g.channels, g.stages - red, g.filt, g.segments, rw * rh, g.bits)
            wanted = rm.expected(oracle, streams[f], red, g.channels, g.stages, g.filt, g.segments, rw * rh, g.bits)
            assert have[:3] == wanted[:3] == (0, rw, rh), (name, red, f)
            assert all(np.array_equal(a, b) for a, b in zip(have[3], wanted[3])), (name, red, f)
    # reduce 0 is the byte-quota re-cut, alone and next to another reduce; a plain recutter refuses reduce 1
    quotas = [ebc.quota(g, c) for c in ("lossless", "cut", "progressive", "tiny60")]
    plain = tg.recutter(g)
    assert plain.max_reduce == 0
    same = tg.recut(torch, plain, masters, sizes, quotas)
    assert recut_cuts(torch, r, masters, sizes, [(0, q) for q in quotas]) == same
    assert recut_cuts(torch, plain, masters, sizes, [(0, q) for q in quotas]) == same
    assert recut_cuts(torch, r, masters, sizes, [(0, q) for q in quotas] + [(2, quotas[1])])[: len(quotas)] == same
    assert tg.recut(torch, r, masters, sizes, quotas) == same
    with pytest.raises(RuntimeError, match="icerx_recut_device_cuts_async: -11"):
        recut_cuts(torch, plain, masters, sizes, [(0, quotas[0]), (1, quotas[1])])
    assert enc.stats()["unit_timeouts"] == 0
    plain.close()
    enc.close()
    r.close()


# ---- 2. several thousand units -----------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_multi_segment_frame_of_3744_units(torch):
    g = ebc.Geometry(1021, 765, 1, 4, 0, 32)
    enc, r = tg.encoder(g, 1), recutter(g, max_reduce=3)
    t = synth.gray_frames_torch(1, g.w, g.h, 4321, torch.device("cuda", 0))
    masters, sizes, enc_rcs = tg.encode_masters(torch, enc, t, ebc.quota(g, "lossless"))
    assert int(enc_rcs[0]) == 0
    streams = host_streams(masters, sizes)
    assert len(list(rm.walk(streams[0]))) == (3 * g.stages + 1) * 9 * g.segments == 3744
    rng = np.random.default_rng(9)
    cuts = []
    for red in (0, 1, 3):
        top = len(rm.derive(streams[0], red))
        cuts += [(red, top + 1), (red, top // 2), (red, top // 5)]
    cuts += [(3, 60), (1, 28), (0, 27), cuts[4]]
    rng.shuffle(cuts)
    cuts = [(int(a), int(b)) for a, b in cuts]
    got = recut_cuts(torch, r, masters, sizes, cuts)
    check_cuts(got, by_definition(torch, g, streams, cuts, rng), cuts, "1021 x 765 gray, 32 segments")
    for c, (red, quota) in enumerate(cuts):
        if quota > len(rm.derive(streams[0], red)):
            ebc.check_frame(*got[c][0], (0, rm.derive(streams[0], red)), f"generous cut at r {red}")
    plain = tg.recutter(g)
    quotas = [q for red, q in cuts if red == 0]
    assert [got[c] for c, (red, _) in enumerate(cuts) if red == 0] == tg.recut(torch, plain, masters, sizes, quotas)
    assert enc.stats()["unit_timeouts"] == 0
    plain.close()
    enc.close()
    r.close()


# ---- 3. damage, bad frames -------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_damaged_masters_and_bad_frames(torch, expected):
    g = YUV
    S = g.stages
    other = ebc.Geometry(249, 188, 3, 3, 1, 5)              # (at r = 1 its packets would be resized to the recutter's 125 x 94)
    assert rm.reduced_size(other.w, other.h, 1) == rm.reduced_size(g.w, g.h, 1)
    specs = [("smooth", 0), ("noise8", 1)]
    enc = tg.encoder(g, len(specs))
    t = tl.device_frames(ebc.batch(g, specs))
    masters, sizes, _ = tg.encode_masters(torch, enc, t, ebc.quota(g, "lossless"))
    good = host_streams(masters, sizes)
    enc.close()
    rng = np.random.default_rng(3)
    r = recutter(g)
    # damage: a level-1 payload, a level-S header, the level-1 packets alone
    low = rm.flip_in_packet(good[1], 1, False, which=2)
    head = rm.flip_in_packet(good[1], S, True, which=1)
    only1 = b"".join(good[1][o: o + n] for o, n in rm.walk(good[1]) if good[1][o + 4] == 1)
    streams = [good[1], low, head, only1]
    top = len(good[1]) + 3
    cuts = [(red, q) for red in range(S) for q in (top, len(rm.derive(good[1], red)) // 2)]
    data, offsets, lens = tg.blob_of(torch, rng, streams)
    got = recut_cuts(torch, r, data, lens, cuts, offsets=offsets)
    check_cuts(got, by_definition(torch, g, streams, cuts, rng), cuts, "damaged masters")
    for c, (red, quota) in enumerate(cuts):
        assert got[c][1] == got[c][0] or red == 0, (red, quota)
        assert got[c][1] != got[c][0] or (red, quota) != (0, top), (red, quota)
        assert got[c][2][0] == QUOTA_EXCEEDED and (quota != top or len(got[c][2][1]) < len(got[c][0][1])), (red, quota)
        assert red == 0 or got[c][3] == (OUT_OF_DATA, b""), (red, quota)
    # bad frames: six frames, the two good ones untouched
    junk = rng.integers(0, 256, 5000).astype(np.uint8).tobytes()
    alien = expected(other, ("smooth", 0), ebc.quota(other, "lossless"))[1]
    data, offsets, lens = tg.blob_of(torch, rng, [good[0], junk, alien, b"", good[1]])
    offsets = torch.cat([offsets, torch.tensor([data.numel() - 10], dtype=torch.int64, device="cuda")])    # (leaves the blob)
    lens = torch.cat([lens, torch.tensor([11], dtype=torch.int64, device="cuda")])
    cuts = [(0, ebc.quota(g, "cut")), (1, top), (2, 60), (2, top), (1, 5000)]
    got = recut_cuts(torch, r, data, lens, cuts, offsets=offsets)
    want = by_definition(torch, g, good, cuts, rng)
    for c, cut in enumerate(cuts):
        for j, f in enumerate((0, 4)):
            ebc.check_frame(*got[c][f], want[c][j], f"a neighbour of bad frames: cut {cut} frame {f}")
        assert [got[c][f] for f in (1, 2, 3, 5)] == [(OUT_OF_DATA, b""), (INVALID_INPUT, b""), (OUT_OF_DATA, b""), (INVALID_INPUT, b"")], cut
    r.close()


# ---- 4. encoder -> cut -> decoder for stages - r on one stream -------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", list(MIXED))
def test_chain_cut_into_the_decoder_without_the_host(torch, name):
    g, specs = MIXED[name]
    # (not the aborted frames, and not the "wide" one: 12-bit noise has coefficients above the nine coded planes, its chains
    # read on into the bytes that follow the packet, and those differ between a master and its derived stream -- the
    # documented exception of the reduced decode's definition)
    specs = [s for s in specs if s[0] not in tg.ABORTED and "wide" not in s[0]]
    n, S = len(specs), g.stages
    assert n >= 3
    mq = ebc.quota(g, "lossless")
    cuts = [(red, mq) for red in range(1, S)]                # (generous: above any stream of this geometry)
    enc, r = tg.encoder(g, n), recutter(g)
    dt = torch.int16 if g.bits == 16 else torch.uint8
    st = torch.cuda.Stream()
    decs = []
    try:
        with torch.cuda.stream(st):
            t = tl.device_frames(ebc.batch(g, specs))
            masters, sizes, _ = tg.encode_masters(torch, enc, t, mq)
            out = torch.zeros((len(cuts), n, mq + 3), dtype=torch.uint8, device="cuda")
            cut_sizes = torch.zeros((len(cuts), n), dtype=torch.int64, device="cuda")
            cut_rcs = torch.zeros((len(cuts), n), dtype=torch.int32, device="cuda")
            r.recut_cuts_torch(masters, sizes, cuts, out, cut_sizes, cut_rcs)
            res = []
            for c, (red, _) in enumerate(cuts):
                rw, rh = rm.reduced_size(g.w, g.h, red)
                pair = []
                # a plain decoder for stages - r on the cut's block of rows as it is; a reduced decoder on the masters
                for d, data, lens in ((decoder.Decoder(g.channels, S - red, g.filt, g.segments, bits=g.bits), out[c], cut_sizes[c]),
                                      (decoder.Decoder(g.channels, S, g.filt, g.segments, bits=g.bits, reduce=red), masters, sizes)):
                    decs.append(d)
                    planes = torch.full((n, g.channels, rw * rh), 0x5A, dtype=dt, device="cuda")
                    rcs = torch.full((n,), 77, dtype=torch.int32, device="cuda")
                    ws, hs = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
                    d.decode_torch(data, lens, planes, rcs, ws, hs, stream_stride=data.stride(0))
                    pair.append((planes, rcs, ws, hs))
                res.append(pair)
        st.synchronize()
        assert cut_rcs.cpu().tolist() == [[0] * n] * len(cuts)
        for (red, _), (cut, reduced) in zip(cuts, res):
            rw, rh = rm.reduced_size(g.w, g.h, red)
            assert cut[1].cpu().tolist() == reduced[1].cpu().tolist() == [0] * n, (name, red)
            assert cut[2].cpu().tolist() == reduced[2].cpu().tolist() == [rw] * n and cut[3].cpu().tolist() == reduced[3].cpu().tolist() == [rh] * n
            assert torch.equal(cut[0], reduced[0]), (name, red)
    finally:
        for d in decs:
            d.close()
        enc.close()
        r.close()


# ---- 5. two calls in flight ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_two_calls_in_flight_on_two_streams(torch, expected):
    """one recutter, two streams, a workspace each (recut_cuts_torch keeps one per stream): the rows of one call after the other"""
    g = YUV
    specs = [("smooth", 0), ("noise8", 1), (("sparse", "dot", "wide"), 2)]
    mq = ebc.quota(g, "lossless")
    streams = [expected(g, s, mq)[1] for s in specs]
    cuts = [(1, ebc.quota(g, "progressive")), (0, 60), (2, mq), (0, ebc.quota(g, "cut")), (1, mq)]
    n, Q, stride = len(specs), len(cuts), (mq + 5) | 1
    r = recutter(g)
    data, offsets, lens = tg.blob_of(torch, np.random.default_rng(0), streams)
    alone = recut_cuts(torch, r, data, lens, cuts, offsets=offsets)
    runs = []
    for k, st in enumerate((torch.cuda.Stream(), torch.cuda.Stream())):
        order = list(range(n)) if k == 0 else list(reversed(range(n)))
        with torch.cuda.stream(st):
            data, offsets, lens = tg.blob_of(torch, np.random.default_rng(k), [streams[f] for f in order])
            out = torch.full((Q * n + 1, stride), SENT, dtype=torch.uint8, device="cuda")
            sizes = torch.full((Q * n + 1,), SENT_SIZE, dtype=torch.int64, device="cuda")
            rcs = torch.full((Q * n + 1,), SENT_RC, dtype=torch.int32, device="cuda")
            torch.cuda._sleep(int(10e-3 * 2.1e9))
            r.recut_cuts_torch(data, lens, cuts, out[: Q * n], sizes[: Q * n], rcs[: Q * n], offsets=offsets)
        runs.append((order, out, sizes, rcs, data))
    assert len(r._cuts_workspaces) >= 3
    torch.cuda.synchronize()
    for order, out, sizes, rcs, _ in runs:
        got = tg.read_rows(out, sizes, rcs, n, [q for _, q in cuts])
        for c, cut in enumerate(cuts):
            for k, f in enumerate(order):
                assert got[c][k] == alone[c][f], f"two streams: cut {cut} frame {f}"
    r.close()
