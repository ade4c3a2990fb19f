"""icerx_recut_device_cuts_async end to end on the CPU (the mock build of tests/test_recut_mock.py): stored masters cut by
resolution as well as by byte quota.  A cut (reduce r, quota Q) of a master M is DEFINED as the existing re-cut at Q of the
derived stream M_r (tests/reduced_model.derive) by a plain recutter made for the geometry at 1/2^r size, so that is the
expected value: bytes, size and return code.  Independently of any recutter, a generous cut of a complete master is
derive(M, r) itself, every packet of every cut verifies both CRCs, and the oracle -- and the unmodified reference decoder --
decode the cuts at stages - r.  Odd image sizes, so that every ceil matters.  The frame kinds are those of
test_recut_mock.GEOMETRIES with one addition for the 8-bit gray geometry (see GEOMETRIES below).  CPU only."""
import zlib

import numpy as np
import pytest

from tests import encoder_batch_cases as ebc
from tests import reduced_model as rm
from tests import test_recut_mock as trm
from tests.decoder_batch_cases import oracle_decode
from tests.test_recut_mock import expected, mock_lib        # noqa: F401  (fixtures: the oracle's streams, the mock build)

SENT, SENT_SIZE, SENT_RC = trm.SENT, trm.SENT_SIZE, trm.SENT_RC
QUOTA_EXCEEDED, OUT_OF_DATA, INVALID_INPUT, FATAL = trm.QUOTA_EXCEEDED, trm.OUT_OF_DATA, trm.INVALID_INPUT, trm.FATAL
GUARD = trm.GUARD

# (w, h, channels, stages, filter, segments, bits) with the frame kinds of test_recut_mock.GEOMETRIES.  At 250 x 187 the uint8
# frame ("noise6", 1) overflows in the transform (the oracle returns ICER_INTEGER_OVERFLOW and no stream): it stays as an
# empty master, which every cut answers with ICER_DECODER_OUT_OF_DATA, and a dense frame of another seed is added.
OVERFLOW = -1
GEOMETRIES = {
    "yuv16": (ebc.Geometry(250, 187, 3, 3, 1, 5), trm.GEOMETRIES["yuv16"][1]),
    "gray16": (ebc.Geometry(509, 383, 1, 4, 3, 2), trm.GEOMETRIES["gray16"][1]),
    "gray8": (ebc.Geometry(250, 187, 1, 3, 0, 6, bits=8), trm.GEOMETRIES["gray8"][1] + [("noise6", 3)]),
    "yuv8": (ebc.Geometry(125, 93, 3, 3, 0, 5, bits=8), trm.GEOMETRIES["yuv8"][1]),
}


def reduced_geometry(g, r):
    w, h = rm.reduced_size(g.w, g.h, r)
    return g._replace(w=w, h=h, stages=g.stages - r)


def recutter(lib, g, max_reduce=None):
    from icer_compression_amd import decoder
    return decoder.Recutter(g.w, g.h, g.channels, g.stages, g.segments, bits=g.bits, lib=lib,
                            max_reduce=g.stages - 1 if max_reduce is None else max_reduce)


def cuts_call(r, blob, offsets, lens, cuts, stream_stride=0, stride=None, ws_bytes=None, **override):
    """icerx_recut_device_cuts_async on host arrays (the mock's device memory) into len(cuts) * n + 1 sentinel rows of an odd
    stride -> (rc of the call, res[c][f] = (rc, stream)) after checking the buffer promises (test_recut_mock.recut_call)"""
    n, Q = len(lens), len(cuts)
    reduces, quotas = [c[0] for c in cuts], [c[1] for c in cuts]
    stride = stride or (max(quotas) + 5) | 1
    out = np.full((Q * n + 1, stride), SENT, np.uint8)
    sizes = np.full(Q * n + 1, SENT_SIZE, np.uint64)
    rcs = np.full(Q * n + 1, SENT_RC, np.int32)
    offs = np.asarray(offsets, np.uint64) if offsets is not None else None
    ln = np.asarray(lens, np.uint64)
    keep = blob.copy()
    need = r.cuts_workspace_bytes(n, len(blob), Q)
    work = np.full(need + GUARD, 0xCD, np.uint8)                        # (the call is handed `need` bytes; a guard tail behind them)
    args = dict(n=n, d_data=blob.ctypes.data, data_bytes=len(blob), d_offsets=offs.ctypes.data if offs is not None else None,
                stream_stride=stream_stride, d_lens=ln.ctypes.data, reduces=reduces, quotas=quotas, d_out=out.ctypes.data,
                out_stride=stride, d_sizes=sizes.ctypes.data, d_rcs=rcs.ctypes.data, d_workspace=work.ctypes.data,
                workspace_bytes=need if ws_bytes is None else ws_bytes, stream=None)
    args.update(override)
    rc = r.recut_cuts_device_async_ptrs(**args)
    assert (work[need:] == 0xCD).all(), "written behind the workspace"
    assert np.array_equal(blob, keep), "the masters were modified"
    if rc != 0:
        assert (out == SENT).all() and (sizes == SENT_SIZE).all() and (rcs == SENT_RC).all(), "a refused call wrote"
        return rc, None
    assert (out[Q * n] == SENT).all() and sizes[Q * n] == SENT_SIZE and rcs[Q * n] == SENT_RC, "written past the n_cuts * n rows"
    res = []
    for c, quota in enumerate(quotas):
        row = []
        for f in range(n):
            k = c * n + f
            s = int(sizes[k])
            assert 0 <= s <= quota, (c, f, s, quota)
            assert (out[k, s:] == SENT).all(), f"cut {c} frame {f}: bytes written behind its stream of {s} bytes"
            row.append((int(rcs[k]), out[k, :s].tobytes()))
        res.append(row)
    return rc, res


def both_layouts(rng, streams, call):
    """call(blob, offsets, lens, stream_stride) with the masters at odd offsets with junk between them, then in rows of a stride"""
    blob, offsets = trm.pack_odd(rng, streams)
    rows, stride = trm.pack_rows(streams)
    lens = [len(s) for s in streams]
    return (("odd offsets", call(blob, offsets, lens, 0)), ("stride", call(rows, None, lens, stride)))


def by_definition(lib, g, streams, cuts, rng):
    """want[c][f] = (rc, stream): the existing icerx_recut_device_async of a plain recutter for the geometry at 1/2^r size on
    derive(M, r), one call per reduce"""
    want = [None] * len(cuts)
    for r in sorted({c[0] for c in cuts}):
        idx = [i for i, c in enumerate(cuts) if c[0] == r]
        derived = [rm.derive(s, r) if r else s for s in streams]
        plain = trm.recutter(lib, reduced_geometry(g, r))
        blob, offsets = trm.pack_odd(rng, derived)
        rc, got = trm.recut_call(plain, blob, offsets, [len(s) for s in derived], [cuts[i][1] for i in idx])
        plain.close()
        assert rc == 0
        for j, i in enumerate(idx):
            want[i] = got[j]
    return want


def mixed_cuts(g, streams, rng):
    """every r in 0 .. S - 1 with quotas above, at half and at a fifth of the longest derived master, 60 / 28 / 27 bytes at
    some r each, and one cut twice; shuffled.  13 cuts for 3 stages, 16 for 4."""
    cuts = []
    for r in range(g.stages):
        top = max(len(rm.derive(s, r)) for s in streams)
        cuts += [(r, top + 9), (r, top // 2), (r, top // 5)]
    cuts += [(int(rng.integers(0, g.stages)), q) for q in (60, 28, 27)]
    cuts.append(cuts[int(rng.integers(0, len(cuts)))])
    rng.shuffle(cuts)
    cuts = [(int(r), int(q)) for r, q in cuts]
    assert len(cuts) <= 16
    return cuts


def masters_of(expected, g, specs, cls):
    mq = ebc.quota(g, cls)
    masters = [expected(g, s, mq) for s in specs]
    assert all(m[0] in (0, QUOTA_EXCEEDED) or (m[0] == OVERFLOW and m[1] == b"") for m in masters)
    assert sum(m[0] == OVERFLOW for m in masters) <= 1
    return [m[1] for m in masters], [m[0] for m in masters]


def check_packets(stream, what):
    """the stream is a run of packets whose header CRC and payload CRC verify, and nothing else"""
    at = 0
    for off, n in rm.walk(stream):
        assert off == at, f"{what}: bytes {at} .. {off} belong to no valid packet"
        assert zlib.crc32(stream[off: off + 24]) == int.from_bytes(stream[off + 24: off + 28], "little"), what
        assert zlib.crc32(stream[off + 28: off + n]) == int.from_bytes(stream[off + 20: off + 24], "little"), what
        at = off + n
    assert at == len(stream), f"{what}: {len(stream) - at} bytes behind the last valid packet"


@pytest.mark.parametrize("master_cls", ["lossless", "cut"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_cuts_equal_the_definition(mock_lib, expected, name, master_cls):
    g, specs = GEOMETRIES[name]
    rng = np.random.default_rng(sum(map(ord, name + master_cls)))
    streams, mrcs = masters_of(expected, g, specs, master_cls)
    assert master_cls == "lossless" or any(rc == QUOTA_EXCEEDED for rc in mrcs), "no master of this batch is cut"
    cuts = mixed_cuts(g, streams, rng)
    assert g.stages != 4 or len(cuts) == 16, "the 4-stage geometry makes the call with exactly ICERX_MAX_LADDER cuts"
    want = by_definition(mock_lib, g, streams, cuts, rng)
    r = recutter(mock_lib, g)
    assert r.max_reduce == g.stages - 1
    for what, (rc, got) in both_layouts(rng, streams, lambda b, o, ln, st: cuts_call(r, b, o, ln, cuts, stream_stride=st)):
        assert rc == 0, what
        for c, cut in enumerate(cuts):
            for f, spec in enumerate(specs):
                ebc.check_frame(*got[c][f], want[c][f], f"{name} {master_cls} master, {what}: cut {cut} frame {f} {spec}")
                check_packets(got[c][f][1], f"{name} {master_cls} master, {what}: cut {cut} frame {f}")
    r.close()


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_generous_cut_is_the_derived_stream(mock_lib, expected, oracle, name):
    """no recutter in the expected value: derive(M, r) byte for byte with rc 0, and the oracle's plain decode of it at
    stages - r is the reduced decode of M at r.  Generous is a quota ABOVE the derived stream's length: the quota walk keeps a
    unit iff floor(bits / 8) < quota - used - 28, so at a quota of exactly that length it can drop the last unit, as an
    encode at that quota does."""
    g, specs = GEOMETRIES[name]
    rng = np.random.default_rng(11)
    streams, mrcs = masters_of(expected, g, specs, "lossless")
    streams, specs = [s for s, rc in zip(streams, mrcs) if rc == 0], [s for s, rc in zip(specs, mrcs) if rc == 0]
    assert len(streams) >= 3
    derived = [[rm.derive(s, r) for s in streams] for r in range(g.stages)]
    cuts = [(r, max(len(d) for d in derived[r]) + k) for r in range(g.stages) for k in (1, 77)]
    r = recutter(mock_lib, g)
    for what, (rc, got) in both_layouts(rng, streams, lambda b, o, ln, st: cuts_call(r, b, o, ln, cuts, stream_stride=st)):
        assert rc == 0, what
        for c, (red, _) in enumerate(cuts):
            for f in range(len(specs)):
                ebc.check_frame(*got[c][f], (0, derived[red][f]), f"{name} {what}: generous cut at r {red} frame {f}")
    for c, (red, _) in enumerate(cuts[::2]):
        rw, rh = rm.reduced_size(g.w, g.h, red)
        for f in range(len(specs)):
            have = oracle_decode(oracle, got[2 * c][f][1], g.channels, g.stages - red, g.filt, g.segments, rw * rh, g.bits)
            want = rm.expected(oracle, streams[f], red, g.channels, g.stages, g.filt, g.segments, rw * rh, g.bits)
            assert have[:3] == want[:3] == (0, rw, rh), (name, red, f)
            assert all(np.array_equal(a, b) for a, b in zip(have[3], want[3])), (name, red, f)
    r.close()


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_reference_decoder_decodes_the_cuts(mock_lib, expected, oracle, reference, name):
    """the unmodified reference decoder, told stages - r, decodes the generous cut and a mid-quota cut to the oracle's image"""
    g, specs = GEOMETRIES[name]
    streams, mrcs = masters_of(expected, g, specs[:3], "lossless")
    streams = [s for s, rc in zip(streams, mrcs) if rc == 0][:2]
    cuts = []
    for red in range(1, g.stages):
        top = max(len(rm.derive(s, red)) for s in streams)
        cuts += [(red, top + 1), (red, top // 3)]
    r = recutter(mock_lib, g)
    blob, offsets = trm.pack_odd(np.random.default_rng(3), streams)
    rc, got = cuts_call(r, blob, offsets, [len(s) for s in streams], cuts)
    assert rc == 0
    for c, (red, quota) in enumerate(cuts):
        rw, rh = rm.reduced_size(g.w, g.h, red)
        for f in range(len(streams)):
            rc_f, s = got[c][f]
            assert rc_f == 0 if c % 2 == 0 else rc_f in (0, QUOTA_EXCEEDED), (name, red, quota, f)
            assert len(s) > 28, (name, red, quota, f)
            ref = reference.decompress_raw(s, g.channels, g.stages - red, g.filt, g.segments, rw * rh, g.bits)
            orc = oracle_decode(oracle, s, g.channels, g.stages - red, g.filt, g.segments, rw * rh, g.bits)
            assert ref[:3] == orc[:3] and ref[1:3] == (rw, rh), (name, red, quota, f, ref[:3], orc[:3])
            assert all(np.array_equal(a, b) for a, b in zip(ref[3], orc[3])), (name, red, quota, f)
    r.close()


@pytest.mark.parametrize("name", ["yuv16", "gray8"])
def test_reduce_0_is_the_existing_recut(mock_lib, expected, name):
    g, specs = GEOMETRIES[name]
    rng = np.random.default_rng(17)
    streams, _ = masters_of(expected, g, specs, "lossless")
    quotas = [ebc.quota(g, c) for c in ("lossless", "cut", "progressive", "tiny60")]
    lens = [len(s) for s in streams]
    blob, offsets = trm.pack_odd(rng, streams)
    plain = trm.recutter(mock_lib, g)
    assert plain.max_reduce == 0 and mock_lib.icerx_recutter_max_reduce(plain.handle) == 0 and mock_lib.icerx_recutter_max_reduce(None) == 0
    rc, want = trm.recut_call(plain, blob, offsets, lens, quotas)
    assert rc == 0
    r = recutter(mock_lib, g)
    # all reduces 0, and reduce 0 next to another reduce
    for cuts in ([(0, q) for q in quotas], [(0, q) for q in quotas] + [(1, quotas[1])]):
        for rec in (r, plain) if cuts[-1][0] == 0 else (r,):
            rc, got = cuts_call(rec, blob, offsets, lens, cuts)
            assert rc == 0
            assert got[: len(quotas)] == want, cuts
    # the byte-quota entry point of a recutter made with max_reduce
    assert trm.recut_call(r, blob, offsets, lens, quotas) == (0, want)
    assert r.workspace_bytes(len(lens), len(blob), 4) == plain.workspace_bytes(len(lens), len(blob), 4)
    assert cuts_call(plain, blob, offsets, lens, [(0, quotas[0]), (1, quotas[1])])[0] == INVALID_INPUT, "a plain recutter refuses reduce 1"
    plain.close()
    r.close()
    if name != "gray8":
        return
    # the same entry point on test_recut_mock's gray8 geometry (256 x 192, several segments, the 8-bit final order), where the
    # oracle's streams are the expected value: a recutter that holds reduced geometries works in the byte-quota call's own,
    # smaller workspace (recut_call hands it just that much and checks the bytes behind it)
    g, specs = trm.GEOMETRIES["gray8"]
    mq = ebc.quota(g, "lossless")
    masters = [expected(g, s, mq) for s in specs]
    quotas = [ebc.quota(g, c) for c in ("lossless", "cut", "progressive", "tiny60")]
    blob, offsets = trm.pack_odd(rng, [m[1] for m in masters])
    r = recutter(mock_lib, g)
    assert r.max_reduce == g.stages - 1 and r.workspace_bytes(len(masters), len(blob), 4) < r.cuts_workspace_bytes(len(masters), len(blob), 4)
    rc, got = trm.recut_call(r, blob, offsets, [len(m[1]) for m in masters], quotas)
    assert rc == 0
    for q, quota in enumerate(quotas):
        for f, spec in enumerate(specs):
            ebc.check_frame(*got[q][f], trm.wanted(expected, g, spec, masters[f], mq, quota), f"quota {quota} frame {f} {spec}")
    r.close()


@pytest.mark.parametrize("name", ["yuv16", "gray16", "yuv8"])
def test_damage(mock_lib, expected, name):
    g, specs = GEOMETRIES[name]
    S = g.stages
    rng = np.random.default_rng(23)
    master = masters_of(expected, g, specs[:1], "lossless")[0][0]
    top = len(master) + 3
    cuts = [(r, q) for r in range(S) for q in (top, len(rm.derive(master, r)) // 2)]
    low = rm.flip_in_packet(master, 1, False, which=2)                        # a level-1 payload
    head = rm.flip_in_packet(master, S, True, which=1)                         # a level-S header
    body = rm.flip_in_packet(master, S, False, which=3, subband=0)             # a level-S payload of LL
    only1 = b"".join(master[o: o + n] for o, n in rm.walk(master) if master[o + 4] == 1)
    assert only1 and len(only1) < len(master)
    streams = [master, low, head, body, only1]
    want = by_definition(mock_lib, g, streams, cuts, rng)
    r = recutter(mock_lib, g)
    blob, offsets = trm.pack_odd(rng, streams)
    rc, got = cuts_call(r, blob, offsets, [len(s) for s in streams], cuts)
    assert rc == 0
    for c, (red, quota) in enumerate(cuts):
        for f in range(len(streams)):
            ebc.check_frame(*got[c][f], want[c][f], f"{name}: cut {(red, quota)} frame {f}")
        # damage at level 1 is invisible from r = 1 on, and cuts the r = 0 stream
        assert got[c][1] == got[c][0] or red == 0, (red, quota)
        assert got[c][1] != got[c][0] or (red, quota) != (0, top), (red, quota)
        # damage at level S cuts every r at that unit
        for f in (2, 3):
            assert got[c][f][0] == QUOTA_EXCEEDED and len(got[c][f][1]) <= len(got[c][0][1]), (red, quota, f)
        if quota == top:
            assert len(got[c][2][1]) < len(got[c][0][1]) and len(got[c][3][1]) < len(got[c][0][1]), (red, quota)
        # level-1 packets only: no stream from r = 1 on, the existing result at r = 0
        if red >= 1:
            assert got[c][4] == (OUT_OF_DATA, b""), (red, quota)
    plain = trm.recutter(mock_lib, g)
    rc0, got0 = trm.recut_call(plain, blob, offsets, [len(s) for s in streams], [top])
    assert rc0 == 0 and got0[0][4] == got[0][4] and cuts[0] == (0, top)
    plain.close()
    r.close()


def test_bad_frames_and_refused_calls(mock_lib, expected):
    g, specs = GEOMETRIES["gray16"]
    other = ebc.Geometry(510, 384, 1, 4, 3, 2)             # (at r = 1 its packets would be resized to the recutter's 255 x 192)
    assert rm.reduced_size(other.w, other.h, 1) == rm.reduced_size(g.w, g.h, 1)
    mq = ebc.quota(g, "lossless")
    good = [expected(g, s, mq)[1] for s in specs[:2]]
    alien = expected(other, ("smooth", 0), ebc.quota(other, "lossless"))[1]
    rng = np.random.default_rng(5)
    junk = rng.integers(0, 256, 3000).astype(np.uint8).tobytes()
    streams = [good[0], junk, alien, good[1], b""]
    blob, offsets = trm.pack_odd(rng, streams)
    lens = [len(s) for s in streams]
    offsets += [len(blob) - 10, len(blob) + 1]                          # two frames that leave the blob
    lens += [11, 0]
    cuts = [(0, ebc.quota(g, "cut")), (1, mq), (3, 60), (2, 5000), (3, mq), (1, 2000)]
    want = by_definition(mock_lib, g, good, cuts, rng)
    r = recutter(mock_lib, g)
    rc, got = cuts_call(r, blob, offsets, lens, cuts)
    assert rc == 0
    for c, cut in enumerate(cuts):
        for j, f in enumerate((0, 3)):
            ebc.check_frame(*got[c][f], want[c][j], f"a neighbour of bad frames: cut {cut} frame {f}")
        # (the alien frame: the status rule is the master's, also where derive would have dropped or resized its packets)
        assert [got[c][f] for f in (1, 2, 4, 5, 6)] == [(OUT_OF_DATA, b""), (INVALID_INPUT, b""), (OUT_OF_DATA, b""),
                                                         (INVALID_INPUT, b""), (INVALID_INPUT, b"")], cut
    # refused calls write nothing (cuts_call checks that)
    n = len(lens)
    need = r.cuts_workspace_bytes(n, len(blob), len(cuts))
    assert need >= r.workspace_bytes(n, len(blob), len(cuts))
    reduces, quotas = [c[0] for c in cuts], [c[1] for c in cuts]
    cases = {
        "null reduces": dict(reduces=None), "reduce above max_reduce": dict(reduces=[r.max_reduce + 1] + reduces[1:]),
        "negative reduce": dict(reduces=reduces[:-1] + [-1]),
        "no cuts": dict(n_cuts=0), "17 cuts": dict(reduces=[1] * 17, quotas=[60] * 17), "negative cut count": dict(n_cuts=-1),
        "no frames": dict(n=0), "negative frames": dict(n=-1), "too many frames": dict(n=65536),
        "null quotas": dict(quotas=None, n_cuts=2), "null data": dict(d_data=None), "null lens": dict(d_lens=None),
        "null out": dict(d_out=None), "null sizes": dict(d_sizes=None), "null rcs": dict(d_rcs=None), "null workspace": dict(d_workspace=None),
        "stride below the largest quota": dict(out_stride=mq - 1), "workspace too small": dict(workspace_bytes=need - 1),
    }
    for what, kw in cases.items():
        assert cuts_call(r, blob, offsets, lens, cuts, **kw)[0] == INVALID_INPUT, what
    assert cuts_call(r, blob, offsets, lens, cuts, data_bytes=0xFFFFFFFF - 64)[0] == FATAL
    assert r.lib.icerx_recut_device_cuts_async(None, n, blob.ctypes.data, len(blob), None, 0, None, None, None, 1, None, 0, None, None,
                                               None, 0, None) == INVALID_INPUT
    assert r.cuts_workspace_bytes(n, len(blob), 0) == 0 == r.cuts_workspace_bytes(n, len(blob), 17)
    r.close()
    for bad in (g.stages, -1):
        with pytest.raises(RuntimeError, match="icerx_recutter_create_reduced: -11 "):
            recutter(mock_lib, g, max_reduce=bad)
    with pytest.raises(RuntimeError, match="icerx_recutter_create_reduced: -4 "):           # (the planner's code for the full geometry)
        recutter(mock_lib, g._replace(stages=7), max_reduce=1)


@pytest.mark.parametrize("name", ["yuv16", "gray16", "yuv8"])
def test_cuts_compose(mock_lib, expected, name):
    """a stored output of cut (r, Q1), re-cut by a plain recutter of the geometry at 1/2^r size to Q2 < Q1, is cut (r, Q2)"""
    g, specs = GEOMETRIES[name]
    rng = np.random.default_rng(29)
    streams, _ = masters_of(expected, g, specs, "lossless")
    r = recutter(mock_lib, g)
    for red in range(1, g.stages):
        top = max(len(rm.derive(s, red)) for s in streams)
        q1s, q2s = [top + 1, top // 2], [top // 3, top // 7, 60]
        blob, offsets = trm.pack_odd(rng, streams)
        rc, got = cuts_call(r, blob, offsets, [len(s) for s in streams], [(red, q) for q in q1s + q2s])
        assert rc == 0
        plain = trm.recutter(mock_lib, reduced_geometry(g, red))
        for i in range(len(q1s)):
            stored = [s for _, s in got[i]]
            blob1, offsets1 = trm.pack_odd(rng, stored)
            rc, again = trm.recut_call(plain, blob1, offsets1, [len(s) for s in stored], q2s)
            assert rc == 0
            assert again == got[len(q1s):], (name, red, q1s[i])
        plain.close()
    r.close()
