"""Cases and scenarios of the decode-session tests, shared by tests/test_session_mock.py (the host pipeline on the mock HIP
runtime) and tests/test_gpu_session.py (the GPU): small frames whose level-1 chains are wider than 64 samples and whose packets
are mostly above 16 bits, so that the wave-per-plane kernel runs rows of several blocks; the oracle's nested quota cuts of them;
increments by tests/combine_model.py.  A scenario drives a `rig` -- rig.open(case, **decoder options) -> (session, model),
rig.feed(session, feeds, slots, display, sizes) -> (rcs, ws, hs, rows) with rows[k] the fed frame's output row filled with
SENT where nothing was written -- and compares every step with tests/session_model.py."""
import numpy as np

from tests import combine_model as cm
from tests import encoder_batch_cases as ebc
from tests import reduced_model as red
from tests import roi_model as rm
from tests import session_model as sm
from tests import target_model as tm
from tests.display_model import display_of
from tests.sweep_cut_cases import reads_on

SENT = 0x5A
CASES = {
    "gray16_A4": (ebc.Geometry(200, 136, 1, 3, 0, 4), ("smooth", 3)),
    "gray16_C1": (ebc.Geometry(200, 136, 1, 3, 2, 1), ("smooth", 1)),
    "yuv8": (ebc.Geometry(96, 80, 3, 3, 0, 3, bits=8), ("smooth6", 2)),
}
OTHER_SIZE = (ebc.Geometry(96, 80, 1, 3, 0, 4), ("smooth", 5))       # a frame of another size for gray16_A4's decoder
_MEMO = {}


def model_of(g):
    return tm.Model(g.w, g.h, g.channels, g.stages, g.filt, g.segments, g.bits)


def ladder(expected, name):
    """(g, master, [three nested cuts], [the first cut and the two increments]) of a case, by the oracle and combine_model"""
    if name not in _MEMO:
        g, spec = CASES[name]
        rc, master = expected(g, spec, ebc.quota(g, "lossless"))[:2]
        assert rc == 0
        L = len(master)
        cuts = [expected(g, spec, q)[1] for q in (L // 6, L // 3, (2 * L) // 3)]
        m = model_of(g)
        assert cm.units(m, cuts[0]) < cm.units(m, cuts[1]) < cm.units(m, cuts[2]) < cm.units(m, master)
        # (where a chain reads on into the bytes behind its packet, what ANY decoder makes of the packets depends on what follows
        # each -- tests/reduced_model.py; the cases are chosen so that none does)
        assert not any(reads_on(expected.orc, g, c, 0) for c in cuts), name
        incs = [cuts[0]] + [cm.combine(m, cuts[i], cuts[i + 1], cm.DIFFERENCE)[1] for i in range(2)]
        _MEMO[name] = (g, master, cuts, incs)
    return _MEMO[name]


def delivered(row, w, h, channels, stride):
    """the w * h samples (display: channels * w * h bytes, one row) a fed frame delivered, per channel"""
    return [row[c * stride: c * stride + w * h] for c in range(channels)]


def check_step(g, got, k, want, tag, display=False):
    """row k of a feed against the model's (rc, w, h, planes): planes None = refused, the row untouched"""
    rcs, ws, hs, rows = got
    rc, w, h, planes = want
    assert (rcs[k], ws[k], hs[k]) == (rc, w, h), (tag, k, rcs[k], ws[k], hs[k], want[:3])
    stride = rows[k].size // g.channels
    sent = SENT if rows[k].dtype == np.uint8 else SENT * 0x0101
    if planes is None or w * h == 0:
        assert (rows[k] == sent).all(), (tag, k, "a frame that delivers nothing was written")
        return
    if display:
        ref = display_of([p[: w * h] for p in planes], g.channels).reshape(-1)
        assert np.array_equal(rows[k][: ref.size], ref), (tag, k, "display image differs")
        assert (rows[k][ref.size:] == sent).all(), (tag, k, "written behind the image")
        return
    for c, p in enumerate(delivered(rows[k], w, h, g.channels, stride)):
        bad = np.flatnonzero(p != planes[c][: w * h])
        assert bad.size == 0, (tag, k, c, f"{bad.size} samples differ, first at {bad[:1]}")


def flip_payload(stream, which):
    """a payload byte of the `which`-th packet flipped: its payload CRC fails, a decoder steps over it byte by byte"""
    s = bytearray(stream)
    off, n = list(red.walk(stream))[which]
    assert n > red.HEADER + 2
    s[off + red.HEADER + (n - red.HEADER) // 2] ^= 0x10
    return bytes(s)


# ------------------------------------------------------------------------------------------------ scenarios
def run_ladder(rig, expected, orc, name, **options):
    """the three nested cuts fed as increments: every step is the oracle's decode of that cut (through the model of the
    decoder's options), and an empty feed delivers the image of the state again"""
    from tests.decoder_batch_cases import oracle_decode
    g, master, cuts, incs = ladder(expected, name)
    ses, mod = rig.open(name, **options)
    plain = not options.get("reduce") and not options.get("reconstruct")
    for i, inc in enumerate(incs):
        got = rig.feed(ses, [inc], display=options.get("display", False))
        want = mod.feed(0, inc)
        if plain:                                           # (the model itself: T is the cut, packet for packet)
            ref = oracle_decode(orc, cuts[i], g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
            assert ref[:3] == want[:3] and all(np.array_equal(a, b) for a, b in zip(ref[3], want[3])), (name, i)
        check_step(g, got, 0, want, (name, "step", i), options.get("display", False))
    again = rig.feed(ses, [b""], display=options.get("display", False))
    check_step(g, again, 0, mod.feed(0, b""), (name, "empty feed"), options.get("display", False))
    assert ses.stats()[2:] == [mod.decoded, mod.dropped], (name, ses.stats(), mod.decoded, mod.dropped)
    return ses, mod


def run_roi_then_quota(rig, expected, name="gray16_A4"):
    """an ROI cut, then the increment to a quota cut: neither holds the other, the session has their union"""
    g, master, cuts, _ = ladder(expected, name)
    m = model_of(g)
    held = rm.roi_stream(m, master, (0, 0, 60, 40), 5, len(master) // 5)[0]
    uh, uw = cm.units(m, held), cm.units(m, cuts[1])
    assert uh - uw and uw - uh
    inc = cm.combine(m, held, cuts[1], cm.DIFFERENCE)[1]
    union = cm.combine(m, held, cuts[1], cm.UNION)[1]
    ses, mod = rig.open(name)
    check_step(g, rig.feed(ses, [held]), 0, mod.feed(0, held), (name, "roi cut"))
    check_step(g, rig.feed(ses, [inc]), 0, mod.feed(0, inc), (name, "roi + increment"))
    assert cm.units(m, mod.stream_of(0)) == cm.units(m, union)
    return ses, mod


def run_slots(rig, expected, name="gray16_A4"):
    """three slots: a feed to two of them in permuted order, the third left alone; a reset of one slot; a feed of another image
    size and a duplicate of held planes"""
    g, master, cuts, incs = ladder(expected, name)
    ses, mod = rig.open(name, n_slots=3)
    got = rig.feed(ses, [incs[0], cuts[1]], slots=[2, 0])
    for k, (slot, data) in enumerate(((2, incs[0]), (0, cuts[1]))):
        check_step(g, got, k, mod.feed(slot, data), (name, "slots", slot))
    got = rig.feed(ses, [incs[1], b""], slots=[2, 1], sizes=[(0, 0), (7, 5)])
    check_step(g, got, 0, mod.feed(2, incs[1]), (name, "slot 2 refined"))
    check_step(g, got, 1, mod.feed(1, b"", 7, 5), (name, "an empty slot"))
    # another image size: refused, the row untouched, the slot as it was
    og, ospec = OTHER_SIZE
    other = expected(og, ospec, ebc.quota(og, "lossless"))[1]
    before = ses.stats()
    got = rig.feed(ses, [other], slots=[2])
    want = mod.feed(2, other)
    assert want == (sm.INVALID_INPUT, g.w, g.h, None)
    check_step(g, got, 0, want, (name, "size mismatch"))
    assert ses.stats() == before
    # a duplicate of held planes is dropped; the image is the same
    got = rig.feed(ses, [incs[1]], slots=[2])
    check_step(g, got, 0, mod.feed(2, incs[1]), (name, "duplicate"))
    assert ses.stats()[2:] == [mod.decoded, mod.dropped] and mod.dropped >= len(list(red.walk(incs[1])))
    # reset of one slot: it starts over (an increment alone holds no top plane of the chains it refines), the others stay
    ses.reset(2)
    mod.reset(2)
    assert ses.planes_held(2, 0, g.stages, 0, 0) == 0 and ses.planes_held(0, 0, g.stages, 0, 0) == mod.planes_held(0, 0, g.stages, 0, 0) > 0
    got = rig.feed(ses, [incs[2], incs[2]], slots=[0, 2])
    check_step(g, got, 0, mod.feed(0, incs[2]), (name, "slot 0 after the reset of slot 2"))
    check_step(g, got, 1, mod.feed(2, incs[2]), (name, "slot 2 after its reset"))
    assert ses.stats()[2:] == [mod.decoded, mod.dropped]
    return ses, mod


def run_damaged_increment(rig, expected, name="gray16_A4"):
    """one packet of the second increment fails its payload CRC: its chain gaps there, its later planes are dropped"""
    g, master, cuts, incs = ladder(expected, name)
    ses, mod = rig.open(name)
    check_step(g, rig.feed(ses, [incs[0]]), 0, mod.feed(0, incs[0]), (name, "held"))
    hurt = flip_payload(incs[1], len(list(red.walk(incs[1]))) // 3)
    check_step(g, rig.feed(ses, [hurt]), 0, mod.feed(0, hurt), (name, "damaged increment"))
    dropped = mod.dropped
    check_step(g, rig.feed(ses, [incs[2]]), 0, mod.feed(0, incs[2]), (name, "behind the gap"))
    assert mod.dropped > dropped, "no later plane of the gapped chain was dropped"
    assert ses.stats()[2:] == [mod.decoded, mod.dropped]
    return ses, mod


def shorten_packet(stream, which, bits=1):
    """the `which`-th packet with its header's data_length cut to `bits`, its payload cut to match and both CRCs recomputed: a
    valid packet whose entropy decode runs out of data -> (stream, (channel, level, subband, segment, lsb) of the packet)"""
    import zlib
    off, n = list(red.walk(stream))[which]
    hdr = bytearray(stream[off: off + red.HEADER])
    payload = stream[off + red.HEADER: off + red.HEADER + (bits + 7) // 8]
    hdr[16:20] = bits.to_bytes(4, "little")
    hdr[20:24] = zlib.crc32(payload).to_bytes(4, "little")
    hdr[24:28] = zlib.crc32(bytes(hdr[:24])).to_bytes(4, "little")
    return stream[:off] + bytes(hdr) + payload + stream[off + n:], (0, hdr[4], hdr[5], hdr[6], hdr[7] & 15)


def failing_plane(expected, orc, name="gray16_A4"):
    """(crafted second increment, key of its failing packet) such that the decoder oracle shows the chain stopping at that
    plane: with the chain's lower planes taken out of held + crafted + third increment the image is the same, and it is not the
    image of the undamaged third cut"""
    from tests.decoder_batch_cases import oracle_decode
    g, master, cuts, incs = ladder(expected, name)
    dec = lambda s: oracle_decode(orc, s, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
    same = lambda a, b: a[:3] == b[:3] and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    clean = dec(cuts[2])
    n = len(list(red.walk(incs[1])))
    for which in range(n // 3, n - 1):
        crafted, key = shorten_packet(incs[1], which)
        below = [(o, m) for o, m in red.walk(incs[2]) if (0, incs[2][o + 4], incs[2][o + 5], incs[2][o + 6]) == key[:4] and (incs[2][o + 7] & 15) < key[4]]
        if not below:
            continue
        without = b"".join(incs[2][o: o + m] for o, m in red.walk(incs[2]) if (o, m) not in below)
        full = dec(cuts[0] + crafted + incs[2])
        if same(full, dec(cuts[0] + crafted + without)) and not same(full, clean):
            return crafted, key
    raise AssertionError("no packet of the increment makes the oracle stop a chain")


def run_failing_plane(rig, expected, orc, name="gray16_A4"):
    """a plane whose entropy decode fails: the chain stops for good, its later planes are dropped, every step is the oracle's
    decode of everything fed so far as one stream"""
    from tests.decoder_batch_cases import oracle_decode
    g, master, cuts, incs = ladder(expected, name)
    crafted, key = failing_plane(expected, orc, name)
    ses, _ = rig.open(name)
    fed = b""
    for i, data in enumerate((cuts[0], crafted, incs[2])):
        fed += data
        want = oracle_decode(orc, fed, g.channels, g.stages, g.filt, g.segments, g.w * g.h, g.bits)
        check_step(g, rig.feed(ses, [data]), 0, want, (name, "failing plane, step", i))
        if i == 0:
            assert 0 < ses.planes_held(0, *key[:4]) <= (9 if g.bits == 16 else 7) - 1 - key[4], "the failing packet's chain holds nothing above it"
    assert ses.planes_held(0, *key[:4]) == -1, "the chain has not stopped"
    assert ses.stats()[1] > 0 and ses.stats()[3] > 0, ses.stats()
    return ses
