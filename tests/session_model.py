"""The definition of a decode session (include/icer_hip_dec_session.h; csrc/decoder_session.hpp) in plain Python over the
decoder oracle, in the manner of reduced_model.py and recon_model.py.

A slot keeps a set T of accepted packets keyed by (channel, level, subband, segment, lsb) -- level as the header names it --,
the image size and the LL means.  A feed is walked on its own as a decoder walks a stream (reduced_model.walk); for a reduced
decoder packets of level <= r move the cursor and nothing else; a packet that names no entry of the decoder's table is dropped;
the last packet of a kind wins.  Size and means are those of the packets in T (a feed of which nothing is accepted teaches the
slot nothing).  A feed with a packet of another size than the slot's (not yet known: than the feed's first packet), or of another
LL mean than the slot's for that channel, is refused: INVALID_INPUT, slot untouched, nothing delivered; an image of more than
frame_stride samples likewise, with QUOTA.  Per chain the feed contributes the planes next, next - 1, ...
for as long as it has them, next being one below the chain's lowest held plane (the top plane for a chain that holds none);
everything else is dropped and counted.  stats()[2] is "planes decoded": of the accepted planes those whose chain the plan of
the slot's image runs (`planned`) -- all of them, unless a subband's segment grid fails (quirk P1), where the plan stops and the
chains at and behind the stop are held but never run.  What the session delivers is the plain decode of the packets of T as one
stream (the oracle; reduced_model / recon_model for a reduced decoder and for a reconstruction setting).

Not modelled: a chain that stops for good at a plane whose entropy decode fails (the oracle does not say which plane of which
chain failed); the tests feed no such packet."""
from tests import recon_model as rcm
from tests import reduced_model as red
from tests import target_model as tm

OK, QUOTA, INVALID_INPUT = 0, -5, -11
MAX_STAGES, MAX_SEGMENTS, MAX_PLANES = 6, 32, 9


class Slot:
    def __init__(self):
        self.T, self.size, self.mean, self.low = {}, None, {}, {}             # low: per chain the lowest plane in T


class SessionModel:
    def __init__(self, orc, channels, stages, filt, segments, frame_stride, bits=16, reduce=0, reconstruct=0, n_slots=1):
        self.orc, self.channels, self.stages, self.filt, self.segments = orc, channels, stages, filt, segments
        self.frame_stride, self.bits, self.r, self.k = frame_stride, bits, reduce, reconstruct
        self.planes = 9 if bits == 16 else 7
        self.slots = [Slot() for _ in range(n_slots)]
        # planes decoded, packets dropped: stats()[2], stats()[3]; runs: (feed, chain) pairs that brought a chain new planes to decode
        self.decoded = self.dropped = self.runs = 0

    def reset(self, slot=-1):
        for k in range(len(self.slots)) if slot < 0 else [slot]:
            self.slots[k] = Slot()

    def lowest(self, slot, chain):
        """the lowest plane the chain (channel, level, subband, segment) holds; self.planes: none"""
        return self.slots[slot].low.get(chain, self.planes)

    def planes_held(self, slot, ch, lv, sb, sg):
        return self.planes - self.lowest(slot, (ch, lv, sb, sg))

    def planned(self, key, w, h):
        """does the plan of a w x h image (csrc/decoder_plan.hpp plan_chains) run the chain of packet `key`?  The plan visits
        level 1 .. stages - r, in it the channels, in them LL (deepest level only), HL, LH, HH, and stops for good at the first
        subband whose segment grid fails (quirk P1: rc -3, what was decoded before stays).  A packet of a chain at or behind
        the stop, or of a chain the plan does not have, is accepted and held like any other -- planes_held counts it -- but
        is never decoded and never shows in an image."""
        ch, lv, sb, sg = key[0], key[1] - self.r, key[2], key[3]
        S = self.stages - self.r
        if not (1 <= lv <= S and ch < self.channels and sg < self.segments and (sb > 0 or lv == S)):
            return False
        for l in range(1, lv + 1):
            for c in range(self.channels):
                for s in range(0 if l == S else 1, 4):
                    if tm.grid_fails(*tm.subband_rect(w, h, l, s)[:2], self.segments):
                        return False
                    if (l, c, s) == (lv, ch, sb):
                        return True
        return False

    def stream_of(self, slot):
        """the packets of T as one stream (a decoder does not mind their order)"""
        T = self.slots[slot].T
        return b"".join(T[key] for key in sorted(T))

    def decode(self, slot, w0=0, h0=0):
        """(rc, w, h, flat planes) of the plain decode of the slot's packets"""
        args = (self.channels, self.stages, self.filt, self.segments, self.frame_stride, self.bits, w0, h0)
        if self.k:
            return rcm.expected_reduced(self.orc, self.stream_of(slot), self.k, self.r, *args)
        return red.expected(self.orc, self.stream_of(slot), self.r, *args)

    def feed(self, slot, data, w0=0, h0=0):
        """-> (rc, w, h, flat planes); planes None: the feed was refused and nothing is delivered"""
        data = bytes(data)
        sl = self.slots[slot]
        size, mean, table, walked = sl.size, dict(sl.mean), {}, 0
        for off, n in red.walk(data):
            hdr = data[off: off + red.HEADER]
            if self.r > 0 and hdr[4] <= self.r:
                continue
            walked += 1
            ch, lv, sb, sg, lsb = (hdr[7] >> 4 if self.channels == 3 else 0), hdr[4], hdr[5], hdr[6], hdr[7] & 15
            if not (lv - self.r <= MAX_STAGES and sb < 4 and sg <= MAX_SEGMENTS and lsb < MAX_PLANES and ch < 3):
                continue
            wh = red.reduced_size(int.from_bytes(hdr[8:12], "little"), int.from_bytes(hdr[12:16], "little"), self.r)
            m = int.from_bytes(hdr[2:4], "little")
            size = wh if size is None else size
            if wh != size or mean.setdefault(ch, m) != m:
                return (INVALID_INPUT,) + (sl.size if sl.size is not None else (w0, h0)) + (None,)
            table[(ch, lv, sb, sg, lsb)] = data[off: off + n]
        took = {}
        for chain in sorted({key[:4] for key in table}):
            nxt = self.lowest(slot, chain) - 1
            while nxt >= 0 and chain + (nxt,) in table:
                took[chain + (nxt,)] = table[chain + (nxt,)]
                nxt -= 1
        # size and means are those of the packets the slot holds: a feed of which nothing is accepted teaches it nothing
        w, h = size if (sl.size is not None or took) else (w0, h0)
        if w * h > self.frame_stride:
            return QUOTA, w, h, None
        if took:
            sl.size = size
            sl.mean.update({ch: mean[ch] for ch in {key[0] for key in took}})
        sl.T.update(took)
        for key in took:
            sl.low[key[:4]] = min(sl.low.get(key[:4], self.planes), key[4])
        # an accepted packet is not dropped; it counts as decoded where the plan runs its chain (`planned`)
        ran = [key for key in took if self.planned(key, w, h)]
        self.decoded += len(ran)
        self.runs += len({key[:4] for key in ran})
        self.dropped += walked - len(took)
        return self.decode(slot, w0, h0)
