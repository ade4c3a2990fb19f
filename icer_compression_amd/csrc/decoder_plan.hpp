// decoder_plan.hpp -- host-side planner of the decoder: from the verified packets of a stream to
// the list of chains the decode kernel runs and the levels the inverse transform undoes.  Pure host C++, shared by
// decoder.hip and the CPU build in tests/emu.
//
// Restates   icer_find_packet_in_bytestream (the walk; the CRCs are checked per candidate, on the device)
//                                                        lib_icer/src/icer_compress.c:569-588
//            the packet table + image size + LL mean     icer_compress.c:443-463, icer_color.c:550-570
//            the subband / segment loops                 icer_compress.c:472-518, icer_color.c:585-634
#pragma once
#include <algorithm>
#include <stdint.h>
#include <utility>
#include <vector>

#include "decoder_core.hpp"
#include "plan.hpp"

namespace icer {

// a position in the stream where a packet header with the preamble and a matching header CRC starts
struct PacketCandidate {
    uint32_t off;           // byte offset of the header in its stream
    uint32_t payload_bytes; // ceil(data_length / 8)
    uint32_t fits;          // the payload lies inside the stream
    uint32_t payload_ok;    // ... and its CRC-32 matches
    uint32_t frame;         // which stream of a batch
    uint32_t crc_acc;       // device: CRC-32 of the payload, XOR-accumulated from the pieces of check_payloads_kernel
    uint8_t hdr[kHeaderBytes];  // copy of the header, so that the host planner never reads the (device-resident) stream
};

// reflected CRC-32 (zlib), byte at a time; `tab` = the usual 256-entry table
inline void build_crc32_table(uint32_t *tab)
{
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
        tab[i] = c;
    }
}
ICER_HD uint32_t crc32_bytes(const uint32_t *tab, const uint8_t *p, uint32_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; i++) c = tab[(c ^ p[i]) & 255u] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
ICER_HD uint32_t load_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// does a header candidate start at `off`?  (preamble + header CRC; icer_compress.c:574-575)
ICER_HD bool header_candidate(const uint32_t *tab, const uint8_t *s, uint32_t len, uint32_t off, PacketCandidate *out)
{
    if (len - off < (uint32_t)kHeaderBytes) return false;           // (the reference reads the header regardless)
    const uint8_t *p = s + off;
    if (p[0] != 0x5Bu || p[1] != 0x60u) return false;
    if (load_le32(p + 24) != crc32_bytes(tab, p, 24)) return false;
    const uint32_t bits = load_le32(p + 16);
    out->off = off;
    out->frame = 0;
    for (int i = 0; i < kHeaderBytes; i++) out->hdr[i] = p[i];
    out->payload_bytes = bits / 8u + ((bits % 8u) ? 1u : 0u);
    out->fits = out->payload_bytes <= len - off - (uint32_t)kHeaderBytes;
    out->payload_ok = 0;
    out->crc_acc = 0;
    return true;
}
// payload check of one candidate (icer_compress.c:576-577)
ICER_HD void check_payload(const uint32_t *tab, const uint8_t *s, PacketCandidate *c)
{
    if (!c->fits) return;
    const uint8_t *p = s + c->off;
    c->payload_ok = load_le32(p + 20) == crc32_bytes(tab, p + kHeaderBytes, c->payload_bytes);
}

// ---- the payload CRC in pieces (device: check_payloads_kernel, 64 threads per candidate).  For the init / final-xor form
// crc(A || B) = crc(A) * x^(8 |B|) + crc(B) in GF(2)[x] / P (zlib's crc32_combine), so the CRC of a payload is the XOR of
// its pieces' CRCs, each multiplied by x^(8 * bytes behind the piece).
ICER_HD uint32_t dec_gf_mulmod(uint32_t a, uint32_t b)         // a(x) * b(x) mod P(x), reflected representation (bit 31 = x^0)
{
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m != 0; m >>= 1) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1u)) == 0) break;
        }
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
ICER_HD uint32_t dec_gf_xpow_bytes(uint32_t nbytes)            // x^(8 * nbytes) mod P by repeated squaring
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;                   // x^0, x^8
    for (; nbytes != 0; nbytes >>= 1) {
        if (nbytes & 1u) p = dec_gf_mulmod(sq, p);
        sq = dec_gf_mulmod(sq, sq);
    }
    return p;
}
// piece `k` of `pieces` of candidate c's payload: its contribution to the payload CRC
ICER_HD uint32_t payload_piece_crc(const uint32_t *tab, const uint8_t *s, const PacketCandidate &c, uint32_t k, uint32_t pieces)
{
    if (!c.fits) return 0;
    const uint32_t n = c.payload_bytes, piece = (((n + pieces - 1u) / pieces) + 15u) & ~15u;
    const uint32_t start = k * piece, end = start + piece < n ? start + piece : n;
    if (start >= end) return 0;
    uint32_t v = crc32_bytes(tab, s + c.off + (uint32_t)kHeaderBytes + start, end - start);
    if (n > end) v = dec_gf_mulmod(dec_gf_xpow_bytes(n - end), v);
    return v;
}

// a side of the image at 1 / 2^r size: ceil(v / 2^r) (r < kMaxStages)
ICER_HD uint64_t reduced_dim(uint64_t v, int r) { return (v + ((uint64_t(1) << r) - 1)) >> r; }

// ------------------------------------------------------------------------------------------ window decode: the rule
// A window decode (include/icer_hip_dec_window.h) delivers a rectangle of the image, and runs only the chains that rectangle
// depends on.  The dependence is written down per line: of a line of n stored samples [nl lows | nh highs] whose restored
// samples [a, b) are wanted, the stored lows [lo0, lo1) and highs [hi0, hi1) are needed.
//   whole      n < 8, or a position table that is not the plain interleave (the odd lines of an 8-bit decoder): all of it
//   filter A   (pairwise: beta = 0 and alpha_-1 = 0) restored high k reads stored high k and the lows k - 1 .. k + 1
//   the rest   restored high k reads restored high k + 1, and alpha_-1 the low k - 2: everything from pair a / 2 - 2 on
// win_geom chains the lines of the levels: the wanted rectangle of a level is the needed LL rectangle of the next finer one.
struct WinAxis { uint32_t n, a, b, lo0, lo1, hi0, hi1, whole; };
struct WinLevel { WinAxis x, y; };
struct WinGeom {
    uint32_t active;                 // the frame is transformed: its chains and passes are restricted to the window
    uint32_t skip;                   // the window holds more samples than the output stride: nothing runs, nothing is written
    uint32_t x0, y0, ww, wh;         // the window clipped to the image the frame runs with
    uint32_t nlev, w;                // levels of the transform; the image width (the row pitch of the working planes)
    WinLevel lv[kMaxStages];         // lv[0]: level 1, the finest
};
ICER_HD WinAxis win_axis(uint32_t n, uint32_t a, uint32_t b, bool pairwise, int bits)
{
    WinAxis r;
    const uint32_t nl = (n + 1u) / 2u, nh = n / 2u;
    r.n = n; r.a = a; r.b = b; r.whole = 0u;
    r.lo0 = r.lo1 = r.hi0 = r.hi1 = 0u;
    if (a >= b) { r.a = r.b = 0u; return r; }
    if (n < 8u || (bits == 8 && (n & 1u))) { r.whole = 1u; r.lo1 = nl; r.hi1 = nh; return r; }
    const uint32_t ka = a >> 1, kb = (b - 1u) >> 1;
    if (pairwise) {
        r.hi1 = kb + 1u < nh ? kb + 1u : nh;
        r.hi0 = ka < r.hi1 ? ka : r.hi1;
        r.lo0 = ka ? ka - 1u : 0u;
        r.lo1 = kb + 2u < nl ? kb + 2u : nl;
    } else {
        r.hi1 = nh;
        r.hi0 = ka < nh ? ka : nh;
        r.lo0 = ka >= 2u ? ka - 2u : 0u;
        r.lo1 = nl;
    }
    return r;
}
// the pairs of a line that its inverse pass restores for the wanted samples: [k0, k1), k = nh standing for the last low of an odd line
ICER_HD void win_pairs(const WinAxis &ax, uint32_t *k0, uint32_t *k1)
{
    if (ax.a >= ax.b) { *k0 = *k1 = 0u; return; }
    if (ax.whole) { *k0 = 0u; *k1 = (ax.n + 1u) / 2u; return; }
    *k0 = ax.a >> 1; *k1 = ((ax.b - 1u) >> 1) + 1u;
}
// `runs`: the frame delivers samples (w x h of them); `transformed`: it reaches the inverse transform and that has levels.
// win = x, y, w, h in pixels of the w x h image; out_stride: samples the caller has room for.
ICER_HD void win_geom(WinGeom *g, uint64_t w, uint64_t h, int stages, bool runs, bool transformed, const uint32_t *win,
                      uint64_t out_stride, bool pairwise, int bits)
{
    const uint64_t iw = runs ? w : 0u, ih = runs ? h : 0u;
    const uint64_t x0 = win[0] < iw ? win[0] : iw, y0 = win[1] < ih ? win[1] : ih;
    const uint64_t ww = win[2] < iw - x0 ? win[2] : iw - x0, wh = win[3] < ih - y0 ? win[3] : ih - y0;
    const bool empty = ww == 0u || wh == 0u;
    g->x0 = (uint32_t)x0; g->y0 = (uint32_t)y0; g->ww = empty ? 0u : (uint32_t)ww; g->wh = empty ? 0u : (uint32_t)wh;
    g->skip = (!empty && ww * wh > out_stride) ? 1u : 0u;
    g->active = (runs && transformed) ? 1u : 0u;
    g->nlev = (uint32_t)stages; g->w = (uint32_t)iw;
    uint32_t xa = g->x0, xb = g->x0 + g->ww, ya = g->y0, yb = g->y0 + g->wh;
    if (g->skip) xa = xb = ya = yb = 0u;
    for (int j = 0; j < kMaxStages; j++) {
        const bool on = g->active && j < stages;
        const uint32_t cw = on ? (uint32_t)((w + ((uint64_t(1) << j) - 1)) >> j) : 0u, ch = on ? (uint32_t)((h + ((uint64_t(1) << j) - 1)) >> j) : 0u;
        g->lv[j].x = win_axis(cw, on ? xa : 0u, on ? xb : 0u, pairwise, bits);
        g->lv[j].y = win_axis(ch, on ? ya : 0u, on ? yb : 0u, pairwise, bits);
        xa = g->lv[j].x.lo0; xb = g->lv[j].x.lo1; ya = g->lv[j].y.lo0; yb = g->lv[j].y.lo1;
    }
}
// is the chain of the segment rectangle (rx, ry, rw, rh) of subband `sb` at level `lv` (1 = finest) kept?
ICER_HD bool win_keeps(const WinGeom &g, int lv, int sb, uint64_t rx, uint64_t ry, uint64_t rw, uint64_t rh)
{
    if (g.skip) return false;
    if (!g.active) return true;
    const WinAxis &ax = g.lv[lv - 1].x, &ay = g.lv[lv - 1].y;
    const uint64_t x0 = (sb & 1) ? ax.hi0 : ax.lo0, x1 = (sb & 1) ? ax.hi1 : ax.lo1;
    const uint64_t y0 = (sb & 2) ? ay.hi0 : ay.lo0, y1 = (sb & 2) ? ay.hi1 : ay.lo1;
    return rx < x1 && rx + rw > x0 && ry < y1 && ry + rh > y0;
}

struct DecodeLevel { uint32_t cw, ch; };        // region of one inverse-transform level (deepest first)

struct DecodePlan {
    int rc = kOk;                               // return code of the reference for this call
    bool transform = false;                     // the run reaches sign-magnitude removal / mean / inverse DWT / clamping
    size_t w = 0, h = 0;
    uint16_t mean[3] = {0, 0, 0};
    std::vector<ChainDesc> chains;
    std::vector<DecodeLevel> levels;            // empty when the deepest LL is thinner than 3 (ICER_TOO_MANY_STAGES, ignored)
    // a window decode (`window` given): the frame's geometry, and the chains the plain call runs (`chains` holds the kept ones)
    WinGeom win = {};
    uint32_t chains_full = 0;
};

// [chan][level][subband][segment][lsb] -> packet offset (kNoPacket: none) and that packet's data_length
struct PacketTable {
    std::vector<uint32_t> off, bits;
    PacketTable() : off((size_t)3 * (kMaxStages + 1) * 4 * (kMaxSegments + 1) * kPlanes, kNoPacket), bits(off.size(), 0u) {}
    static size_t chain_index(int ch, int lv, int sb, int sg) { return (((size_t)ch * (kMaxStages + 1) + lv) * 4 + sb) * (kMaxSegments + 1) + sg; }
    static size_t index(int ch, int lv, int sb, int sg, int lsb) { return chain_index(ch, lv, sb, sg) * kPlanes + lsb; }
    // does a header name an entry?  (level `lv`: already less the decoder's reduce)
    static bool names(int ch, int lv, int sb, int sg, int lsb) { return lv >= 0 && lv <= kMaxStages && sb < 4 && sg <= kMaxSegments && lsb < kPlanes && ch < 3; }
};

// The second half of plan_decode, from the packet table of a w x h image (pl->w, pl->h, pl->mean set) to its chains, levels
// and return code.  A decode session (decoder_session.hpp) calls it with a table of its own, whose held planes read kHeldPlane.
// `keys`: of each chain its PacketTable::chain_index.
inline void plan_chains(DecodePlan *pl, const PacketTable &tab, int channels, int stages, unsigned segments, int planes, size_t bufsize,
                        std::vector<std::pair<int, Rect>> *where = nullptr, std::vector<size_t> *keys = nullptr)
{
    auto slot = [&](int ch, int lv, int sb, int sg, int lsb) { return tab.off[PacketTable::index(ch, lv, sb, sg, lsb)]; };
    if (bufsize < pl->w * pl->h) { pl->rc = kByteQuotaExceeded; return; }
    const size_t w = pl->w, h = pl->h;
    std::vector<Rect> rects;
    for (int lv = 1; lv <= stages && pl->rc == kOk; lv++)
        for (int ch = 0; ch < channels && pl->rc == kOk; ch++)
            for (int sb = (lv == stages ? 0 : 1); sb < 4; sb++) {
                size_t sw, sh, ox, oy;
                switch (sb) {
                case kLL: sw = dim_low(w, lv);  sh = dim_low(h, lv);  ox = 0; oy = 0; break;
                case kHL: sw = dim_high(w, lv); sh = dim_low(h, lv);  ox = dim_low(w, lv); oy = 0; break;
                case kLH: sw = dim_low(w, lv);  sh = dim_high(h, lv); ox = 0; oy = dim_low(h, lv); break;
                default:  sw = dim_high(w, lv); sh = dim_high(h, lv); ox = dim_low(w, lv); oy = dim_low(h, lv); break;
                }
                SegmentGrid g;
                // (unlike the encoder, P1, the decoder stops on a grid error: whatever was decoded before stays, as
                // sign-magnitude words)
                if ((pl->rc = make_grid(&g, sw, sh, segments)) != kOk) break;
                grid_rects(g, &rects);
                for (size_t sg = 0; sg < rects.size() && sg <= (size_t)kMaxSegments; sg++) {
                    if (slot(ch, lv, sb, (int)sg, planes - 1) == kNoPacket) continue;
                    ChainDesc c;
                    c.frame = 0;
                    c.subband = (uint32_t)sb;
                    c.chan = (uint32_t)ch;
                    c.first = (uint32_t)((oy + rects[sg].y) * w + ox + rects[sg].x);
                    c.w = (uint16_t)rects[sg].w; c.h = (uint16_t)rects[sg].h;
                    for (int lsb = 0; lsb < kPlanes; lsb++) c.pkt[lsb] = lsb < planes ? slot(ch, lv, sb, (int)sg, lsb) : kNoPacket;
                    c.fast = (c.w > 0 && c.h > 0) ? 1u : 0u;
                    for (int lsb = planes - 1; lsb >= 0 && c.pkt[lsb] != kNoPacket; lsb--)
                        if (tab.bits[PacketTable::index(ch, lv, sb, (int)sg, lsb)] < kFastPacketBits) c.fast = 0u;
                    pl->chains.push_back(c);
                    if (where) where->push_back({lv, rects[sg]});
                    if (keys) keys->push_back(PacketTable::chain_index(ch, lv, sb, (int)sg));
                }
            }
    if (pl->rc != kOk) return;
    pl->transform = true;
    if (dim_low(w, stages) >= 3 && dim_low(h, stages) >= 3)
        for (int it = 1; it <= stages; it++)
            pl->levels.push_back(DecodeLevel{(uint32_t)dim_low(w, stages - it), (uint32_t)dim_low(h, stages - it)});
}

// does a frame with this plan deliver samples?  (the three codes the reference returns before it decodes anything deliver none)
inline bool plan_delivers(const DecodePlan &pl)
{
    return !(pl.rc == kInvalidInput || pl.rc == kTooManyStages || pl.rc == kByteQuotaExceeded) && pl.w * pl.h > 0;
}

// a packet the walk accepted, its header split: the level less the decoder's reduce, the image size at 1 / 2^reduce
struct WalkedPacket {
    uint32_t off, bits;                         // where the packet starts in its stream; its data_length
    int ch, lv, sb, sg, lsb;
    size_t w, h;
    uint16_t mean;
    bool named() const { return PacketTable::names(ch, lv, sb, sg, lsb); }
    void enter(PacketTable &tab) const { tab.off[PacketTable::index(ch, lv, sb, sg, lsb)] = off; tab.bits[PacketTable::index(ch, lv, sb, sg, lsb)] = bits; }
};

// The decoder's definition of which packets of a stream count, written once (the device's copy: walk_frame, decoder_dplan.hpp).
// `cands`: the candidates of ONE stream, sorted by offset.  The scan accepts a candidate when it starts at or behind the end of
// the previous packet and both CRCs hold; anything else is stepped over byte by byte.  `reduce` = r > 0 (a reduced-resolution
// decoder, include/icer_hip_dec.h): the walk reads the stream as its derived stream -- a valid packet of level <= r moves the
// cursor and nothing else, any other counts as level - r of an image of ceil(w / 2^r) x ceil(h / 2^r).
// visit(const WalkedPacket &) sees every other accepted packet, in stream order, whether or not its fields name a table entry.
template <class Visit>
inline void walk_packets(const std::vector<PacketCandidate> &cands, int channels, int reduce, Visit visit)
{
    uint32_t cursor = 0;
    for (const PacketCandidate &c : cands) {
        if (c.off < cursor || !c.fits || !c.payload_ok) continue;
        const uint8_t *p = c.hdr;
        cursor = c.off + (uint32_t)kHeaderBytes + c.payload_bytes;
        if ((int)p[4] <= reduce && reduce > 0) continue;          // (dropped from the derived stream)
        visit(WalkedPacket{c.off, load_le32(p + 16), channels == 3 ? (p[7] >> 4) : 0, p[4] - reduce, p[5], p[6], p[7] & 15,
                           (size_t)reduced_dim(load_le32(p + 8), reduce), (size_t)reduced_dim(load_le32(p + 12), reduce),
                           (uint16_t)(p[2] | (p[3] << 8))});
    }
}

// The plan of one stream (walk_packets).  w_in / h_in: the caller's values, kept when the stream holds no valid packet; `stages`: of a
// reduced-resolution decoder, its S - r; `where` (window decode): of each chain its level and its rectangle inside its subband.
inline void plan_decode(DecodePlan *pl, const std::vector<PacketCandidate> &cands, int channels,
                        int stages, unsigned segments, int sample_bits, size_t w_in, size_t h_in, size_t bufsize, int reduce = 0,
                        std::vector<std::pair<int, Rect>> *where = nullptr)
{
    const int planes = sample_bits == 8 ? kPlanes8 : kPlanes;
    *pl = DecodePlan();
    pl->w = w_in; pl->h = h_in;
    if (channels != 1 && channels != 3) { pl->rc = kInvalidInput; return; }
    if (stages < 1 || stages > kMaxStages) { pl->rc = kTooManyStages; return; }      // (reference: out-of-bounds table)
    // the last packet of a kind wins; size and mean are those of the last packet walked, named or not
    PacketTable tab;
    walk_packets(cands, channels, reduce, [&](const WalkedPacket &k) {
        if (k.named()) k.enter(tab);
        pl->w = k.w; pl->h = k.h;
        if (k.ch < 3) pl->mean[k.ch] = k.mean;
    });
    plan_chains(pl, tab, channels, stages, segments, planes, bufsize, where);
}

// The plan of a window decode (`window`: x, y, w, h in pixels of the delivered image): the plan of the plain call, less the
// chains the window does not depend on (win_keeps) -- pl->win, pl->chains_full.  A window of more than out_stride samples turns
// rc into ICER_BYTE_QUOTA_EXCEEDED and keeps no chain.  `pairwise`: the decoder's filter has no recurrence along a line (filter A).
inline void plan_decode_window(DecodePlan *pl, const std::vector<PacketCandidate> &cands, int channels, int stages, unsigned segments,
                               int sample_bits, size_t w_in, size_t h_in, size_t bufsize, int reduce, const uint32_t *window,
                               size_t out_stride, bool pairwise)
{
    std::vector<std::pair<int, Rect>> where;
    plan_decode(pl, cands, channels, stages, segments, sample_bits, w_in, h_in, bufsize, reduce, &where);
    const bool runs = plan_delivers(*pl);
    win_geom(&pl->win, pl->w, pl->h, stages, runs, pl->transform && !pl->levels.empty(), window, out_stride, pairwise, sample_bits);
    pl->chains_full = runs ? (uint32_t)pl->chains.size() : 0u;
    std::vector<ChainDesc> kept;
    for (size_t i = 0; i < pl->chains.size(); i++)
        if (win_keeps(pl->win, where[i].first, (int)pl->chains[i].subband, where[i].second.x, where[i].second.y, where[i].second.w, where[i].second.h))
            kept.push_back(pl->chains[i]);
    pl->chains.swap(kept);
    if (pl->win.skip) pl->rc = kByteQuotaExceeded;
}

}  // namespace icer
