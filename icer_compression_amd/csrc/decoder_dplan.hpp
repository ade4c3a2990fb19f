// decoder_dplan.hpp -- the planner of the asynchronous decode (decoder_async.hpp), on the device: the twin of plan_decode
// (decoder_plan.hpp) written as ICER_HD functions, so that g++ runs it against plan_decode (tests/test_decoder_plan_device.py).
//
//   candidates   the whole blob is searched once for packet headers (preamble 0x5B 0x60 + header CRC); two preambles
//                cannot overlap, so a blob of B bytes holds at most ceil(B / 2) of them.  A candidate is a DCandRec
//                (blob offset, payload CRC); whether it lies inside a frame is decided per frame (dplan_summary).
//   walk         per frame, its candidates in offset order with the reference's cursor rule (dplan_accept) fill a
//                packet table [chan][level][subband][segment][lsb] and set w / h / mean.
//   chains       one slot per (level, chan, subband, segment) in plan_decode's order (dplan_chain); the make_grid errors
//                become a slot bound (dplan_finish).
#pragma once
#include <stdint.h>

#include "decoder_core.hpp"
#include "decoder_plan.hpp"
#include "decoder_route.hpp"
#include "plan.hpp"

namespace icer {

struct DCandRec { uint32_t off, crc; };           // blob offset of a header candidate, CRC-32 of its payload (0: does not fit)

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kDroppedSlot = 0xFFFFFFFEu;    // DCand::slot of a valid packet that a reduced-resolution decoder steps over
constexpr uint32_t kNoChain = 0xFFFFFFFFu;        // ChainDesc::frame of an empty chain slot

// the packet table and chain slots of one frame, for one decoder configuration.  reduce = r > 0 (a reduced-resolution
// decoder): stages is the decoder's S - r and the walk reads a frame as its derived stream, as plan_decode does.
struct DPlanGeom {
    uint32_t channels, stages, segments, planes;
    ICER_HD uint32_t slots() const { return channels * (stages + 1u) * 4u * segments * (uint32_t)kPlanes; }
    ICER_HD uint32_t slot(uint32_t ch, uint32_t lv, uint32_t sb, uint32_t sg, uint32_t lsb) const
    {
        return (((ch * (stages + 1u) + lv) * 4u + sb) * segments + sg) * (uint32_t)kPlanes + lsb;
    }
    // chain slot j = ((lv - 1) * channels + ch) * 4 * segments + sb * segments + sg: plan_decode's order
    ICER_HD uint32_t chain_slots() const { return stages * channels * 4u * segments; }
    uint32_t reduce;
};

// ---- segment grid: make_grid / grid_rects of plan.hpp, callable on the device, one rectangle at a time
ICER_HD int dmake_grid(SegmentGrid *g, uint64_t w, uint64_t h, uint32_t segments)
{
    if ((uint64_t)segments > w * h || segments > (uint32_t)kMaxSegments) return kTooManySegments;
    const uint64_t s = segments;
    uint64_t r;
    if (h > (s - 1) * w) r = s;
    else for (r = 1; r < s && (r + 1) * r * w < h * s; r++) {}
    const uint64_t c = s / r, r_t = (c + 1) * r - s;
    uint64_t h_t = ((2 * h * c * r_t + s) / 2) / s;
    if (h_t < r_t) h_t = r_t;
    const uint64_t x_t = w / c, c_t0 = (x_t + 1) * c - w, y_t = h_t / r_t, r_t0 = (y_t + 1) * r_t - h_t;
    uint64_t x_b = 0, c_b0 = 0, y_b = 0, r_b0 = 0;
    if (r_t < r) {
        x_b = w / (c + 1);
        c_b0 = (x_b + 1) * (c + 1) - w;
        y_b = (h - h_t) / (r - r_t);
        r_b0 = (y_b + 1) * (r - r_t) - (h - h_t);
    }
    *g = SegmentGrid{(uint16_t)w, (uint16_t)h, (uint16_t)r, (uint16_t)c, (uint16_t)r_t, (uint16_t)h_t,
                     (uint16_t)x_t, (uint16_t)c_t0, (uint16_t)y_t, (uint16_t)r_t0, (uint16_t)x_b,
                     (uint16_t)c_b0, (uint16_t)y_b, (uint16_t)r_b0, (uint16_t)s};
    return kOk;
}
// rectangle `sg` in coding order (grid_rects: the top region row-major, then the bottom region row-major)
ICER_HD Rect dgrid_rect(const SegmentGrid &g, uint32_t sg)
{
    const uint32_t top = (uint32_t)g.r_t * g.c;
    uint32_t row, col, y0, x, y, sw, sh;
    if (sg < top) {
        row = sg / g.c; col = sg % g.c; y0 = 0;
        sh = g.y_t + (row >= g.r_t0 ? 1u : 0u);
        y = row * g.y_t + (row > g.r_t0 ? row - g.r_t0 : 0u);
        sw = g.x_t + (col >= g.c_t0 ? 1u : 0u);
        x = col * g.x_t + (col > g.c_t0 ? col - g.c_t0 : 0u);
    } else {
        const uint32_t b = sg - top, cols = g.c + 1u;
        row = b / cols; col = b % cols; y0 = g.h_t;
        sh = g.y_b + (row >= g.r_b0 ? 1u : 0u);
        y = row * g.y_b + (row > g.r_b0 ? row - g.r_b0 : 0u);
        sw = g.x_b + (col >= g.c_b0 ? 1u : 0u);
        x = col * g.x_b + (col > g.c_b0 ? col - g.c_b0 : 0u);
    }
    return Rect{x, y0 + y, sw, sh};
}

// subband geometry of plan_decode
ICER_HD void dsubband(uint64_t w, uint64_t h, int lv, int sb, uint64_t *sw, uint64_t *sh, uint64_t *ox, uint64_t *oy)
{
    const uint64_t lw = (w + ((uint64_t(1) << lv) - 1)) >> lv, lh = (h + ((uint64_t(1) << lv) - 1)) >> lv;
    const uint64_t pw = (w + ((uint64_t(1) << (lv - 1)) - 1)) >> (lv - 1), ph = (h + ((uint64_t(1) << (lv - 1)) - 1)) >> (lv - 1);
    switch (sb) {
    case kLL: *sw = lw; *sh = lh; *ox = 0; *oy = 0; break;
    case kHL: *sw = pw / 2; *sh = lh; *ox = lw; *oy = 0; break;
    case kLH: *sw = lw; *sh = ph / 2; *ox = 0; *oy = lh; break;
    default:  *sw = pw / 2; *sh = ph / 2; *ox = lw; *oy = lh; break;
    }
}

// ---- candidates
// a header candidate at blob offset `off` (the header lies inside the blob, preamble and header CRC hold)
ICER_HD bool dheader_at(const uint32_t *crc_tab, const uint8_t *blob, uint32_t blob_len, uint32_t off)
{
    if (blob_len - off < (uint32_t)kHeaderBytes) return false;
    const uint8_t *p = blob + off;
    return p[0] == 0x5Bu && p[1] == 0x60u && load_le32(p + 24) == crc32_bytes(crc_tab, p, 24);
}
// what the walk of frame [frame_off, frame_off + frame_len) needs of one candidate: where it starts and ends in the frame,
// its table slot and fields.  end = 0: not a packet of this frame (header or payload outside it, payload CRC wrong).
// slot = kDroppedSlot: a packet of the frame at a level the decoder leaves out; it moves the cursor and sets nothing.
struct DCand {
    uint32_t rel, end, slot, bits, w, h, mean_ch;   // mean_ch: mean | channel << 16 (channel 3 and up: none)
};
ICER_HD DCand dplan_summary(const DPlanGeom &g, const uint8_t *blob, uint32_t frame_off, uint32_t frame_len, const DCandRec &r)
{
    DCand d;
    d.rel = r.off - frame_off; d.end = 0; d.slot = kNoSlot; d.bits = 0; d.w = 0; d.h = 0; d.mean_ch = 0;
    if (frame_len - d.rel < (uint32_t)kHeaderBytes) return d;
    const uint8_t *p = blob + r.off;
    const uint32_t bits = load_le32(p + 16), pb = bits / 8u + ((bits % 8u) ? 1u : 0u);
    if (pb > frame_len - d.rel - (uint32_t)kHeaderBytes || r.crc != load_le32(p + 20)) return d;   // (icer_compress.c:576-577)
    d.end = d.rel + (uint32_t)kHeaderBytes + pb;
    if ((uint32_t)p[4] <= g.reduce && g.reduce > 0u) { d.slot = kDroppedSlot; return d; }
    const uint32_t lv = p[4] - g.reduce, sb = p[5], sg = p[6], lsb = p[7] & 15u, ch = g.channels == 3 ? (uint32_t)(p[7] >> 4) : 0u;
    if (lv <= g.stages && sb < 4u && sg < g.segments && lsb < (uint32_t)kPlanes && ch < g.channels) d.slot = g.slot(ch, lv, sb, sg, lsb);
    d.bits = bits;
    d.w = (uint32_t)reduced_dim(load_le32(p + 8), (int)g.reduce); d.h = (uint32_t)reduced_dim(load_le32(p + 12), (int)g.reduce);
    d.mean_ch = (uint32_t)(p[2] | (p[3] << 8)) | ((ch < 3u ? ch : 3u) << 16);
    return d;
}

// the walk's state: plan_decode's cursor, w / h (in: the caller's values) and means
struct DWalk {
    uint32_t cursor;
    uint64_t w, h;
    uint16_t mean[3];
};
ICER_HD void dwalk_init(DWalk *s, uint64_t w_in, uint64_t h_in)
{
    s->cursor = 0; s->w = w_in; s->h = h_in; s->mean[0] = s->mean[1] = s->mean[2] = 0;
}
// one candidate of the frame, in offset order: the last packet of a kind wins its table slot (tab_off: offset in the frame,
// tab_bits: its data_length; tab_off starts out kNoPacket)
ICER_HD void dplan_accept(DWalk *s, const DCand &c, uint32_t *tab_off, uint32_t *tab_bits)
{
    if (c.end == 0 || c.rel < s->cursor) return;
    s->cursor = c.end;
    if (c.slot == kDroppedSlot) return;
    if (c.slot != kNoSlot) { tab_off[c.slot] = c.rel; tab_bits[c.slot] = c.bits; }
    s->w = c.w; s->h = c.h;
    if ((c.mean_ch >> 16) < 3u) s->mean[c.mean_ch >> 16] = (uint16_t)(c.mean_ch & 0xFFFFu);
}

// first candidate at or behind blob offset `off` (recs sorted by offset)
ICER_HD uint32_t dlower_bound(const DCandRec *recs, uint32_t n, uint32_t off)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (recs[mid].off < off) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// after the walk: the frame's return code, whether it runs and is transformed, and the first chain slot that a make_grid
// error cuts off (chain slots before it are plan_decode's chains)
struct DPlanResult {
    int rc;
    uint32_t runs, transform, chain_end;
};
ICER_HD DPlanResult dplan_finish(const DPlanGeom &g, const DWalk &s, uint64_t bufsize)
{
    DPlanResult r;
    r.rc = kOk; r.runs = 0; r.transform = 0; r.chain_end = g.chain_slots();
    if (bufsize < s.w * s.h) { r.rc = kByteQuotaExceeded; return r; }
    for (uint32_t lv = 1; lv <= g.stages && r.rc == kOk; lv++)
        for (uint32_t sb = (lv == g.stages ? 0u : 1u); sb < 4u; sb++) {
            uint64_t sw, sh, ox, oy;
            dsubband(s.w, s.h, (int)lv, (int)sb, &sw, &sh, &ox, &oy);
            SegmentGrid grid;
            if ((r.rc = dmake_grid(&grid, sw, sh, g.segments)) != kOk) {
                r.chain_end = (lv - 1u) * g.channels * 4u * g.segments + sb * g.segments;       // (channel 0 of that subband)
                break;
            }
        }
    r.runs = s.w * s.h > 0 ? 1u : 0u;
    r.transform = (r.runs && r.rc == kOk) ? 1u : 0u;
    return r;
}

// chain slot j of a frame: false where plan_decode has no chain; else *c (c->frame = `frame`)
ICER_HD bool dplan_chain(const DPlanGeom &g, const DWalk &s, const DPlanResult &res, const uint32_t *tab_off,
                         const uint32_t *tab_bits, uint32_t j, uint32_t frame, ChainDesc *c)
{
    if (!res.runs || j >= res.chain_end) return false;
    const uint32_t sg = j % g.segments, sb = (j / g.segments) % 4u, lc = j / (g.segments * 4u);
    const uint32_t ch = lc % g.channels, lv = lc / g.channels + 1u;
    if (sb == (uint32_t)kLL && lv != g.stages) return false;
    if (tab_off[g.slot(ch, lv, sb, sg, g.planes - 1u)] == kNoPacket) return false;
    uint64_t sw, sh, ox, oy;
    dsubband(s.w, s.h, (int)lv, (int)sb, &sw, &sh, &ox, &oy);
    SegmentGrid grid;
    if (dmake_grid(&grid, sw, sh, g.segments) != kOk) return false;
    const Rect r = dgrid_rect(grid, sg);
    c->frame = frame;
    c->subband = sb;
    c->chan = ch;
    c->first = (uint32_t)((oy + r.y) * s.w + ox + r.x);
    c->w = (uint16_t)r.w; c->h = (uint16_t)r.h;
    for (uint32_t lsb = 0; lsb < (uint32_t)kPlanes; lsb++) c->pkt[lsb] = lsb < g.planes ? tab_off[g.slot(ch, lv, sb, sg, lsb)] : kNoPacket;
    c->fast = (c->w > 0 && c->h > 0) ? 1u : 0u;
    for (int lsb = (int)g.planes - 1; lsb >= 0 && c->pkt[lsb] != kNoPacket; lsb--)
        if (tab_bits[g.slot(ch, lv, sb, sg, (uint32_t)lsb)] < kFastPacketBits) c->fast = 0u;
    return true;
}

// ---- window decode: is chain slot j of a w x h frame kept by the frame's window?  (win_keeps with the slot's rectangle:
// plan_decode_window's answer, decoder_plan.hpp)
ICER_HD bool dplan_window_keeps(const DPlanGeom &g, const WinGeom &win, uint64_t w, uint64_t h, uint32_t j)
{
    const uint32_t sg = j % g.segments, sb = (j / g.segments) % 4u, lv = j / (g.segments * 4u) / g.channels + 1u;
    uint64_t sw, sh, ox, oy;
    dsubband(w, h, (int)lv, (int)sb, &sw, &sh, &ox, &oy);
    SegmentGrid grid;
    if (dmake_grid(&grid, sw, sh, g.segments) != kOk) return true;
    const Rect r = dgrid_rect(grid, sg);
    return win_keeps(win, (int)lv, (int)sb, r.x, r.y, r.w, r.h);
}

// ---- chain routing: which list a chain goes to, and its place in the list (DRouteRule, takes_planes, dwant_planes: decoder_route.hpp)
// kernels: 0 = wave per plane, 1 + k = lane per plane of ring class k, kRouteThread = thread per chain
constexpr int kRouteClasses = 4, kRouteThread = 1 + kRouteClasses, kRouteKernels = kRouteThread + 1;
constexpr int kRouteBuckets = 33;                  // by chain area, largest first: bucket = clz(w * h)
ICER_HD int droute(const DRouteRule &r, const ChainDesc &c, uint32_t stream_len, bool want_planes)
{
    if (takes_planes(r, c, stream_len, want_planes)) return 0;
    const size_t e = ring_elems_for(c.w, (int)r.nplanes);
    if (r.mode == 0 || e > r.ring_elems_max) return kRouteThread;
    int k = 0;
    while (k + 1 < kRouteClasses && e <= (size_t)(r.ring_elems_max >> (k + 1))) k++;
    return 1 + k;
}
ICER_HD int droute_bucket(const ChainDesc &c)
{
    const uint32_t a = (uint32_t)c.w * c.h;
    int b = 0;
    for (uint32_t m = 0x80000000u; m && !(a & m); m >>= 1) b++;
    return b;
}

// ---- inverse-transform positions: where value v of a line's [lows | highs] lands (the plain interleave; the uint8
// routine's odd lengths through a table, wl_interleave_positions_u8)
struct DPos {
    const uint32_t *tab;
    uint32_t nl;
    ICER_HD uint32_t operator()(uint32_t v) const { return tab ? tab[v] : (v < nl ? 2u * v : 2u * (v - nl) + 1u); }
};

}  // namespace icer
