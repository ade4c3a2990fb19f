// roi_core.hpp -- region-of-interest encode: the byte quota is spent inside a rectangle first (icerx_encode_device_roi).
//
// The feature chooses which packets of a frame's stream are kept, never what a packet holds: every output is a subset of the
// packets of the lossless stream, byte for byte, in the usual final order ("Region of interest";
// tests/roi_model.py is the definition in plain integers).
//
//   A unit is FOREGROUND when it belongs to the LL subband, or when its rectangle, taken in its subband's own coordinates, comes
//   within kRoiGuard coefficients of the frame's rectangle scaled to the unit's level (roi_foreground).  All bit planes of a
//   family share a rectangle, so a family is entirely one or the other.
//   eff(u) = prio(u) << shift for foreground units, prio(u) for the others; the ROI order sorts the units by eff descending,
//   ties by unit index ascending.  rank[u] is u's position in it, order[] the inverse.  A frame whose clipped rectangle is
//   empty has no region of interest: its shift is 0 and its order the priority order (roi_shift), though its LL units still
//   count as foreground.
//   The quota walk (P3, quota_cut_wave) runs over the units in ROI order and gives K; the units with rank < K are kept and
//   copied in the plan's final order.
//
//   roi_*_wave                 the four phases of roi_rank_kernel, one workgroup per frame: classify and count, scan the block
//                              counts, compact the two classes' sort keys, merge by one binary search per unit
//   final_offsets_ranked_wave  final_offsets_wave for a cut that keeps the units with rank[u] < K
//   scan_roi_wave              scan_ladder_wave's twin: one frame at one quota, one wavefront
// Both classes are subsequences of the priority order under a uniform shift, so each is already sorted by (eff descending,
// index ascending): the ROI order is the merge of two sorted lists, and no general sort is needed.
// Written with the SPMD macros of wave.hpp, so that tests/emu/roi_emu.cpp runs the same source on a CPU.
#pragma once
#include "assemble_ladder.hpp"

namespace icer {

constexpr int kRoiWaves = 16;                 // wavefronts of roi_rank_kernel's workgroup
constexpr uint32_t kRoiGuard = 2;             // coefficients around the scaled rectangle that still count as inside
constexpr int kMaxRoiShift = 16;              // ICERX_MAX_ROI_SHIFT
constexpr uint32_t kRoiMaxBlocks = 512;       // blocks of 64 units a frame can have
static_assert((uint32_t)kMaxPackets * kMaxSegments <= 64u * kRoiMaxBlocks, "every plan's units fit the block table of roi_rank_kernel");
constexpr int kRoiIndexBits = 20;             // a sort key = eff << kRoiIndexBits | (2^kRoiIndexBits - 1 - unit index)
constexpr uint64_t kRoiMaxPrio = 1ull << 24;  // no packet priority exceeds it (make_packets: YUV, six stages, LL, plane 8), so a key stays below 2^61

// The sort keys' preconditions, checked where the table is made: the priorities of `p`'s units in unit order; false if one exceeds
// kRoiMaxPrio, if they ever grow with the unit index (a class would not be sorted), or if a unit index does not fit a key.
inline bool roi_priorities(const Plan &p, std::vector<uint64_t> *prio)
{
    prio->clear();
    if (p.units.size() >> kRoiIndexBits) return false;
    for (const UnitDesc &u : p.units) {
        uint64_t pr = ~0ull;
        for (const Packet &pk : p.packets)
            if (pk.chan == u.chan && pk.level == u.level && pk.subband == u.subband && pk.lsb == u.lsb) { pr = pk.priority; break; }
        if (pr > kRoiMaxPrio || (!prio->empty() && pr > prio->back())) return false;
        prio->push_back(pr);
    }
    return true;
}

// A frame's rectangle clipped to the frame: [x0, x1) x [y0, y1); empty when x1 <= x0 or y1 <= y0.
struct RoiBox {
    uint32_t x0, y0, x1, y1;
};
ICER_DEV RoiBox roi_clip(const uint32_t *r, uint32_t w, uint32_t h)
{
    RoiBox b;
    const uint64_t xe = (uint64_t)r[0] + r[2], ye = (uint64_t)r[1] + r[3];
    b.x0 = r[0] < w ? r[0] : w;
    b.y0 = r[1] < h ? r[1] : h;
    b.x1 = xe < w ? (uint32_t)xe : w;
    b.y1 = ye < h ? (uint32_t)ye : h;
    return b;
}

ICER_DEV bool roi_empty(const RoiBox &b) { return b.x1 <= b.x0 || b.y1 <= b.y0; }
// the shift of a frame: the call's, or 0 for a frame without a region of interest
ICER_DEV uint32_t roi_shift(const RoiBox &b, uint32_t shift) { return roi_empty(b) ? 0u : shift; }

// Whether unit `u` of a w x h frame is foreground for `b`.  Nothing goes negative: every term is an unsigned 64-bit sum.
ICER_DEV bool roi_foreground(const UnitDesc &u, uint32_t w, uint32_t h, const RoiBox &b)
{
    if (u.subband == (uint32_t)kLL) return true;
    if (roi_empty(b)) return false;
    const uint32_t l = u.level, round = (1u << l) - 1u;
    // the unit's rectangle less its subband's origin (plan.hpp build_plan)
    const uint64_t sx = u.x0 - ((u.subband == (uint32_t)kHL || u.subband == (uint32_t)kHH) ? (w + round) >> l : 0u);
    const uint64_t sy = u.y0 - ((u.subband == (uint32_t)kLH || u.subband == (uint32_t)kHH) ? (h + round) >> l : 0u);
    const uint64_t x_hi = (((uint64_t)b.x1 + round) >> l) + kRoiGuard, x_lo = b.x0 >> l;
    const uint64_t y_hi = (((uint64_t)b.y1 + round) >> l) + kRoiGuard, y_lo = b.y0 >> l;
    return sx < x_hi && sx + u.w + kRoiGuard > x_lo && sy < y_hi && sy + u.h + kRoiGuard > y_lo;
}

ICER_DEV uint64_t roi_key(uint64_t prio, bool fg, uint32_t shift, uint32_t u)
{
    return ((prio << (fg ? shift : 0u)) << kRoiIndexBits) | (uint64_t)(((1u << kRoiIndexBits) - 1u) - u);
}

// The LDS of roi_rank_kernel: per block of 64 units the foreground units in it (roi_count_wave), then those before it
// (roi_scan_wave); the frame's foreground units.
struct RoiShared {
    uint32_t fg_before[kRoiMaxBlocks];
    uint32_t n_fg;
};

// One frame's units, as every phase takes them.
struct RoiFrame {
    const UnitDesc *units;
    uint32_t n_units, w, h;
    RoiBox box;
};

// Phase 1, wave `wv` of `nwv`: the foreground units of every block of 64.
ICER_DEV void roi_count_wave(RoiShared &s, const RoiFrame &f, uint32_t wv, uint32_t nwv)
{
    DECL_LANE;
    for (uint32_t base = wv * 64u; base < f.n_units; base += nwv * 64u) {
        const uint64_t m = BALLOT(base + (uint32_t)lane < f.n_units && roi_foreground(f.units[base + (uint32_t)lane], f.w, f.h, f.box));
        FOR_LANES
        {
            if (lane == 0) s.fg_before[base >> 6] = (uint32_t)popc64(m);
        }
    }
}

// Phase 2, one wave: counts -> counts before each block; the total.
ICER_DEV void roi_scan_wave(RoiShared &s, uint32_t n_units)
{
    DECL_LANE;
    const uint32_t n_blocks = (n_units + 63u) >> 6;
    uint32_t run = 0;
    for (uint32_t base = 0; base < n_blocks; base += 64u) {
        LANEVAR(uint32_t, c); LANEVAR(uint32_t, before);
        FOR_LANES
        {
            LV(c) = base + (uint32_t)lane < n_blocks ? s.fg_before[base + (uint32_t)lane] : 0u;
        }
        uint32_t total;
        WAVE_EXCL_SCAN(uint32_t, before, c, total);
        FOR_LANES
        {
            if (base + (uint32_t)lane < n_blocks) s.fg_before[base + (uint32_t)lane] = run + LV(before);
        }
        run += total;
    }
    FOR_LANES
    {
        if (lane == 0) s.n_fg = run;
    }
}

// Phases 3 and 4 share the walk: unit u's class, its position among the units of its class, its key.
// Phase 3 (`rank` null): keys[] = the foreground units' keys in unit order, then the background units'.
// Phase 4: rank[u] = u's position in its class + the units of the other class whose key is larger (one binary search in
// that class's sorted keys); order[rank[u]] = u.
ICER_DEV void roi_place_wave(const RoiShared &s, const RoiFrame &f, const uint64_t *prio, uint32_t call_shift, uint64_t *keys, uint32_t *rank,
                             uint32_t *order, uint32_t wv, uint32_t nwv)
{
    DECL_LANE;
    const uint32_t shift = roi_shift(f.box, call_shift);
    const uint32_t n_fg = s.n_fg;
    for (uint32_t base = wv * 64u; base < f.n_units; base += nwv * 64u) {
        const uint64_t valid = BALLOT(base + (uint32_t)lane < f.n_units);
        const uint64_t m = BALLOT(base + (uint32_t)lane < f.n_units && roi_foreground(f.units[base + (uint32_t)lane], f.w, f.h, f.box));
        const uint32_t fg_before = s.fg_before[base >> 6];
        FOR_LANES
        {
            const uint32_t u = base + (uint32_t)lane;
            if (u < f.n_units) {
                const bool fg = (m >> lane) & 1u;
                const uint32_t pos = fg ? fg_before + (uint32_t)mbcnt64(m, lane) : (base - fg_before) + (uint32_t)mbcnt64(valid & ~m, lane);
                const uint64_t key = roi_key(prio[u], fg, shift, u);
                if (!rank) keys[fg ? pos : n_fg + pos] = key;
                else {
                    const uint64_t *other = fg ? keys + n_fg : keys;           // sorted, descending
                    uint32_t lo = 0, hi = fg ? f.n_units - n_fg : n_fg;
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (other[mid] > key) lo = mid + 1u; else hi = mid;
                    }
                    rank[u] = pos + lo;
                    order[pos + lo] = u;
                }
            }
        }
    }
}

// final_offsets_wave for a cut along a rank: unit u is kept iff rank[u] < K.
ICER_DEV int final_offsets_ranked_wave(const uint32_t *bits, const uint32_t *final_order, const uint32_t *rank, uint32_t n_units, uint32_t K,
                                       uint64_t *final_off, uint64_t *size_used)
{
    DECL_LANE;
    uint64_t off = 0;
    for (uint32_t base = 0; base < n_units; base += 64) {
        LANEVAR(uint64_t, sz); LANEVAR(uint64_t, before); LANEVAR(uint32_t, unit); LANEVAR(uint32_t, keep);
        FOR_LANES
        {
            const uint32_t j = base + (uint32_t)lane;
            const uint32_t u = j < n_units ? final_order[j] : 0xFFFFFFFFu;
            LV(unit) = u;
            LV(keep) = u != 0xFFFFFFFFu && rank[u] < K;
            LV(sz) = LV(keep) ? (uint64_t)kHeaderBytes + (((uint64_t)bits[u] + 7u) >> 3) : 0u;
        }
        uint64_t total;
        WAVE_EXCL_SCAN(uint64_t, before, sz, total);
        FOR_LANES
        {
            if (LV(unit) != 0xFFFFFFFFu) final_off[LV(unit)] = LV(keep) ? off + LV(before) : ~0ull;
        }
        off += total;
    }
    *size_used = off;
    return K < n_units ? kByteQuotaExceeded : kOk;
}

// One frame at one quota, cut along the frame's ROI order: final offsets `foff`, *size, *rc as scan_ladder_wave writes them,
// *kept = K (0 for a frame without a stream).  `pbits`: n_units words of scratch of this (frame, quota), the bit counts in ROI
// order.  Returns scan_ladder_wave's flag bits; the unit at which the ranked walk stops is order[K].
ICER_DEV uint32_t scan_roi_wave(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t quota, int skip,
                                const UnitDesc *units, const uint32_t *rank, const uint32_t *order, uint32_t *pbits, uint64_t *foff,
                                unsigned long long *size, int32_t *rc, uint32_t *kept)
{
    DECL_LANE;
    uint32_t flags = 0;
    if (drop_frame_wave(bits, n_units, skip, foff, size, rc, &flags)) {
        FOR_LANES
        {
            if (lane == 0) *kept = 0u;
        }
        return flags;
    }
    FOR_LANES
    {
        for (uint32_t i = (uint32_t)lane; i < n_units; i += 64) pbits[i] = bits[order[i]];
    }
    WAVE_SYNC();
    const uint32_t K = quota_cut_wave(pbits, n_units, quota);
    uint64_t used;
    const int r = final_offsets_ranked_wave(bits, final_order, rank, n_units, K, foff, &used);
    if (K < n_units) {
        const uint32_t stop = order[K];
        if (bits[stop] == kUnitTooBig && units[stop].cap_is_bound) flags |= 1;
    }
    FOR_LANES
    {
        if (lane == 0) { *size = used; *rc = r; *kept = K; }
    }
    return flags;
}

}  // namespace icer
