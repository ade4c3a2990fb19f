// dplan_emu.cpp -- TEST ONLY.  The device planner of the asynchronous decode (decoder_dplan.hpp) compiled by g++ and driven the
// way decoder_async.hpp drives it -- candidates over the whole blob, per-frame validity, the cursor walk, the chain slots --
// next to the host planner of the synchronous decode (per-frame candidates, plan_decode).  tests/test_decoder_plan_device.py
// holds one to the other.
#include "../../icer_compression_amd/csrc/decoder_wave.hpp"      // (lane-loop build of the SPMD macros: -DICER_WAVE_EMU)
#include "../../icer_compression_amd/csrc/decoder_planes.hpp"
#include "../../icer_compression_amd/csrc/decoder_core.hpp"
#include "../../icer_compression_amd/csrc/decoder_plan.hpp"
#include "../../icer_compression_amd/csrc/decoder_dplan.hpp"
#include "../../icer_compression_amd/csrc/wavelet_core.hpp"
#include <algorithm>
#include <stdio.h>
#include <string.h>
#include <tuple>
#include <vector>

using namespace icer;

static char g_msg[256];
extern "C" const char *emu_dplan_message(void) { return g_msg; }

static std::vector<uint32_t> chain_key(const ChainDesc &c)
{
    std::vector<uint32_t> k = {c.frame, c.subband, c.chan, c.first, c.w, c.h, c.fast};
    for (int i = 0; i < kPlanes; i++) k.push_back(c.pkt[i]);
    return k;
}

// n frames of one blob (offsets / lens in bytes; frames inside the blob).  ws / hs: in-values.  Returns 0 when the device
// planner and plan_decode agree on every frame (rc, w, h, means, transform flag, levels, chain multiset, accepted packets);
// else the number of the first check that failed (emu_dplan_message says where).  out[0] = blob candidates, out[1] = frames
// whose walk accepted a packet, out[2] = chains
// that may take the wave-per-plane kernel (ChainDesc::fast).
extern "C" int emu_dplan(const uint8_t *blob, uint32_t blob_len, int n, const uint64_t *offsets, const uint64_t *lens, int channels,
                         int stages, unsigned segments, int bits, uint64_t bufsize, const uint64_t *ws, const uint64_t *hs,
                         uint64_t *out)
{
    uint32_t tab[256];
    build_crc32_table(tab);
    const DPlanGeom g{(uint32_t)channels, (uint32_t)stages, segments, (uint32_t)(bits == 8 ? kPlanes8 : kPlanes)};
    // blob: candidates in offset order, their payload CRCs in 64 pieces (mark / compact / payload_crcs kernels)
    std::vector<DCandRec> recs;
    for (uint32_t off = 0; off < blob_len; off++)
        if (dheader_at(tab, blob, blob_len, off)) recs.push_back(DCandRec{off, 0u});
    for (DCandRec &r : recs) {
        PacketCandidate c;
        c.off = r.off;
        const uint32_t b = load_le32(blob + r.off + 16);
        c.payload_bytes = b / 8u + ((b % 8u) ? 1u : 0u);
        c.fits = c.payload_bytes <= blob_len - r.off - (uint32_t)kHeaderBytes;
        for (uint32_t k = 0; k < 64u; k++) r.crc ^= payload_piece_crc(tab, blob, c, k, 64u);
    }
    out[0] = recs.size();
    out[1] = 0;
    out[2] = 0;
    if (recs.size() > (blob_len + 1u) / 2u) { snprintf(g_msg, sizeof g_msg, "%zu candidates in %u bytes", recs.size(), blob_len); return 1; }
    std::vector<uint32_t> tab_off(g.slots()), tab_bits(g.slots());
    for (int k = 0; k < n; k++) {
        const uint32_t off = (uint32_t)offsets[k], len = (uint32_t)lens[k];
        // the synchronous path: candidates of the frame alone, plan_decode
        std::vector<PacketCandidate> mine;
        for (uint32_t o = 0; o < len; o++) {
            PacketCandidate c;
            if (!header_candidate(tab, blob + off, len, o, &c)) continue;
            check_payload(tab, blob + off, &c);
            mine.push_back(c);
        }
        DecodePlan pl;
        plan_decode(&pl, mine, channels, stages, segments, bits, ws[k], hs[k], bufsize);
        std::vector<uint32_t> acc_sync, acc_dev;
        uint32_t cursor = 0;
        for (const PacketCandidate &c : mine)                // (plan_decode's cursor rule)
            if (c.off >= cursor && c.fits && c.payload_ok) { acc_sync.push_back(c.off); cursor = c.off + (uint32_t)kHeaderBytes + c.payload_bytes; }
        // the device path
        std::fill(tab_off.begin(), tab_off.end(), kNoPacket);
        DWalk s;
        dwalk_init(&s, ws[k], hs[k]);
        const uint32_t first = dlower_bound(recs.data(), (uint32_t)recs.size(), off), last = dlower_bound(recs.data(), (uint32_t)recs.size(), off + len);
        for (uint32_t i = first; i < last; i++) {
            const DCand c = dplan_summary(g, blob, off, len, recs[i]);
            const uint32_t before = s.cursor;
            dplan_accept(&s, c, tab_off.data(), tab_bits.data());
            if (s.cursor != before) acc_dev.push_back(c.rel);
        }
        if (!acc_dev.empty()) out[1]++;
        const DPlanResult res = dplan_finish(g, s, bufsize);
        std::vector<std::vector<uint32_t>> ch_sync, ch_dev;
        const bool runs = !(pl.rc == kInvalidInput || pl.rc == kTooManyStages || pl.rc == kByteQuotaExceeded) && pl.w * pl.h > 0;
        if (runs) for (ChainDesc c : pl.chains) { c.frame = (uint32_t)k; ch_sync.push_back(chain_key(c)); }
        for (uint32_t j = 0; j < g.chain_slots(); j++) {
            ChainDesc c;
            if (dplan_chain(g, s, res, tab_off.data(), tab_bits.data(), j, (uint32_t)k, &c)) { ch_dev.push_back(chain_key(c)); out[2] += c.fast; }
        }
        std::sort(ch_sync.begin(), ch_sync.end());
        std::sort(ch_dev.begin(), ch_dev.end());
        std::vector<DecodeLevel> lv_dev;
        if (res.transform && dim_low(s.w, stages) >= 3 && dim_low(s.h, stages) >= 3)
            for (int it = 1; it <= stages; it++) lv_dev.push_back(DecodeLevel{(uint32_t)dim_low(s.w, stages - it), (uint32_t)dim_low(s.h, stages - it)});
        int bad = 0;
        if (acc_dev != acc_sync) bad = 2;
        else if (res.rc != pl.rc) bad = 3;
        else if (s.w != pl.w || s.h != pl.h) bad = 4;
        else if (memcmp(s.mean, pl.mean, sizeof s.mean) != 0) bad = 5;
        else if ((res.transform != 0) != (runs && pl.transform)) bad = 6;
        else if ((res.runs != 0) != runs) bad = 7;
        else if (lv_dev.size() != pl.levels.size() ||
                 !std::equal(lv_dev.begin(), lv_dev.end(), pl.levels.begin(), [](const DecodeLevel &a, const DecodeLevel &b) { return a.cw == b.cw && a.ch == b.ch; })) bad = 8;
        else if (ch_dev != ch_sync) bad = 9;
        if (bad) {
            snprintf(g_msg, sizeof g_msg, "frame %d: check %d (rc %d / %d, %zux%zu / %llux%llu, %zu / %zu accepted, %zu / %zu chains)", k, bad,
                     res.rc, pl.rc, pl.w, pl.h, (unsigned long long)s.w, (unsigned long long)s.h, acc_dev.size(), acc_sync.size(),
                     ch_dev.size(), ch_sync.size());
            return bad;
        }
    }
    return 0;
}

// dmake_grid / dgrid_rect against make_grid / grid_rects: 0 = equal (rc, fields, every rectangle)
extern "C" int emu_dgrid(uint64_t w, uint64_t h, unsigned segments)
{
    SegmentGrid a, b;
    const int ra = make_grid(&a, w, h, segments), rb = dmake_grid(&b, w, h, segments);
    if (ra != rb) return 1;
    if (ra != kOk) return 0;
    if (memcmp(&a, &b, sizeof a) != 0) return 2;
    std::vector<Rect> rects;
    grid_rects(a, &rects);
    if (rects.size() != segments) return 3;
    for (uint32_t i = 0; i < rects.size(); i++) {
        const Rect r = dgrid_rect(b, i);
        if (r.x != rects[i].x || r.y != rects[i].y || r.w != rects[i].w || r.h != rects[i].h) return 4;
    }
    return 0;
}

// interleave positions as the asynchronous inverse transform takes them (DPos: the plain interleave, or for uint8 odd lengths
// the table of wl_interleave_positions_u8, decoder_async.hpp level_positions_kernel) against interleave_positions
extern "C" int emu_dpos(uint32_t len, int bits)
{
    std::vector<uint32_t> want(len), table(2u * len);
    interleave_positions(len, bits, want.data());
    const bool odd8 = bits == 8 && (len & 1u);
    if (odd8) wl_interleave_positions_u8(len, table.data() + len, table.data());
    const DPos p{odd8 ? table.data() : nullptr, (len + 1u) / 2u};
    for (uint32_t v = 0; v < len; v++)
        if (p(v) != want[v]) return 1;
    return 0;
}
