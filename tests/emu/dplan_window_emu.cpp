// dplan_window_emu.cpp -- TEST ONLY.  Both planners of a window decode -- plan_decode_window (decoder_plan.hpp, the synchronous
// calls) and the device planner with dplan_window_keeps (decoder_dplan.hpp, as window_frames_kernel of decoder_window.hpp drives
// it) -- compiled by g++ and run next to each other on the frames of a blob, each with its own window.
// tests/test_window_plan_device.py holds the two to one another and their counts to tests/window_model.py.
#include "../../icer_compression_amd/csrc/decoder_wave.hpp"      // (lane-loop build of the SPMD macros: -DICER_WAVE_EMU)
#include "../../icer_compression_amd/csrc/decoder_planes.hpp"
#include "../../icer_compression_amd/csrc/decoder_core.hpp"
#include "../../icer_compression_amd/csrc/decoder_plan.hpp"
#include "../../icer_compression_amd/csrc/decoder_dplan.hpp"
#include <algorithm>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace icer;

static char g_msg[320];
extern "C" const char *emu_wplan_message(void) { return g_msg; }

namespace {

std::vector<uint32_t> chain_key(const ChainDesc &c)
{
    std::vector<uint32_t> k = {c.subband, c.chan, c.first, c.w, c.h, c.fast};
    for (int i = 0; i < kPlanes; i++) k.push_back(c.pkt[i]);
    return k;
}

}  // namespace

// n frames of `blob`, frame k with windows[4 k ..]: 0 when the planners agree on every frame's rc, size, clipped window and
// kept chains, else 1 + the frame, and what differs in emu_wplan_message.  out[6 k ..]: rc, ww * wh, chains run, chains of the
// plain call, active, skip of frame k (the host planner's, equal to the device's).
extern "C" int emu_wplan(const uint8_t *blob, uint32_t blob_len, int n, const uint64_t *offsets, const uint64_t *lens, const uint32_t *windows,
                         int channels, int stages, unsigned segments, int bits, int filt, uint64_t full_stride, uint64_t out_stride,
                         int64_t *out)
{
    uint32_t tab[256];
    build_crc32_table(tab);
    const FilterTaps taps = filter_taps(filt);
    const bool pairwise = taps.be == 0 && taps.am1 == 0;
    const DPlanGeom g{(uint32_t)channels, (uint32_t)stages, segments, (uint32_t)(bits == 8 ? kPlanes8 : kPlanes), 0u};
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
    for (int k = 0; k < n; k++) {
        const uint32_t off = (uint32_t)offsets[k], len = (uint32_t)lens[k];
        const uint32_t *win = windows + 4 * (size_t)k;
        // the synchronous path
        std::vector<PacketCandidate> mine;
        for (uint32_t o = 0; o < len; o++) {
            PacketCandidate c;
            if (!header_candidate(tab, blob + off, len, o, &c)) continue;
            check_payload(tab, blob + off, &c);
            mine.push_back(c);
        }
        DecodePlan pl;
        plan_decode_window(&pl, mine, channels, stages, segments, bits, 0, 0, full_stride, 0, win, out_stride, pairwise);
        const bool runs = !(pl.rc == kInvalidInput || pl.rc == kTooManyStages || pl.rc == kByteQuotaExceeded) && pl.w * pl.h > 0;
        std::vector<std::vector<uint32_t>> host;
        if (runs) for (const ChainDesc &c : pl.chains) host.push_back(chain_key(c));
        std::sort(host.begin(), host.end());
        // the asynchronous path: plan_frames_kernel, then window_frames_kernel
        std::vector<uint32_t> tab_off(g.slots(), kNoPacket), tab_bits(g.slots(), 0u);
        DWalk wk;
        dwalk_init(&wk, 0, 0);
        const uint32_t first = dlower_bound(recs.data(), (uint32_t)recs.size(), off), last = dlower_bound(recs.data(), (uint32_t)recs.size(), off + len);
        for (uint32_t i = first; i < last; i++) dplan_accept(&wk, dplan_summary(g, blob, off, len, recs[i]), tab_off.data(), tab_bits.data());
        const DPlanResult res = dplan_finish(g, wk, full_stride);
        const uint32_t fw = res.runs ? (uint32_t)wk.w : 0u, fh = res.runs ? (uint32_t)wk.h : 0u;
        const uint32_t ll_w = (uint32_t)dim_low(wk.w, stages), ll_h = (uint32_t)dim_low(wk.h, stages);
        WinGeom wg;
        win_geom(&wg, fw, fh, stages, fw != 0u && fh != 0u, res.transform && ll_w >= 3u && ll_h >= 3u, win, out_stride, pairwise, bits);
        std::vector<std::vector<uint32_t>> dev;
        uint32_t full = 0;
        for (uint32_t j = 0; j < g.chain_slots(); j++) {
            ChainDesc c;
            if (!dplan_chain(g, wk, res, tab_off.data(), tab_bits.data(), j, 0u, &c)) continue;
            full++;
            if (dplan_window_keeps(g, wg, fw, fh, j)) dev.push_back(chain_key(c));
        }
        std::sort(dev.begin(), dev.end());
        const int dev_rc = wg.skip ? (int)kByteQuotaExceeded : res.rc;
        const char *bad = nullptr;
        if (dev_rc != pl.rc) bad = "rc";
        else if (wk.w != pl.w || wk.h != pl.h) bad = "size";
        else if (memcmp(&wg, &pl.win, sizeof wg) != 0) bad = "geometry";
        else if (full != pl.chains_full) bad = "chains of the plain call";
        else if (dev != host) bad = "kept chains";
        if (bad) {
            snprintf(g_msg, sizeof g_msg, "frame %d: %s (rc %d / %d, kept %zu / %zu, full %u / %u; device / host)", k, bad, dev_rc, pl.rc,
                     dev.size(), host.size(), full, pl.chains_full);
            return 1 + k;
        }
        int64_t *o = out + 6 * (size_t)k;
        o[0] = pl.rc; o[1] = (int64_t)pl.win.ww * pl.win.wh; o[2] = (int64_t)host.size(); o[3] = pl.chains_full; o[4] = pl.win.active; o[5] = pl.win.skip;
    }
    return 0;
}
