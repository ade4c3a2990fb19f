// dplan_reduced_emu.cpp -- TEST ONLY.  Both planners of a reduced-resolution decoder (plan_decode with its `reduce`
// argument, decoder_plan.hpp; the device planner with DPlanGeom::reduce, decoder_dplan.hpp) compiled by g++ and driven as
// decoder.hip / decoder_async.hpp drive them, next to each other and next to the DEFINITION: the plain plan_decode (reduce 0,
// stages - reduce) of the frame's derived stream, which the test builds in Python (tests/reduced_model.py).
// tests/test_reduced_plan_device.py holds the three to one another.
#include "../../icer_compression_amd/csrc/decoder_wave.hpp"      // (lane-loop build of the SPMD macros: -DICER_WAVE_EMU)
#include "../../icer_compression_amd/csrc/decoder_planes.hpp"
#include "../../icer_compression_amd/csrc/decoder_core.hpp"
#include "../../icer_compression_amd/csrc/decoder_plan.hpp"
#include "../../icer_compression_amd/csrc/decoder_dplan.hpp"
#include <algorithm>
#include <map>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace icer;

static char g_msg[320];
extern "C" const char *emu_rplan_message(void) { return g_msg; }

namespace {

struct Side {                              // what one planner says about one frame
    std::vector<uint32_t> accepted;        // offsets (in the frame) of the packets whose fields were taken
    int rc = 0;
    uint64_t w = 0, h = 0;
    uint16_t mean[3] = {0, 0, 0};
    bool runs = false, transform = false;
    std::vector<DecodeLevel> levels;
    std::vector<std::vector<uint32_t>> chains;
};

std::vector<uint32_t> chain_key(const ChainDesc &c)
{
    std::vector<uint32_t> k = {c.subband, c.chan, c.first, c.w, c.h, c.fast};
    for (int i = 0; i < kPlanes; i++) k.push_back(c.pkt[i]);
    return k;
}

std::vector<PacketCandidate> candidates(const uint32_t *tab, const uint8_t *frame, uint32_t len)
{
    std::vector<PacketCandidate> mine;
    for (uint32_t o = 0; o < len; o++) {
        PacketCandidate c;
        if (!header_candidate(tab, frame, len, o, &c)) continue;
        check_payload(tab, frame, &c);
        mine.push_back(c);
    }
    return mine;
}

// the synchronous path: plan_decode on the frame's own candidates
Side host_side(const uint32_t *tab, const uint8_t *frame, uint32_t len, int channels, int stages_eff, unsigned segments, int bits,
               uint64_t w_in, uint64_t h_in, uint64_t bufsize, int reduce)
{
    Side s;
    const std::vector<PacketCandidate> mine = candidates(tab, frame, len);
    DecodePlan pl;
    plan_decode(&pl, mine, channels, stages_eff, segments, bits, w_in, h_in, bufsize, reduce);
    uint32_t cursor = 0;
    for (const PacketCandidate &c : mine)                    // (plan_decode's cursor rule; the kept packets)
        if (c.off >= cursor && c.fits && c.payload_ok) {
            cursor = c.off + (uint32_t)kHeaderBytes + c.payload_bytes;
            if ((int)c.hdr[4] > reduce || reduce == 0) s.accepted.push_back(c.off);
        }
    s.rc = pl.rc; s.w = pl.w; s.h = pl.h;
    memcpy(s.mean, pl.mean, sizeof s.mean);
    s.runs = !(pl.rc == kInvalidInput || pl.rc == kTooManyStages || pl.rc == kByteQuotaExceeded) && pl.w * pl.h > 0;
    s.transform = s.runs && pl.transform;
    if (s.transform) s.levels = pl.levels;
    if (s.runs) for (const ChainDesc &c : pl.chains) s.chains.push_back(chain_key(c));
    std::sort(s.chains.begin(), s.chains.end());
    return s;
}

// the asynchronous path: candidates of the whole blob, per-frame validity, the walk, the chain slots
Side device_side(const DPlanGeom &g, const uint8_t *blob, const std::vector<DCandRec> &recs, uint32_t off, uint32_t len, uint64_t w_in,
                 uint64_t h_in, uint64_t bufsize)
{
    Side s;
    std::vector<uint32_t> tab_off(g.slots(), kNoPacket), tab_bits(g.slots(), 0u);
    DWalk wk;
    dwalk_init(&wk, w_in, h_in);
    const uint32_t first = dlower_bound(recs.data(), (uint32_t)recs.size(), off), last = dlower_bound(recs.data(), (uint32_t)recs.size(), off + len);
    for (uint32_t i = first; i < last; i++) {
        const DCand c = dplan_summary(g, blob, off, len, recs[i]);
        const uint32_t before = wk.cursor;
        dplan_accept(&wk, c, tab_off.data(), tab_bits.data());
        if (wk.cursor != before && c.slot != kDroppedSlot) s.accepted.push_back(c.rel);
    }
    const DPlanResult res = dplan_finish(g, wk, bufsize);
    s.rc = res.rc; s.w = wk.w; s.h = wk.h;
    memcpy(s.mean, wk.mean, sizeof s.mean);
    s.runs = res.runs != 0; s.transform = res.transform != 0;
    const int st = (int)g.stages;
    if (s.transform && dim_low(wk.w, st) >= 3 && dim_low(wk.h, st) >= 3)
        for (int it = 1; it <= st; it++) s.levels.push_back(DecodeLevel{(uint32_t)dim_low(wk.w, st - it), (uint32_t)dim_low(wk.h, st - it)});
    for (uint32_t j = 0; j < g.chain_slots(); j++) {
        ChainDesc c;
        if (dplan_chain(g, wk, res, tab_off.data(), tab_bits.data(), j, 0u, &c)) s.chains.push_back(chain_key(c));
    }
    std::sort(s.chains.begin(), s.chains.end());
    return s;
}

// 0 = equal, else which field differs
int differ(const Side &a, const Side &b, bool offsets_too)
{
    if (offsets_too && a.accepted != b.accepted) return 2;
    if (a.accepted.size() != b.accepted.size()) return 2;
    if (a.rc != b.rc) return 3;
    if (a.w != b.w || a.h != b.h) return 4;
    if (memcmp(a.mean, b.mean, sizeof a.mean) != 0) return 5;
    if (a.transform != b.transform) return 6;
    if (a.runs != b.runs) return 7;
    if (a.levels.size() != b.levels.size() ||
        !std::equal(a.levels.begin(), a.levels.end(), b.levels.begin(), [](const DecodeLevel &x, const DecodeLevel &y) { return x.cw == y.cw && x.ch == y.ch; })) return 8;
    if (a.chains != b.chains) return 9;
    return 0;
}

}  // namespace

// n frames of `blob` through both planners of a decoder made with (stages, reduce), and frame k of `dblob` -- the derived
// stream of frame k -- through the plain plan_decode at stages - reduce.  Returns 0 when the three agree on every frame: the
// kept packets (host and device by offset; against the derived stream by count and order, a chain's packet offsets translated
// through that pairing), rc, size, means, transform flag, levels and chains.  Else 10 * comparison (1: device against host, 2:
// host against the derived stream) + the field (emu_rplan_message says where).  out[0] = frames with a kept packet, out[1] =
// frames whose valid packets were all dropped, out[2] = chains.
extern "C" int emu_rplan(const uint8_t *blob, uint32_t blob_len, const uint8_t *dblob, int n, const uint64_t *offsets, const uint64_t *lens,
                         const uint64_t *doffsets, const uint64_t *dlens, int channels, int stages, unsigned segments, int bits,
                         int reduce, uint64_t bufsize, const uint64_t *ws, const uint64_t *hs, uint64_t *out)
{
    uint32_t tab[256];
    build_crc32_table(tab);
    const int st = stages - reduce;
    const DPlanGeom g{(uint32_t)channels, (uint32_t)st, segments, (uint32_t)(bits == 8 ? kPlanes8 : kPlanes), (uint32_t)reduce};
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
    out[0] = out[1] = out[2] = 0;
    for (int k = 0; k < n; k++) {
        const uint32_t off = (uint32_t)offsets[k], len = (uint32_t)lens[k];
        const Side host = host_side(tab, blob + off, len, channels, st, segments, bits, ws[k], hs[k], bufsize, reduce);
        const Side dev = device_side(g, blob, recs, off, len, ws[k], hs[k], bufsize);
        Side def = host_side(tab, dblob + (uint32_t)doffsets[k], (uint32_t)dlens[k], channels, st, segments, bits, ws[k], hs[k], bufsize, 0);
        int bad = differ(dev, host, true);
        if (bad) bad += 10;
        else {
            // the i-th kept packet of the frame is the i-th packet of its derived stream
            if (def.accepted.size() == host.accepted.size()) {
                std::map<uint32_t, uint32_t> to_frame;
                for (size_t i = 0; i < def.accepted.size(); i++) to_frame[def.accepted[i]] = host.accepted[i];
                for (std::vector<uint32_t> &c : def.chains)
                    for (size_t i = c.size() - (size_t)kPlanes; i < c.size(); i++)
                        if (c[i] != kNoPacket) c[i] = to_frame.count(c[i]) ? to_frame[c[i]] : 0xFFFFFFF0u;
                std::sort(def.chains.begin(), def.chains.end());
            }
            bad = differ(host, def, false);
            if (bad) bad += 20;
        }
        if (bad) {
            snprintf(g_msg, sizeof g_msg, "frame %d: check %d (rc %d / %d / %d, %llux%llu / %llux%llu / %llux%llu, kept %zu / %zu / %zu, chains %zu / %zu / %zu; device / host / derived)",
                     k, bad, dev.rc, host.rc, def.rc, (unsigned long long)dev.w, (unsigned long long)dev.h, (unsigned long long)host.w,
                     (unsigned long long)host.h, (unsigned long long)def.w, (unsigned long long)def.h, dev.accepted.size(),
                     host.accepted.size(), def.accepted.size(), dev.chains.size(), host.chains.size(), def.chains.size());
            return bad;
        }
        if (!host.accepted.empty()) out[0]++;
        else if (!candidates(tab, blob + off, len).empty() && host.w == ws[k] && host.h == hs[k]) {
            // (no packet kept: were there valid ones?)
            const Side plain = host_side(tab, blob + off, len, channels, stages, segments, bits, ws[k], hs[k], bufsize, 0);
            if (!plain.accepted.empty()) out[1]++;
        }
        out[2] += host.chains.size();
    }
    return 0;
}
