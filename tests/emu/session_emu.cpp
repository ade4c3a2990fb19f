// session_emu.cpp -- TEST ONLY.  The resume variants of both chain kernels of a decode session (decoder_planes.hpp
// pw_run_chain_resume's parts: pw_resume_shape, pw_init_resume, pw_load_step in front of pw_step; decoder_core.hpp
// decode_chain_resume) in the CPU lane-loop build, as tests/emu/decoder_emu.cpp mode 4 runs the plain ones.  A stand-alone
// program, so that it can be built with -fsanitize=address,undefined and run on the host:
//     session_emu <case file>
// A case file holds streams and the images the decoder oracle makes of them (tests/test_session_emu.py writes it).  Every chain
// of every stream is decoded in two goes, split at every plane boundary: the top s planes by the plain variant, the rest by the
// resume variant on the same plane -- with the waves of the wave-per-plane kernel stepped round-robin and in seeded random
// orders, and with every chain on the thread-per-chain route; a chain part whose packets are below kFastPacketBits takes the
// thread route as in decoder_session.hpp.  Every image must equal the oracle's (s = 0 and s = all planes are the one-go decodes).
#include "../../icer_compression_amd/csrc/decoder_wave.hpp"      // (lane-loop build of the SPMD macros: -DICER_WAVE_EMU)
#include "../../icer_compression_amd/csrc/decoder_planes.hpp"
#include "../../icer_compression_amd/csrc/decoder_core.hpp"
#include "../../icer_compression_amd/csrc/decoder_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace icer;

// chains resumed behind a loader wave, chains resumed on the thread route, of them because a packet was short, steps a loader
// was refused (its ring slot not recycled yet), lock-ups
static unsigned long long g_stats[5];

static bool part_is_fast(const ChainDesc &c, const uint8_t *stream, uint32_t stream_len, const DecoderTables &t, int planes)
{
    if (!t.lut_ok || stream_len < 4u || c.w == 0 || c.h == 0) return false;
    for (int lsb = planes - 1; lsb >= 0 && c.pkt[lsb] != kNoPacket; lsb--)
        if (c.pkt[lsb] != kHeldPlane && packet_bits(stream, c.pkt[lsb]) < kFastPacketBits) return false;
    return true;
}

// the waves of pw_run_chain_resume in turns: round-robin (seed 0: a full round without progress is a lock-up), or in an order
// drawn from `seed`
static bool run_planes(uint16_t *plane, size_t stride, const ChainDesc &c, const uint8_t *stream, uint32_t stream_len,
                       const DecoderTables &t, int planes, int sign_bit, unsigned seed)
{
    std::vector<uint8_t> lds(pw_lds_bytes(c.w, planes), 0);
    PwShared &sh = *reinterpret_cast<PwShared *>(lds.data());
    uint16_t *zero_row = reinterpret_cast<uint16_t *>(lds.data() + sizeof(PwShared)), *ring = zero_row + pw_ring_pitch(c.w);
    const PwResume s = pw_resume_shape(c, planes);
    if (s.nrun == 0) return true;
    std::vector<PlaneWave> pw(s.nrun);
    for (uint32_t j = 0; j < s.nrun; j++) pw_init_resume(pw[j], j, s, c, planes, sign_bit, plane, stride, stream, stream_len, &t);
    if (s.held) g_stats[0]++;
    unsigned rng = seed * 2654435761u + 12345u;
    for (unsigned long long rounds = 0;; rounds++) {
        bool progress = false, all_done = true;
        for (uint32_t k = 0; k < s.nrun; k++) {
            uint32_t j = k;
            if (seed) { rng = rng * 1664525u + 1013904223u; j = (rng >> 16) % s.nrun; }
            const bool loader = s.held && j == 0u;
            const int st = loader ? pw_load_step(pw[j], sh, ring) : pw_step(pw[j], sh, zero_row, ring);
            if (st == 1) progress = true;
            if (st == 0 && loader) g_stats[3]++;
        }
        for (uint32_t j = 0; j < s.nrun; j++) all_done = all_done && pw[j].r >= pw[j].h;
        if (all_done) return true;
        if ((!progress && !seed) || rounds > (1ull << 24)) { g_stats[4]++; return false; }
    }
}

static void run_part(uint16_t *plane, size_t stride, const ChainDesc &c, const uint8_t *stream, uint32_t stream_len, const DecoderTables &t,
                     int planes, int sign_bit, bool threads, unsigned seed, bool resumed)
{
    const bool fast = part_is_fast(c, stream, stream_len, t, planes);
    if (!threads && fast) { run_planes(plane, stride, c, stream, stream_len, t, planes, sign_bit, seed); return; }
    PlaneDecoder job;
    PlaneStorage own;
    plane_attach_local(job, own);
    uint32_t lowest = 0;
    decode_chain_resume(job, plane, stride, c, (int)c.subband, stream, stream_len, t, planes, sign_bit, &lowest);
    if (resumed) { g_stats[1]++; if (!fast) g_stats[2]++; }
}

// the stream decoded with every chain split after its top `split` planes; planes[c]: w * h words
static int decompress_split(std::vector<std::vector<uint16_t>> &out, int channels, size_t *w, size_t *h, const uint8_t *data, size_t len,
                            int stages, int filt, unsigned segments, int sample_bits, int split, bool threads, unsigned seed)
{
    uint32_t crc_tab[256];
    build_crc32_table(crc_tab);
    std::vector<PacketCandidate> cands;
    for (uint32_t off = 0; off < (uint32_t)len; off++) {
        PacketCandidate c;
        if (header_candidate(crc_tab, data, (uint32_t)len, off, &c)) cands.push_back(c);
    }
    for (PacketCandidate &c : cands) check_payload(crc_tab, data, &c);
    DecodePlan pl;
    plan_decode(&pl, cands, channels, stages, segments, sample_bits, *w, *h, (size_t)1 << 30);
    *w = pl.w; *h = pl.h;
    if (pl.rc == kInvalidInput || pl.rc == kTooManyStages || pl.rc == kByteQuotaExceeded) return pl.rc;
    const size_t W = pl.w, H = pl.h;
    out.assign((size_t)channels, std::vector<uint16_t>(W * H, 0));
    CoderTables ct;
    build_coder_tables(&ct);
    DecoderTables dt;
    build_decoder_tables(&dt, ct);
    const int nplanes = sample_bits == 8 ? kPlanes8 : kPlanes, sign_bit = sample_bits == 8 ? 7 : 15;
    for (const ChainDesc &c : pl.chains) {
        int present = 0;
        while (present < nplanes && c.pkt[nplanes - 1 - present] != kNoPacket) present++;
        const int s = split < present ? split : present;
        uint16_t *plane = out[c.chan].data();
        ChainDesc top = c, rest = c;
        for (int lsb = 0; lsb < nplanes; lsb++) {
            if (lsb < nplanes - s) top.pkt[lsb] = kNoPacket;
            else rest.pkt[lsb] = kHeldPlane;
        }
        if (s > 0) run_part(plane, W, top, data, (uint32_t)len, dt, nplanes, sign_bit, threads, seed, false);
        if (present > s) run_part(plane, W, rest, data, (uint32_t)len, dt, nplanes, sign_bit, threads, seed, s > 0);
    }
    if (!pl.transform) return pl.rc;
    const FilterTaps taps = filter_taps(filt);
    std::vector<int16_t> tmp(W * H);
    std::vector<uint32_t> pos_col, pos_row;
    for (int c = 0; c < channels; c++) {
        int16_t *s = (int16_t *)out[c].data();
        for (size_t i = 0; i < W * H; i++) s[i] = from_sign_magnitude(out[c][i], sign_bit);
        const size_t llw = dim_low(W, stages), llh = dim_low(H, stages);
        for (size_t r = 0; r < llh; r++)
            for (size_t x = 0; x < llw; x++) s[r * W + x] = add_ll_mean(s[r * W + x], pl.mean[c], sample_bits);
        for (const DecodeLevel &lv : pl.levels) {
            pos_col.resize(lv.ch); pos_row.resize(lv.cw);
            interleave_positions(lv.ch, sample_bits, pos_col.data());
            interleave_positions(lv.cw, sample_bits, pos_row.data());
            for (uint32_t x = 0; x < lv.cw; x++) idwt_line(s + x, tmp.data() + x, lv.ch, W, taps, sample_bits, pos_col.data());
            for (uint32_t r = 0; r < lv.ch; r++) idwt_line(tmp.data() + (size_t)r * W, s + (size_t)r * W, lv.cw, 1, taps, sample_bits, pos_row.data());
        }
        for (size_t i = 0; i < W * H; i++) {
            if (s[i] < 0) s[i] = 0;
            if (sample_bits == 8) out[c][i] &= 0xFFu;
        }
    }
    return pl.rc;
}

// case file: per case 9 uint32 (w, h, channels, stages, filter, segments, sample bits, stream bytes, the oracle's rc as int32), the
// stream, then channels * w * h uint16 of the oracle's image
int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: session_emu <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    unsigned long long cases = 0, runs = 0;
    uint32_t hd[9];
    while (fread(hd, sizeof hd, 1, f) == 1) {
        const uint32_t w = hd[0], h = hd[1], channels = hd[2], stages = hd[3], filt = hd[4], segments = hd[5], bits = hd[6], len = hd[7];
        const int want_rc = (int)hd[8];
        std::vector<uint8_t> stream(len ? len : 1);
        std::vector<uint16_t> want((size_t)channels * w * h);
        if ((len && fread(stream.data(), 1, len, f) != len) || (want.size() && fread(want.data(), 2, want.size(), f) != want.size())) {
            fprintf(stderr, "case %llu: the file ends early\n", cases);
            return 2;
        }
        const int nplanes = bits == 8 ? kPlanes8 : kPlanes;
        for (int split = 0; split <= nplanes; split++)
            for (int sched = 0; sched < 4; sched++) {              // round-robin, two random orders, the thread route
                std::vector<std::vector<uint16_t>> got;
                size_t gw = 0, gh = 0;
                const unsigned long long locked = g_stats[4];
                const int rc = decompress_split(got, (int)channels, &gw, &gh, stream.data(), len, (int)stages, (int)filt, segments, (int)bits,
                                                split, sched == 3, sched == 3 ? 0u : (unsigned)sched * 7919u);
                runs++;
                bool same = rc == want_rc && gw == w && gh == h && g_stats[4] == locked;
                for (uint32_t c = 0; same && c < channels; c++)
                    same = memcmp(got[c].data(), want.data() + (size_t)c * w * h, sizeof(uint16_t) * w * h) == 0;
                if (!same) {
                    fprintf(stderr, "case %llu (%u x %u, filter %u, %u bit): split %d schedule %d differs from the oracle (rc %d, want %d; lock-ups %llu)\n",
                            cases, w, h, filt, bits, split, sched, rc, want_rc, g_stats[4] - locked);
                    return 1;
                }
            }
        cases++;
    }
    fclose(f);
    printf("cases %llu runs %llu loader_chains %llu thread_resumes %llu short_packet_resumes %llu loader_waits %llu\n", cases, runs, g_stats[0],
           g_stats[1], g_stats[2], g_stats[3]);
    return 0;
}
