// session_wave_emu.cpp -- TEST ONLY.  The resumable lane-per-plane chain decoder of a decode session (decoder_wave.hpp
// decode_chain_wave_resume) in the CPU lane-loop build, beside the plain one (decode_chain_wave) as tests/emu/session_emu.cpp runs
// the resume variants of the other two chain kernels.  A stand-alone program, so that it can be built with
// -fsanitize=address,undefined and run on the host:
//     session_wave_emu <case file>
// A case file holds streams and the images the decoder oracle makes of them (tests/test_session_wave_emu.py writes it).  Every
// chain of every stream is decoded in two goes, split at every plane boundary: the top s planes by decode_chain_wave, the rest by
// decode_chain_wave_resume in place on the same plane, its ring and per-lane state in heap blocks of exactly the size the kernel
// reserves.  s = 0 is the resume function on an empty plane: it must do what the plain one does -- the two are instantiations of one
// body, and the program runs decode_chain_wave on a copy of the plane and requires the same words and the same schedule counts
// (iterations, samples, roll-backs, rows not retired).  Per resumed chain the program checks
//   - *lowest_ok against decode_chain_resume (decoder_core.hpp) run on a copy of the plane as it was before;
//   - that no bit of a held plane, and no sign of a sample those planes made significant, has changed;
//   - for the packet a case names as failing: that lowest_ok is the plane above it.  (A chain whose failing plane lies in the top
//     part has stopped: the session would not resume it, nor does the program.)
// and per case and split that the image equals the oracle's.
#include "../../icer_compression_amd/csrc/decoder_wave.hpp"      // (lane-loop build of the SPMD macros: -DICER_WAVE_EMU)
#include "../../icer_compression_amd/csrc/decoder_core.hpp"
#include "../../icer_compression_amd/csrc/decoder_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace icer;

// decode_chain_wave_resume's own counts ([2] roll-backs, [3] chains that ended with rows not retired, [4] rows reloaded from the state
// plane), and the program's: calls with held planes, calls with none, chains that reported a stop, of them below a held plane,
// roll-backs below a held plane, calls with no plane held that were repeated by decode_chain_wave and compared
static unsigned long long g_wave[5], g_resumes, g_fresh, g_stops, g_stops_below_held, g_rollbacks_below_held, g_plain_checked;

static bool fail(const char *what, const ChainDesc &c, int held)
{
    fprintf(stderr, "chain %u x %u (subband %u, first %u), %d planes held: %s\n", c.w, c.h, c.subband, c.first, held, what);
    return false;
}

// the planes of `c` that have packets, on top of the `held` planes marked in it; fail_off: the packet that fails (kNoPacket: none)
static bool run_resume(uint16_t *plane, size_t stride, size_t words, const ChainDesc &c, const uint8_t *stream, uint32_t stream_len,
                       const DecoderTables &t, int planes, int sign_bit, uint32_t fail_off)
{
    int held = 0;
    while (held < planes && c.pkt[planes - 1 - held] == kHeldPlane) held++;
    const std::vector<uint16_t> before(plane, plane + words);
    std::vector<uint16_t> copy(before);
    PlaneDecoder job;
    PlaneStorage own;
    plane_attach_local(job, own);
    uint32_t want_ok = 0, ok = 0xFFFFFFFFu;
    const unsigned long long rollbacks = g_wave[2], wave_before[4] = {g_wave[0], g_wave[1], g_wave[2], g_wave[3]};
    decode_chain_resume(job, copy.data(), stride, c, (int)c.subband, stream, stream_len, t, planes, sign_bit, &want_ok);
    std::vector<uint16_t> ring(ring_elems_for(c.w, planes), (uint16_t)0xA5A5u);       // (the function fills its ring itself)
    std::vector<uint8_t> state(kStateBytes, 0);
    decode_chain_wave_resume(ring.data(), plane, stride, c, (int)c.subband, stream, stream_len, t, planes, sign_bit, g_wave, state.data(), &ok);
    (held ? g_resumes : g_fresh)++;
    if (held) g_rollbacks_below_held += g_wave[2] - rollbacks;
    if (ok != want_ok) return fail("lowest_ok differs from decode_chain_resume's", c, held);
    if (memcmp(plane, copy.data(), sizeof(uint16_t) * words) != 0) return fail("the plane differs from decode_chain_resume's", c, held);
    if (held == 0) {
        // nothing held: the two instantiations of the one body are one schedule -- the same words, iteration for iteration
        std::vector<uint16_t> plain(before), plain_ring(ring_elems_for(c.w, planes), (uint16_t)0xA5A5u);
        std::vector<uint8_t> plain_state(kStateBytes, 0);
        unsigned long long plain_stats[5] = {0, 0, 0, 0, 0};
        decode_chain_wave(plain_ring.data(), plain.data(), stride, c, (int)c.subband, stream, stream_len, t, planes, sign_bit, plain_stats,
                          plain_state.data());
        if (memcmp(plane, plain.data(), sizeof(uint16_t) * words) != 0) return fail("the plane differs from decode_chain_wave's", c, held);
        for (int k = 0; k < 4; k++)
            if (g_wave[k] - wave_before[k] != plain_stats[k]) return fail("the schedule's counts differ from decode_chain_wave's", c, held);
        if (plain_stats[4] != 0) return fail("decode_chain_wave counted a reload", c, held);
        g_plain_checked++;
    }
    const uint32_t held_mask = ((1u << sign_bit) - 1u) & ~((1u << (planes - held)) - 1u), sign = 1u << sign_bit;
    for (size_t i = 0; held && i < words; i++) {
        const uint32_t a = before[i], b = plane[i];
        if ((a & held_mask) != (b & held_mask) || ((a & held_mask) && (a & sign) != (b & sign))) return fail("a held bit changed", c, held);
    }
    int lowest_fresh = planes - held;
    while (lowest_fresh > 0 && c.pkt[lowest_fresh - 1] < kHeldPlane) lowest_fresh--;
    if ((int)ok > lowest_fresh) { g_stops++; if (held) g_stops_below_held++; }
    for (int lsb = lowest_fresh; lsb < planes - held; lsb++)
        if (c.pkt[lsb] == fail_off && (int)ok != lsb + 1) return fail("lowest_ok does not name the plane above the failing packet", c, held);
    return true;
}

// the stream decoded with every chain split after its top `split` planes; planes[c]: w * h words.  -> false: a check failed
static bool decompress_split(std::vector<std::vector<uint16_t>> &out, int *rc, int channels, size_t *w, size_t *h, const uint8_t *data, size_t len,
                             int stages, int filt, unsigned segments, int sample_bits, int split, uint32_t fail_off)
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
    *w = pl.w; *h = pl.h; *rc = pl.rc;
    if (pl.rc == kInvalidInput || pl.rc == kTooManyStages || pl.rc == kByteQuotaExceeded) return true;
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
        bool stopped = false;                                   // the failing packet is in the top part
        for (int lsb = 0; lsb < nplanes; lsb++) {
            if (lsb < nplanes - s) top.pkt[lsb] = kNoPacket;
            else { rest.pkt[lsb] = kHeldPlane; stopped = stopped || c.pkt[lsb] == fail_off; }
        }
        if (s > 0) {
            std::vector<uint16_t> ring(ring_elems_for(c.w, nplanes), (uint16_t)0xA5A5u);
            std::vector<uint8_t> state(kStateBytes, 0);
            decode_chain_wave(ring.data(), plane, W, top, (int)c.subband, data, (uint32_t)len, dt, nplanes, sign_bit, nullptr, state.data());
        }
        if (present > s && !stopped && !run_resume(plane, W, W * H, rest, data, (uint32_t)len, dt, nplanes, sign_bit, fail_off)) return false;
    }
    if (!pl.transform) return true;
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
    return true;
}

// case file: per case 10 uint32 (w, h, channels, stages, filter, segments, sample bits, stream bytes, the oracle's rc as int32, the
// offset of the packet that fails or 0xFFFFFFFF), the stream, then channels * w * h uint16 of the oracle's image
int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: session_wave_emu <case file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    unsigned long long cases = 0, runs = 0;
    uint32_t hd[10];
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
        for (int split = 0; split <= nplanes; split++) {
            std::vector<std::vector<uint16_t>> got;
            size_t gw = 0, gh = 0;
            int rc = 0;
            const unsigned long long unretired = g_wave[3];
            bool same = decompress_split(got, &rc, (int)channels, &gw, &gh, stream.data(), len, (int)stages, (int)filt, segments, (int)bits, split, hd[9]);
            runs++;
            same = same && rc == want_rc && gw == w && gh == h && g_wave[3] == unretired;
            for (uint32_t c = 0; same && c < channels; c++)
                same = memcmp(got[c].data(), want.data() + (size_t)c * w * h, sizeof(uint16_t) * w * h) == 0;
            if (!same) {
                fprintf(stderr, "case %llu (%u x %u, filter %u, %u bit): split %d differs from the oracle (rc %d, want %d; chains with rows not retired %llu)\n",
                        cases, w, h, filt, bits, split, rc, want_rc, g_wave[3] - unretired);
                return 1;
            }
        }
        cases++;
    }
    fclose(f);
    printf("cases %llu runs %llu resumes %llu fresh_runs %llu reloaded_rows %llu rollbacks %llu rollbacks_below_held %llu stops %llu stops_below_held %llu "
           "plain_checked %llu\n",
           cases, runs, g_resumes, g_fresh, g_wave[4], g_wave[2], g_rollbacks_below_held, g_stops, g_stops_below_held, g_plain_checked);
    return 0;
}
