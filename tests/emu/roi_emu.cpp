// TESTS ONLY: the region-of-interest kernels (csrc/roi_core.hpp) as a CPU lane-loop build (-DICER_WAVE_EMU, see csrc/wave.hpp):
// roi_rank_kernel phase by phase over its wavefronts, in launch order or in a seeded random order, and scan_roi_kernel's wave,
// over the planner's own units (csrc/plan.hpp), for tests/test_emu_roi.py.  With -DROI_EMU_MAIN it is a stand-alone program that
// checks the same against a plain sort (the build that runs under the host sanitizers).  Not part of the product library.
#define ICER_WAVE_EMU 1
#include "../../icer_compression_amd/csrc/roi_core.hpp"
#include <algorithm>
#include <random>
#include <vector>

using namespace icer;

unsigned long long g_emu_chunks[4] = {0, 0, 0, 0};       // (coder_core.hpp's path counters: unused here, defined by every emu build)

static Plan g_plan;
static std::vector<uint64_t> g_prio;

// Plans a geometry; returns its units, or a negative number: the planner's refusal, or -100 when roi_priorities refuses.
extern "C" int emu_roi_plan(uint32_t w, uint32_t h, int channels, int stages, int segments, int sample_bits)
{
    if (int rc = build_plan(&g_plan, w, h, channels, stages, segments, sample_bits)) return rc;
    if (!roi_priorities(g_plan, &g_prio)) return -100;
    return (int)g_plan.units.size();
}

// The plan's tables: final_order, prio, and per unit level, subband, x0, y0, w, h (six words).
extern "C" void emu_roi_tables(uint32_t *final_order, uint64_t *prio, uint32_t *desc)
{
    for (size_t u = 0; u < g_plan.units.size(); u++) {
        const UnitDesc &d = g_plan.units[u];
        final_order[u] = g_plan.final_order[u];
        prio[u] = g_prio[u];
        const uint32_t row[6] = {d.level, d.subband, d.x0, d.y0, d.w, d.h};
        std::copy(row, row + 6, desc + 6 * u);
    }
}

// roi_rank_kernel for one frame.  seed 0: the waves of every phase in launch order; otherwise in a random order per phase.
extern "C" void emu_roi_rank(const uint32_t *roi, uint32_t shift, uint32_t seed, uint32_t *rank, uint32_t *order, uint32_t *foreground)
{
    const uint32_t n_units = (uint32_t)g_plan.units.size();
    RoiShared s;
    const RoiFrame f{g_plan.units.data(), n_units, (uint32_t)g_plan.w, (uint32_t)g_plan.h, roi_clip(roi, (uint32_t)g_plan.w, (uint32_t)g_plan.h)};
    std::vector<uint64_t> keys(n_units);
    std::vector<uint32_t> waves(kRoiWaves);
    for (uint32_t i = 0; i < waves.size(); i++) waves[i] = i;
    std::mt19937 rng(seed);
    auto shuffle = [&] { if (seed) std::shuffle(waves.begin(), waves.end(), rng); };
    shuffle();
    for (uint32_t wv : waves) roi_count_wave(s, f, wv, (uint32_t)kRoiWaves);
    roi_scan_wave(s, n_units);
    shuffle();
    for (uint32_t wv : waves) roi_place_wave(s, f, g_prio.data(), shift, keys.data(), nullptr, nullptr, wv, (uint32_t)kRoiWaves);
    shuffle();
    for (uint32_t wv : waves) roi_place_wave(s, f, g_prio.data(), shift, keys.data(), rank, order, wv, (uint32_t)kRoiWaves);
    *foreground = s.n_fg;
}

// scan_roi_kernel for one frame: one scan_roi_wave per quota, final offsets of quota q at foff[q * n_units], sizes / rcs / kept at
// [q]; `cap_is_bound` per unit stands for the slot table.  Returns the OR of the slot-bound flag bits.
extern "C" uint32_t emu_scan_roi(const uint32_t *bits, const uint64_t *quotas, uint32_t n_q, int skip, const uint8_t *cap_is_bound,
                                 const uint32_t *rank, const uint32_t *order, uint64_t *foff, unsigned long long *sizes, int32_t *rcs,
                                 uint32_t *kept)
{
    const uint32_t n_units = (uint32_t)g_plan.units.size();
    std::vector<UnitDesc> units(g_plan.units);
    for (uint32_t u = 0; u < n_units; u++) units[u].cap_is_bound = cap_is_bound[u];
    std::vector<uint32_t> pbits(n_units);
    uint32_t flags = 0;
    for (uint32_t q = 0; q < n_q; q++)
        flags |= scan_roi_wave(bits, g_plan.final_order.data(), n_units, quotas[q], skip, units.data(), rank, order, pbits.data(),
                               foff + (size_t)q * n_units, sizes + q, rcs + q, kept + q);
    return flags;
}

#ifdef ROI_EMU_MAIN
#include <stdio.h>
// Ranks against std::sort and the ranked scan against a plain walk, on a few geometries, rectangles and shifts.
int main()
{
    struct Geo { uint32_t w, h; int channels, stages, segments, bits; };
    const Geo geos[] = {{96, 80, 1, 3, 6, 16}, {72, 56, 3, 2, 4, 16}, {64, 64, 3, 2, 3, 8}, {256, 192, 1, 4, 32, 16}, {40, 40, 1, 1, 1, 16}, {9, 200, 1, 1, 17, 16}};
    std::mt19937 rng(12345);
    int checked = 0;
    for (const Geo &g : geos) {
        const int n = emu_roi_plan(g.w, g.h, g.channels, g.stages, g.segments, g.bits);
        if (n <= 0) { printf("plan refused %u x %u: %d\n", g.w, g.h, n); return 1; }
        const uint32_t rois[][4] = {{0, 0, 0, 0}, {0, 0, g.w, g.h}, {g.w / 3, g.h / 3, 5, 7}, {g.w - 4, g.h - 4, 100, 100}, {g.w - 1, g.h - 1, 1, 1},
                                    {g.w, 0, 10, 10}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, {3, 2, 0xFFFFFFFFu, 0xFFFFFFFFu}};
        for (const auto &roi : rois)
            for (uint32_t shift = 0; shift <= (uint32_t)kMaxRoiShift; shift++) {
                std::vector<uint32_t> rank(n), order(n), want(n);
                uint32_t n_fg = 0;
                emu_roi_rank(roi, shift, shift * 7u + 1u, rank.data(), order.data(), &n_fg);
                const RoiBox box = roi_clip(roi, g.w, g.h);
                std::vector<uint64_t> eff(n);
                uint32_t fg = 0;
                for (int u = 0; u < n; u++) {
                    const bool f = roi_foreground(g_plan.units[u], g.w, g.h, box);
                    fg += f;
                    eff[u] = g_prio[u] << (f ? roi_shift(box, shift) : 0u);
                    want[u] = (uint32_t)u;
                }
                std::sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return eff[a] != eff[b] ? eff[a] > eff[b] : a < b; });
                if (fg != n_fg || want != order) { printf("order differs: %u x %u shift %u\n", g.w, g.h, shift); return 1; }
                for (int i = 0; i < n; i++) if (rank[order[i]] != (uint32_t)i) { printf("rank is not the inverse\n"); return 1; }
                // the ranked scan at a few quotas
                std::vector<uint32_t> bits(n);
                for (auto &b : bits) { const uint32_t r = rng() % 20u; b = r == 0 ? 0u : r == 1 ? kUnitTooBig : rng() % 5000u; }
                std::vector<uint8_t> bound(n, 1);
                const uint64_t quotas[4] = {0, 28, (uint64_t)(rng() % (40u * n + 1u)), 1u << 30};
                std::vector<uint64_t> foff(4 * (size_t)n);
                unsigned long long sizes[4]; int32_t rcs[4]; uint32_t kept[4];
                emu_scan_roi(bits.data(), quotas, 4, 0, bound.data(), rank.data(), order.data(), foff.data(), sizes, rcs, kept);
                for (int q = 0; q < 4; q++) {
                    uint64_t used = 0; uint32_t K = 0;
                    for (; K < (uint32_t)n; K++) {
                        const uint32_t b = bits[order[K]];
                        if (b == kUnitTooBig || used + kHeaderBytes > quotas[q] || (b > 0 && (b >> 3) + used + kHeaderBytes >= quotas[q])) break;
                        used += kHeaderBytes + ((b + 7u) >> 3);
                    }
                    uint64_t off = 0;
                    for (int j = 0; j < n; j++) {
                        const uint32_t u = g_plan.final_order[j];
                        const uint64_t w = rank[u] < K ? off : ~0ull;
                        if (foff[(size_t)q * n + u] != w) { printf("offset differs\n"); return 1; }
                        if (rank[u] < K) off += kHeaderBytes + ((bits[u] + 7u) >> 3);
                    }
                    if (kept[q] != K || sizes[q] != used || off != used || rcs[q] != (K < (uint32_t)n ? kByteQuotaExceeded : kOk)) { printf("cut differs\n"); return 1; }
                    checked++;
                }
            }
    }
    printf("roi_emu: %d cuts checked\n", checked);
    return 0;
}
#endif
