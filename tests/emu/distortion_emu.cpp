// TESTS ONLY: the distortion target's kernels (csrc/distortion_core.hpp) as a CPU lane-loop build (-DICER_WAVE_EMU, see
// csrc/wave.hpp): the energy pass workgroup by workgroup and wave by wave, in launch order or in a seeded random order, and
// scan_target_wave beside scan_frame_wave, for tests/test_emu_target.py.  Not part of the product library.
#define ICER_WAVE_EMU 1
#include "../../icer_compression_amd/csrc/distortion_core.hpp"
#include "../../icer_compression_amd/csrc/subband_gain.hpp"
#include <algorithm>
#include <random>
#include <vector>

using namespace icer;

unsigned long long g_emu_chunks[4] = {0, 0, 0, 0};       // (coder_core.hpp's path counters: unused here, defined by every emu build)

// family_energy_kernel for the families of one plane: family f is the rectangle rects[4f .. 4f + 3] = x0, y0, w, h; E[f][0 .. P]
// (zeroed here).  seed 0: workgroups and their waves in launch order; otherwise every (workgroup, wave) pair in a random order,
// then the workgroups' commits in another one.  Returns the workgroups run.
extern "C" uint32_t emu_family_energy(const uint16_t *plane, uint32_t stride, const uint32_t *rects, uint32_t n_families, uint32_t P,
                                      uint32_t seed, unsigned long long *E)
{
    struct Wg { uint32_t family, blk; };
    std::vector<Wg> wgs;
    std::vector<UnitDesc> units(n_families);
    for (uint32_t f = 0; f < n_families; f++) {
        UnitDesc &u = units[f];
        u.x0 = rects[4 * f]; u.y0 = rects[4 * f + 1]; u.w = rects[4 * f + 2]; u.h = rects[4 * f + 3];
        u.family = f;
        for (uint32_t b = 0; b * kEnergyBlock < u.w * u.h; b++) wgs.push_back(Wg{f, b});
        for (uint32_t b = 0; b <= P; b++) E[(size_t)f * (P + 1) + b] = 0;
    }
    std::vector<EnergyShared> lds(wgs.size());
    std::vector<uint32_t> waves(wgs.size() * kEnergyWaves), commits(wgs.size());
    for (uint32_t i = 0; i < waves.size(); i++) waves[i] = i;
    for (uint32_t i = 0; i < commits.size(); i++) commits[i] = i;
    if (seed) {
        std::mt19937 rng(seed);
        std::shuffle(waves.begin(), waves.end(), rng);
        std::shuffle(commits.begin(), commits.end(), rng);
    }
    for (uint32_t i : waves) {
        const Wg &g = wgs[i / kEnergyWaves];
        energy_block_wave(lds[i / kEnergyWaves], plane, stride, units[g.family], g.blk, i % kEnergyWaves, (uint32_t)kEnergyWaves, P);
    }
    for (uint32_t i : commits)
        for (uint32_t tid = 0; tid < 64u * kEnergyWaves; tid++)
            energy_block_commit(lds[i], (uint32_t)kEnergyWaves, P, E + (size_t)wgs[i].family * (P + 1), tid);
    return (uint32_t)wgs.size();
}

// scan_frame_wave on its own (what scan_kernel does for a frame that is neither skipped nor failed); returns its rc
extern "C" int emu_scan_frame(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t quota, uint64_t *foff,
                              uint32_t *kept, uint64_t *used)
{
    return scan_frame_wave(bits, final_order, n_units, quota, foff, kept, used);
}

// scan_target_kernel for one frame and one target; unit u belongs to family fam[u] at plane lsb[u], `cap_is_bound` stands for the slot
// table.  out[0] = size, out[1] = dist, out[2] = equiv; returns the slot-bound flag bits.
extern "C" uint32_t emu_scan_target(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t T, uint64_t byte_cap, int skip,
                                    const uint32_t *fam, const uint32_t *lsb, const uint8_t *cap_is_bound, const unsigned long long *E,
                                    const uint32_t *fam_weight, uint32_t n_families, uint32_t P, const unsigned long long *fam_ll_term,
                                    const uint32_t *fam_chan, const uint16_t *means, uint64_t *foff, unsigned long long *out,
                                    int32_t *rc, int32_t *reached)
{
    std::vector<UnitDesc> units(n_units);
    for (uint32_t u = 0; u < n_units; u++) { units[u].family = fam[u]; units[u].lsb = lsb[u]; units[u].cap_is_bound = cap_is_bound[u]; }
    return scan_target_wave(bits, final_order, n_units, T, byte_cap, skip, units.data(), E, fam_weight, n_families, P, fam_ll_term, fam_chan, means,
                            foff, out, rc, reached,
                            out + 1, out + 2);
}

extern "C" uint32_t emu_subband_gain(int filt, int level, int subband) { return kSubbandGainQ4[filt][level - 1][subband]; }
