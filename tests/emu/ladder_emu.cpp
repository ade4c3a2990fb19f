// TESTS ONLY: the rate ladder's assembly (csrc/assemble_ladder.hpp) as a CPU lane-loop build (-DICER_WAVE_EMU, see
// csrc/wave.hpp), beside scan_frame_wave alone, so that tests/test_emu_ladder.py can compare the ladder with one scan and
// one copy per quota.  Not part of the product library.
#define ICER_WAVE_EMU 1
#include "../../icer_compression_amd/csrc/assemble_ladder.hpp"
#include <vector>

using namespace icer;

unsigned long long g_emu_chunks[4] = {0, 0, 0, 0};       // (coder_core.hpp's path counters: unused here, defined by every emu build)

// scan_frame_wave on its own (what scan_kernel does for a frame that is neither skipped nor failed); returns its rc
extern "C" int emu_scan_frame(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t quota, uint64_t *foff,
                              uint32_t *kept, uint64_t *used)
{
    return scan_frame_wave(bits, final_order, n_units, quota, foff, kept, used);
}

// scan_ladder_kernel for one frame: one scan_ladder_wave per quota, final offsets of quota q at foff[q * n_units], sizes / rcs
// at [q]; `cap_is_bound` per unit stands for the slot table.  Returns the OR of the slot-bound flag bits.
extern "C" uint32_t emu_scan_ladder(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, const uint64_t *quotas,
                                    uint32_t n_q, int skip, const uint8_t *cap_is_bound, uint64_t *foff, unsigned long long *sizes,
                                    int32_t *rcs)
{
    std::vector<UnitDesc> units(n_units);
    for (uint32_t u = 0; u < n_units; u++) units[u].cap_is_bound = cap_is_bound[u];
    uint32_t flags = 0;
    for (uint32_t q = 0; q < n_q; q++)
        flags |= scan_ladder_wave(bits, final_order, n_units, quotas[q], skip, units.data(), foff + (size_t)q * n_units, sizes + q, rcs + q);
    return flags;
}

// gather_ladder_kernel's copy of one unit, its `nth` threads run one after another (they write disjoint bytes)
extern "C" void emu_copy_unit(const uint8_t *src, uint32_t len, const uint64_t *offs, size_t off_pitch, uint32_t n_q, uint8_t *out,
                              size_t q_pitch, uint32_t nth)
{
    for (uint32_t t = 0; t < nth; t++) copy_unit_ladder(src, len, offs, off_pitch, n_q, out, q_pitch, t, nth);
}
