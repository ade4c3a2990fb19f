// TESTS ONLY: the re-cut's own device functions (csrc/recut_core.hpp) as a CPU lane-loop build (-DICER_WAVE_EMU, see
// csrc/wave.hpp), beside scan_frame_wave alone, so that tests/test_emu_recut.py can compare them with one scan and one
// plain copy per quota.  Not part of the product library.
#define ICER_WAVE_EMU 1
#include "../../icer_compression_amd/csrc/recut_core.hpp"
#include <vector>

using namespace icer;

unsigned long long g_emu_chunks[4] = {0, 0, 0, 0};       // (coder_core.hpp's path counters: unused here, defined by every emu build)

// scan_frame_wave on its own; returns its rc
extern "C" int emu_scan_frame(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t quota, uint64_t *foff,
                              uint32_t *kept, uint64_t *used)
{
    return scan_frame_wave(bits, final_order, n_units, quota, foff, kept, used);
}

// recut_plan_kernel's work on one frame after the walk: the frame's status, the units' bit counts out of the packet table
// (`nth` threads, one after another), then one recut_scan_wave per quota; final offsets of quota q at foff[q * n_units],
// sizes / rcs at [q].  Returns the status.
extern "C" int emu_recut_plan(int inside, uint32_t cursor, int other_size, const uint32_t *tab_off, const uint32_t *tab_bits,
                              const uint32_t *unit_slot, uint32_t n_units, const uint32_t *final_order, const uint64_t *quotas,
                              uint32_t n_q, uint32_t nth, uint32_t *bits, uint64_t *foff, unsigned long long *sizes, int32_t *rcs)
{
    const int status = recut_frame_status(inside != 0, cursor, other_size != 0);
    if (status == kOk)
        for (uint32_t t = 0; t < nth; t++) recut_unit_bits(tab_off, tab_bits, unit_slot, n_units, bits, t, nth);
    std::vector<UnitDesc> units(n_units);                   // (cap_is_bound = 0, as the recutter uploads them)
    for (uint32_t q = 0; q < n_q; q++)
        recut_scan_wave(status, bits, final_order, n_units, quotas[q], units.data(), foff + (size_t)q * n_units, sizes + q, rcs + q);
    return status;
}

// recut_gather_kernel's copy of one packet, its `nth` threads run one after another (they write disjoint bytes)
extern "C" void emu_copy_recut(const uint8_t *src, uint32_t len, const uint64_t *offs, size_t off_pitch, uint32_t n_q, uint8_t *out,
                               size_t q_pitch, uint32_t nth)
{
    for (uint32_t t = 0; t < nth; t++) copy_unit_recut(src, len, offs, off_pitch, n_q, out, q_pitch, t, nth);
}
