// assemble_ladder.hpp -- stream assembly of a rate ladder: one coded batch cut at several byte quotas
// (icerx_encode_device_ladder).
//
// The quota decides only where the walk of scan_frame_wave stops (P3, quota_cut_wave): a unit is kept whole or the
// walk ends, and that cut never moves back as the quota grows.  So units coded once -- in slots sized for the LARGEST
// quota, with progressive mode (if any) stopped at it -- hold every unit that any smaller quota keeps, and each
// quota's stream is scan + gather over the same slots ("Rate ladder").
//
//   drop_frame_wave    a skipped frame, a frame with a failed unit: no stream
//   scan_ladder_wave   scan_kernel's per-frame work at one quota (frame skip, failed units, quota walk, slot-bound
//                      check), one wavefront
//   copy_unit_ladder   gather_kernel's per-unit copy to every quota's stream that keeps the unit, the source words read once
// Written with the SPMD macros of wave.hpp, so that tests/emu/ladder_emu.cpp runs the same source on a CPU.
#pragma once
#include "assemble_core.hpp"
#include "plan.hpp"

namespace icer {

constexpr int kMaxLadder = 16;               // quotas per call (ICERX_MAX_LADDER)

// The quotas of a ladder call, passed by value with the launch (no upload).
struct LadderQuotas {
    uint64_t q[kMaxLadder];
};

// A frame that has no stream -- it was skipped (integer overflow) or one of its units reported an internal error (which makes the
// frame fail loudly): every final offset ~0, *size 0, *rc the reason.  Returns false for any other frame, nothing written;
// *flags |= 2 for a failed unit.
ICER_DEV bool drop_frame_wave(const uint32_t *bits, uint32_t n_units, int skip, uint64_t *foff, unsigned long long *size, int32_t *rc,
                              uint32_t *flags)
{
    DECL_LANE;
    bool drop = skip != 0;
    if (!drop) {
        LANEVAR(int, failed);
        FOR_LANES
        {
            LV(failed) = 0;
            for (uint32_t i = (uint32_t)lane; i < n_units; i += 64) LV(failed) |= bits[i] == kUnitFailed;
        }
        if (BALLOT(LV(failed))) { drop = true; *flags |= 2; }
    }
    if (!drop) return false;
    FOR_LANES
    {
        for (uint32_t i = (uint32_t)lane; i < n_units; i += 64) foff[i] = ~0ull;
        if (lane == 0) { *size = 0; *rc = skip ? kIntegerOverflow : kFatalError; }
    }
    return true;
}

// One frame at one quota: final offsets `foff`, stream length *size and return code *rc, as scan_kernel writes them.
// Returns the bits to OR into the slot-bound flag: 1 the cut lands on a unit that outgrew a slot sized by the
// bits-per-pixel bound (the batch is redone with larger slots), 2 a unit reported an internal error.
ICER_DEV uint32_t scan_ladder_wave(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t quota, int skip,
                                   const UnitDesc *units, uint64_t *foff, unsigned long long *size, int32_t *rc)
{
    DECL_LANE;
    uint32_t flags = 0;
    if (drop_frame_wave(bits, n_units, skip, foff, size, rc, &flags)) return flags;
    uint32_t kept;
    uint64_t used;
    const int r = scan_frame_wave(bits, final_order, n_units, quota, foff, &kept, &used);
    if (kept < n_units && bits[kept] == kUnitTooBig && units[kept].cap_is_bound) flags |= 1;
    FOR_LANES
    {
        if (lane == 0) { *size = used; *rc = r; }
    }
    return flags;
}

// One unit of `len` bytes (header + payload) from its slot `src` (4-byte aligned) to its place in the stream of every quota
// that keeps it: quota q's final offset is offs[q * off_pitch] (~0: dropped), its stream starts at out + q * q_pitch.  Thread
// `tid` of `nth`.  Every destination is byte-aligned only: as gather_kernel, a head of up to 3 bytes to its 4-byte boundary,
// aligned words built from two source words (v_alignbyte), then the tail -- with the source words of the body read once
// for all destinations.
ICER_DEV void copy_unit_ladder(const uint8_t *src, uint32_t len, const uint64_t *offs, size_t off_pitch, uint32_t n_q,
                               uint8_t *out, size_t q_pitch, uint32_t tid, uint32_t nth)
{
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src);
    const uint32_t src_words = (len + 3u) >> 2;           // words that hold a byte of the unit (inside its slot)
    for (uint32_t q = 0; q < n_q; q++) {                   // heads and tails
        const uint64_t off = offs[(size_t)q * off_pitch];
        if (off == ~0ull) continue;
        uint8_t *dst = out + (size_t)q * q_pitch + off;
        const uint32_t mis = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
        const uint32_t head = mis < len ? mis : len;
        const uint32_t done = head + ((len - head) >> 2) * 4u;
        for (uint32_t j = tid; j < head; j += nth) dst[j] = src[j];
        for (uint32_t j = tid; j < len - done; j += nth) dst[done + j] = src[done + j];
    }
    // body word i of a destination whose head is h holds source bytes [h + 4i, h + 4i + 4): words i and i + 1
    for (uint32_t i = tid; i < (len >> 2); i += nth) {
        const uint32_t lo = sw[i], hi = i + 1u < src_words ? sw[i + 1u] : 0u;
        for (uint32_t q = 0; q < n_q; q++) {
            const uint64_t off = offs[(size_t)q * off_pitch];
            if (off == ~0ull) continue;
            uint8_t *dst = out + (size_t)q * q_pitch + off;
            const uint32_t mis = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
            const uint32_t head = mis < len ? mis : len;
            if (i >= ((len - head) >> 2)) continue;
            const uint32_t shift = head * 8u;
            reinterpret_cast<uint32_t *>(dst + head)[i] = shift ? (lo >> shift) | (hi << (32u - shift)) : lo;
        }
    }
}

}  // namespace icer
