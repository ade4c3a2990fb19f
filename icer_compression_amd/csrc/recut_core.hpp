// recut_core.hpp -- re-cutting a stored stream to smaller byte quotas (icerx_recut_device_async, recut.hpp): the two pieces
// that the rate ladder (assemble_ladder.hpp) and the device planner of the decoder (decoder_dplan.hpp) do not have.
//
// A byte quota decides only where a stream is cut, never what a packet holds ("Rate ladder").  So the
// stream the encoder makes at quota Q can be cut from a stored master of the same frame: the master's packet table
// (dplan_accept) gives the payload bits of every coding unit in priority order, the quota walk of scan_ladder_wave runs
// over them, and the kept packets are copied verbatim into the final order.
//
//   recut_unit_bits    a frame's packet table -> bit counts in Plan::units order; a unit without a packet counts as
//                      kUnitTooBig ("does not fit"), so the walk ends there
//   recut_scan_wave    one frame at one quota: scan_ladder_wave, or the frame's error (no offsets, size 0)
//   copy_unit_recut    copy_unit_ladder for a source of any byte alignment (a packet inside a stored stream)
// Written with the SPMD macros of wave.hpp, so that tests/emu/recut_emu.cpp runs the same source on a CPU.
#pragma once
#include "assemble_ladder.hpp"
#include "decoder_core.hpp"

namespace icer {

// bit counts of a frame's units (priority order) from its packet table, through the unit -> table slot map; thread `tid` of `nth`
ICER_HD void recut_unit_bits(const uint32_t *tab_off, const uint32_t *tab_bits, const uint32_t *unit_slot, uint32_t n_units,
                             uint32_t *bits, uint32_t tid, uint32_t nth)
{
    for (uint32_t u = tid; u < n_units; u += nth) {
        const uint32_t s = unit_slot[u];
        // (a data_length that reads as one of the coder's marks cannot be a packet of a real stream: no packet)
        bits[u] = (tab_off[s] == kNoPacket || tab_bits[s] >= kUnitFailed) ? kUnitTooBig : tab_bits[s];
    }
}

// what the walk leaves of a frame: kInvalidInput for a frame outside the blob or a valid packet of another image size,
// kDecoderOutOfData without any valid packet, else kOk
ICER_HD int recut_frame_status(bool inside, uint32_t cursor, bool other_size)
{
    if (!inside || other_size) return kInvalidInput;
    return cursor == 0u ? kDecoderOutOfData : kOk;
}

// One frame at one quota, one wavefront: final offsets `foff`, stream length *size and return code *rc.  A frame with a
// status keeps nothing.  No unit is kUnitFailed and the unit table's cap_is_bound is 0, so scan_ladder_wave returns no flag.
ICER_DEV void recut_scan_wave(int status, const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t quota,
                              const UnitDesc *units, uint64_t *foff, unsigned long long *size, int32_t *rc)
{
    DECL_LANE;
    if (status != kOk) {
        FOR_LANES
        {
            for (uint32_t i = (uint32_t)lane; i < n_units; i += 64) foff[i] = ~0ull;
            if (lane == 0) { *size = 0; *rc = status; }
        }
        return;
    }
    (void)scan_ladder_wave(bits, final_order, n_units, quota, 0, units, foff, size, rc);
}

// One packet of `len` bytes (header + payload) at `src`, of ANY byte alignment, to its place in the stream of every quota
// that keeps it (arguments as copy_unit_ladder).  The source words that lie whole inside the packet -- from its first 4-byte
// boundary, `sa` bytes in -- are read once for all destinations; a destination whose own 4-byte boundary lies `shift`
// bytes behind a source word's builds its words from two of them (v_alignbyte) and stores them aligned; what is left at
// both ends (fewer than 8 bytes each) goes byte by byte.  Nothing outside [src, src + len) is read, nothing outside a
// destination's `len` bytes written.  Thread `tid` of `nth`.
ICER_DEV void copy_unit_recut(const uint8_t *src, uint32_t len, const uint64_t *offs, size_t off_pitch, uint32_t n_q,
                              uint8_t *out, size_t q_pitch, uint32_t tid, uint32_t nth)
{
    const uint32_t sa = (uint32_t)((4u - ((uintptr_t)src & 3u)) & 3u);
    const uint32_t nfull = len > sa ? (len - sa) >> 2 : 0u;            // whole source words
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src + (nfull ? sa : 0u));
    for (uint32_t q = 0; q < n_q; q++) {                               // heads and tails
        const uint64_t off = offs[(size_t)q * off_pitch];
        if (off == ~0ull) continue;
        uint8_t *dst = out + (size_t)q * q_pitch + off;
        const uint32_t shift = (4u - (uint32_t)(((uintptr_t)dst + sa) & 3u)) & 3u;      // (dst + sa + shift is 4-byte aligned)
        const uint32_t nw = shift ? (nfull ? nfull - 1u : 0u) : nfull; // words stored: unit bytes [start, start + 4 nw)
        const uint32_t start = nw ? sa + shift : len, end = nw ? start + 4u * nw : len;
        for (uint32_t j = tid; j < start; j += nth) dst[j] = src[j];
        for (uint32_t j = end + tid; j < len; j += nth) dst[j] = src[j];
    }
    for (uint32_t i = tid; i < nfull; i += nth) {
        const uint32_t lo = sw[i], hi = i + 1u < nfull ? sw[i + 1u] : 0u;
        for (uint32_t q = 0; q < n_q; q++) {
            const uint64_t off = offs[(size_t)q * off_pitch];
            if (off == ~0ull) continue;
            uint8_t *dst = out + (size_t)q * q_pitch + off;
            const uint32_t shift = (4u - (uint32_t)(((uintptr_t)dst + sa) & 3u)) & 3u;
            if (shift && i + 1u >= nfull) continue;
            reinterpret_cast<uint32_t *>(dst + sa + shift)[i] = shift ? (lo >> (8u * shift)) | (hi << (32u - 8u * shift)) : lo;
        }
    }
}

}  // namespace icer
