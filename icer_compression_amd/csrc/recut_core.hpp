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
// and, for cuts by resolution as well (icerx_recut_device_cuts_async), at the end of this file:
//   recut_cut_status   a frame's status at reduce r, from what its walk left (RecutFrameHead)
//   recut_cut_header   a kept packet's header as it stands in the derived stream at reduce r
//   recut_offsets_by_master_unit   a cut's final offsets, from its geometry's unit order to the master's
// Written with the SPMD macros of wave.hpp, so that tests/emu/recut_emu.cpp runs the same source on a CPU.
#pragma once
#include "assemble_ladder.hpp"
#include "decoder_core.hpp"
#include "decoder_plan.hpp"

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
ICER_DEV void copy_unit_recut(const uint8_t *__restrict__ src, uint32_t len, const uint64_t *__restrict__ offs, size_t off_pitch, uint32_t n_q,
                              uint8_t *__restrict__ out, size_t q_pitch, uint32_t tid, uint32_t nth)
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

// ---- cuts by resolution as well as by byte quota (icerx_recut_device_cuts_async) --------------------------------------
// A cut (reduce r, quota Q) of a master M is the re-cut at Q of its derived stream M_r (include/icer_hip_dec.h): M's packet
// table is read through the unit -> slot map of the geometry at 1/2^r size, whose unit (ch, lv, sb, sg, lsb) is M's slot
// (ch, lv + r, sb, sg, lsb), and a kept packet gets the header it has in M_r.
constexpr int kRecutMaxReduce = kMaxStages - 1;

// a frame's status at reduce r: the master's own, and at r > 0 no stream when no valid packet lies above level r
ICER_HD int recut_cut_status(int status, uint32_t max_level, uint32_t reduce)
{
    if (status != kOk || reduce == 0u) return status;
    return max_level <= reduce ? kDecoderOutOfData : kOk;
}
// what a master's walk leaves of a frame (recut_walk, recut.hpp), and the head of every call's frame record
struct RecutFrameHead {
    int32_t status;
    uint32_t max_level;
};
ICER_HD int recut_cut_status(const RecutFrameHead &f, uint32_t reduce) { return recut_cut_status(f.status, f.max_level, reduce); }

// the 28 header bytes at `src` as they stand in the derived stream at reduce r -> dst: decomp_level - r, image_w and image_h
// ceil(. / 2^r), the header CRC over the 24 bytes before it; r = 0: a copy.  Any alignment on both sides, one thread.
ICER_HD void recut_cut_header(const uint32_t *__restrict__ crc_tab, const uint8_t *__restrict__ src, uint32_t reduce, uint8_t *__restrict__ dst)
{
    if (reduce == 0u) {
        for (uint32_t j = 0; j < (uint32_t)kHeaderBytes; j++) dst[j] = src[j];
        return;
    }
    const uint32_t w = (uint32_t)reduced_dim(load_le32(src + 8), (int)reduce), h = (uint32_t)reduced_dim(load_le32(src + 12), (int)reduce);
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < 24u; j++) {
        uint8_t b = src[j];
        if (j == 4u) b = (uint8_t)(b - reduce);
        else if (j >= 8u && j < 12u) b = (uint8_t)(w >> (8u * (j - 8u)));
        else if (j >= 12u && j < 16u) b = (uint8_t)(h >> (8u * (j - 12u)));
        dst[j] = b;
        c = crc_tab[(c ^ b) & 255u] ^ (c >> 8);
    }
    c ^= 0xFFFFFFFFu;
    for (uint32_t j = 0; j < 4u; j++) dst[24u + j] = (uint8_t)(c >> (8u * j));
}

// final offsets of one frame at one cut, from the order of the geometry at 1/2^r size (`by_unit`, what the quota walk
// leaves) to the order of the master's units: full_to_cut[u] is the unit of that geometry that master unit u stands for,
// kNoPacket for a unit of a level the cut leaves out.  Thread `tid` of `nth`.
ICER_HD void recut_offsets_by_master_unit(const uint64_t *by_unit, const uint32_t *full_to_cut, uint32_t n_full, uint64_t *by_master,
                                          uint32_t tid, uint32_t nth)
{
    for (uint32_t u = tid; u < n_full; u += nth) {
        const uint32_t v = full_to_cut[u];
        by_master[u] = v == kNoPacket ? ~0ull : by_unit[v];
    }
}

}  // namespace icer
