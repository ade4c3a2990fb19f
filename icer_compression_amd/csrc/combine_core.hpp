// combine_core.hpp -- the set algebra of icerx_combine_device_async (combine.hpp) on two packet tables of one frame: which
// operand a coding unit's packet is taken from, the frame's status, and the two passes over a part of the final order that the
// workgroup's scan is made of.  Plain host/device functions, so that the mock build runs the same text.
//
//   UNION        unit u is kept when A or B has a valid packet of it; B's if B has one, else A's
//   DIFFERENCE   unit u is kept when B has a valid packet of it and A has none; B's
// "Has" is decided by the unit alone (its slot of the packet table is filled), never by comparing payloads.
#pragma once
#include "recut_core.hpp"

namespace icer {

constexpr int kCombineUnion = 0, kCombineDifference = 1;                 // ICERX_COMBINE_UNION / _DIFFERENCE
constexpr uint32_t kCombineNone = 0, kCombineFromA = 1, kCombineFromB = 2;

// where unit u's packet comes from
ICER_HD uint32_t combine_source(int op, bool a_has, bool b_has)
{
    if (b_has) return (op == kCombineUnion || !a_has) ? kCombineFromB : kCombineNone;
    return (op == kCombineUnion && a_has) ? kCombineFromA : kCombineNone;
}

// the frame's status from its operands' (recut_frame_status each): either one invalid -> kInvalidInput; then UNION has no
// stream when neither holds a valid packet, DIFFERENCE when B holds none
ICER_HD int combine_frame_status(int op, int status_a, int status_b)
{
    if (status_a == kInvalidInput || status_b == kInvalidInput) return kInvalidInput;
    if (op == kCombineUnion) return (status_a == kOk || status_b == kOk) ? kOk : kDecoderOutOfData;
    return status_b;
}

// header and payload of a packet of `bits` payload bits
ICER_HD uint32_t combine_packet_bytes(uint32_t bits) { return (uint32_t)kHeaderBytes + (bits >> 3) + ((bits & 7u) ? 1u : 0u); }

struct CombineSum {
    uint64_t bytes;                                   // of the kept packets
    uint32_t packets, from_a;
};

// the packet tables of a frame's two operands (tab_off: offset in the operand, kNoPacket: none)
struct CombineTables {
    const uint32_t *off_a, *bits_a, *off_b, *bits_b;
};

ICER_HD uint32_t combine_unit_source(int op, const CombineTables &t, uint32_t slot)
{
    return combine_source(op, t.off_a[slot] != kNoPacket, t.off_b[slot] != kNoPacket);
}

// positions [i0, i1) of the final order: what they keep
ICER_HD CombineSum combine_sum_range(int op, const CombineTables &t, const uint32_t *unit_slot, const uint32_t *final_order, uint32_t i0,
                                     uint32_t i1)
{
    CombineSum s;
    s.bytes = 0; s.packets = 0; s.from_a = 0;
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t slot = unit_slot[final_order[i]], src = combine_unit_source(op, t, slot);
        if (src == kCombineNone) continue;
        s.bytes += combine_packet_bytes(src == kCombineFromA ? t.bits_a[slot] : t.bits_b[slot]);
        s.packets++;
        s.from_a += src == kCombineFromA ? 1u : 0u;
    }
    return s;
}

// positions [i0, i1) of the final order, the first kept packet of which lies `at` bytes into the result: per unit its offset
// there (foff, ~0: not kept), where its packet starts in the blob and how long it is.  place = false: nothing is kept.
ICER_HD void combine_place_range(int op, const CombineTables &t, const uint32_t *unit_slot, const uint32_t *final_order, uint32_t i0,
                                 uint32_t i1, bool place, uint64_t at, uint32_t blob_off_a, uint32_t blob_off_b, uint64_t *foff,
                                 uint32_t *from, uint32_t *bytes)
{
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t u = final_order[i], slot = unit_slot[u], src = place ? combine_unit_source(op, t, slot) : kCombineNone;
        if (src == kCombineNone) { foff[u] = ~0ull; continue; }
        const bool a = src == kCombineFromA;
        const uint32_t len = combine_packet_bytes(a ? t.bits_a[slot] : t.bits_b[slot]);
        foff[u] = at;
        from[u] = a ? blob_off_a + t.off_a[slot] : blob_off_b + t.off_b[slot];
        bytes[u] = len;
        at += len;
    }
}

}  // namespace icer
