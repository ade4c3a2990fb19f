// distortion_core.hpp -- cutting a frame where a distortion target is met (icerx_encode_device_target).
//
// A unit is one bit plane of one family -- a (channel, level, subband, segment) rectangle --, a stream keeps a prefix of the
// units in priority order (quota_cut_wave), and the decoder rebuilds a magnitude by truncation (decoder_core.hpp:
// val = cur | (bit << lsb)).  So with P coded planes and the planes >= b of a family kept, a coefficient of magnitude m is
// left with the error r_b(m) = m with its bits [b, P) cleared (bits >= P are never sent and always count; b = P: nothing
// kept), and the squared error of a stream in the wavelet domain is an exact integer function of the coefficient planes:
//
//   energy_block_wave / energy_block_commit   E[family][b] = sum of r_b(m)^2 over the family's rectangle, b = 0 .. P
//   scan_target_wave                          D_k = sum over families of weight x E[family][lowest plane among units [0, k), or P]
//                                             + the LL means' loss in the packet header (mean_loss);
//                                             the cut K = the first k with D_k <= T, or where the byte cap ends the walk
//
// (weights: subband_gain.hpp, Q4).  Everything is integer: partial sums are added in any order to the same result.
// Written with the SPMD macros of wave.hpp, so that tests/emu/distortion_emu.cpp runs the same source on a CPU.
#pragma once
#include "assemble_ladder.hpp"

namespace icer {

constexpr int kEnergyWaves = 4;                     // wavefronts of a workgroup of the energy pass
constexpr uint32_t kEnergyBlock = 4096;             // coefficients per workgroup: one entry of Plan::sig_blocks (64 chunks of 64)
constexpr int kEnergyEntries = kPlanes + 1;         // b = 0 .. P for the largest P

// The thresholds of a target call, passed by value with the launch (as LadderQuotas).
struct TargetList {
    uint64_t t[kMaxLadder];
};

struct EnergyShared {
    unsigned long long part[kEnergyWaves][kEnergyEntries];      // the waves' sums
};
struct EnergyLane {
    unsigned long long a[kEnergyEntries];
};

// Wave `wv` of the `nwv` of a workgroup, for coefficients [blk * kEnergyBlock, + kEnergyBlock) of the rectangle of `u` (row-major
// inside the rectangle; `plane`: the channel's sign-magnitude words, rows `stride` apart): thread t of the workgroup takes the
// coefficients first + t, first + t + threads, ...  Leaves the wave's sums in s.part[wv].
//
// Widths: m < 2^15, so r^2 <= (2^15 - 1)^2 = 2^30 - 2^16 + 1, and FOUR of them are at most 2^32 - 2^18 + 4 < 2^32: a lane adds
// four squares in 32 bits, then widens.  A workgroup adds at most 4096 squares (< 2^42) and a family fewer than 2^32 (65535^2
// coefficients): < 2^62 in the 64-bit entries.
ICER_DEV void energy_block_wave(EnergyShared &s, const uint16_t *plane, uint32_t stride, const UnitDesc &u, uint32_t blk, uint32_t wv,
                                uint32_t nwv, uint32_t P)
{
    DECL_LANE;
    const uint32_t n = u.w * u.h, first = blk * kEnergyBlock;
    const uint32_t end = n - first < kEnergyBlock ? n : first + kEnergyBlock;
    const uint32_t nth = 64u * nwv, sent = (1u << P) - 1u;            // `sent`: the bits a stream can carry
    LANEVAR(EnergyLane, acc);
    FOR_LANES
    {
        for (int b = 0; b < kEnergyEntries; b++) LV(acc).a[b] = 0;
        for (uint32_t i0 = first + wv * 64u + (uint32_t)lane; i0 < end; i0 += 4u * nth) {
            uint32_t four[kEnergyEntries];
            for (int b = 0; b < kEnergyEntries; b++) four[b] = 0;
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t i = i0 + k * nth;
                if (i >= end) break;
                const uint32_t y = i / u.w, x = i - y * u.w;
                const uint32_t m = plane[(size_t)(u.y0 + y) * stride + u.x0 + x] & 0x7FFFu;
                const uint32_t hi = m & ~sent, lo = m & sent;
                for (int b = 0; b < kEnergyEntries; b++) {              // (b > P: r = m, never read)
                    const uint32_t r = hi | (lo & ((1u << b) - 1u));
                    four[b] += r * r;
                }
            }
            for (int b = 0; b < kEnergyEntries; b++) LV(acc).a[b] += four[b];
        }
    }
    for (int b = 0; b < kEnergyEntries; b++) {
        LANEVAR(unsigned long long, x);
        FOR_LANES { LV(x) = LV(acc).a[b]; }
        unsigned long long tot;
        WAVE_SUM64(tot, x);
        FOR_LANES
        {
            if (lane == 0) s.part[wv][b] = tot;
        }
    }
}

// After every wave of the workgroup has left its sums (a workgroup barrier in between): thread `tid` <= P adds the workgroup's
// sum for b = tid to the family's entry, E_family[tid] -- one 64-bit integer add per entry and workgroup, which other workgroups
// of the family add to as well (zeroed before the launch).  Integer adds: the table does not depend on their order.
ICER_DEV void energy_block_commit(const EnergyShared &s, uint32_t nwv, uint32_t P, unsigned long long *E_family, uint32_t tid)
{
    if (tid > P) return;
    unsigned long long sum = 0;
    for (uint32_t w = 0; w < nwv; w++) sum += s.part[w][tid];
    if (sum) GLOBAL_ADD64(E_family + tid, sum);
}

// The term a unit takes out of the frame's distortion when it is kept: its family moves from plane lsb + 1 to plane lsb
// (the planes of a family come in the priority order from the top down, make_packets).  r_{b+1}(m) >= r_b(m): never negative.
ICER_DEV uint64_t unit_gain(const UnitDesc &u, const unsigned long long *E, const uint32_t *fam_weight, uint32_t P)
{
    const unsigned long long *e = E + (size_t)u.family * (P + 1u);
    return (uint64_t)fam_weight[u.family] * (e[u.lsb + 1u] - e[u.lsb]);
}

// The LL mean of a channel travels in ONE byte of the packet header (lib_icer's format; finish_unit_wave: mean & 0xFF): a decoder adds
// back mean & 0xFF, and every LL coefficient of the channel comes back short by mean & 0xFF00, at any quota.  The frame's distortion
// counts that as a constant: fam_ll_term[f] x (mean & 0xFF00)^2 with fam_ll_term[f] = weight x coefficients of an LL family, 0 for
// every other family (and for the uint8 twins, whose mean is a byte).  The cross term with the coded residual is left out: the LL
// residuals of a channel sum to less than its coefficient count by the definition of the mean.
ICER_DEV unsigned long long mean_loss(uint16_t mean)
{
    const unsigned long long d = mean & 0xFF00u;
    return d * d;
}

// One frame at one target, one wavefront: the cut K = min(K_t, K_cap) with K_t the first k whose distortion D_k is <= T
// (D_0: nothing kept; D_k: units [0, k) kept) and K_cap where the byte cap ends the walk (quota_cut_wave); then what
// scan_ladder_wave leaves for that cut -- final offsets `foff`, *size, *rc -- and
//   *reached   1: D_K <= T, 0: the byte cap (or the end of the units) came first
//   *dist      D_K
//   *equiv     a byte quota at which the plain walk (scan_frame_wave) makes this very cut
// A dropped frame (drop_frame_wave): no stream, *reached 0, *dist 0, *equiv the cap.  Returns the slot-bound flag bits as
// scan_ladder_wave; bit 0 only when the byte cap made the cut (a frame whose target was met earlier needs no larger slots).
//
// *equiv.  With used = the bytes of the units [0, K) (= *size), unit j is kept at quota Q iff its header fits,
// used_j + 28 <= Q, and bits_j == 0 or floor(bits_j / 8) + used_j + 28 < Q (P3, quota_cut_wave).
//   K < n_units, bits_K > 0:  Q = used + 28 + floor(bits_K / 8).  Unit K: floor(bits_K / 8) + used + 28 = Q is not < Q: dropped.
//       A unit j < K: used_j + 28 + floor(bits_j / 8) <= used_j + 28 + ceil(bits_j / 8) = used_{j+1} <= used < Q: kept.
//   K < n_units, bits_K == 0: Q = used + 27.  Unit K: used + 28 > Q: dropped.  A unit j < K: used_{j+1} <= used < used + 27
//       (and its header: used_j + 28 <= used_{j+1}): kept.
//   K == n_units: every unit fits the cap, Q = the cap.
//   bits_K == kUnitTooBig (only where the cap made the cut: K_cap never passes such a unit): the unit has no bit count
//       to make a quota from; the cap itself makes this cut, Q = the cap.
ICER_DEV uint32_t scan_target_wave(const uint32_t *bits, const uint32_t *final_order, uint32_t n_units, uint64_t T, uint64_t byte_cap, int skip,
                                   const UnitDesc *units, const unsigned long long *E, const uint32_t *fam_weight, uint32_t n_families,
                                   uint32_t P, const unsigned long long *fam_ll_term, const uint32_t *fam_chan, const uint16_t *means, uint64_t *foff, unsigned long long *size, int32_t *rc, int32_t *reached,
                                   unsigned long long *dist, unsigned long long *equiv)
{
    DECL_LANE;
    uint32_t flags = 0;
    if (drop_frame_wave(bits, n_units, skip, foff, size, rc, &flags)) {
        FOR_LANES
        {
            if (lane == 0) { *reached = 0; *dist = 0; *equiv = byte_cap; }
        }
        return flags;
    }
    // D_0: every family at plane P, and what no unit takes out: the LL mean's bits above its header byte (mean_loss)
    uint64_t d0 = 0;
    for (uint32_t base = 0; base < n_families; base += 64) {
        LANEVAR(unsigned long long, x);
        FOR_LANES
        {
            const uint32_t f = base + (uint32_t)lane;
            LV(x) = f < n_families ? (unsigned long long)fam_weight[f] * E[(size_t)f * (P + 1u) + P] + fam_ll_term[f] * mean_loss(means[fam_chan[f]]) : 0ull;
        }
        unsigned long long tot;
        WAVE_SUM64(tot, x);
        d0 += tot;
    }
    // K_t: lane l of a round holds D_k for k = base + l
    uint32_t Kt = n_units + 1u;                                         // (not met)
    uint64_t run = d0;
    for (uint32_t base = 0; base < n_units && Kt > n_units; base += 64) {
        LANEVAR(uint64_t, g); LANEVAR(uint64_t, before);
        FOR_LANES
        {
            const uint32_t k = base + (uint32_t)lane;
            LV(g) = k < n_units ? unit_gain(units[k], E, fam_weight, P) : 0ull;
        }
        uint64_t total;
        WAVE_EXCL_SCAN(uint64_t, before, g, total);
        const uint64_t met = BALLOT((base + (uint32_t)lane < n_units) && (run - LV(before) <= T));
        if (met) Kt = base + (uint32_t)ffs64(met);
        else run -= total;
    }
    if (Kt > n_units && run <= T) Kt = n_units;                         // (met by the last unit)
    const uint32_t Kcap = quota_cut_wave(bits, n_units, byte_cap);
    const uint32_t K = Kt < Kcap ? Kt : Kcap;
    // D_K
    uint64_t dk = d0;
    for (uint32_t base = 0; base < K; base += 64) {
        LANEVAR(unsigned long long, x);
        FOR_LANES
        {
            const uint32_t k = base + (uint32_t)lane;
            LV(x) = k < K ? unit_gain(units[k], E, fam_weight, P) : 0ull;
        }
        unsigned long long tot;
        WAVE_SUM64(tot, x);
        dk -= tot;
    }
    uint64_t used;
    const int r = final_offsets_wave(bits, final_order, n_units, K, foff, &used);
    uint64_t q = byte_cap;
    if (K < n_units && bits[K] != kUnitTooBig) q = bits[K] ? used + kHeaderBytes + (bits[K] >> 3) : used + kHeaderBytes - 1u;
    if (K == Kcap && K < n_units && bits[K] == kUnitTooBig && units[K].cap_is_bound) flags |= 1;
    FOR_LANES
    {
        if (lane == 0) { *size = used; *rc = r; *reached = Kt <= Kcap ? 1 : 0; *dist = dk; *equiv = q; }
    }
    return flags;
}

}  // namespace icer
