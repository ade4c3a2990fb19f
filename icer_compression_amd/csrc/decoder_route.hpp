// decoder_route.hpp -- which kernel decodes a chain.  What the synchronous batch decode (decode_batch, decoder.hip: decided on the host,
// route_batch_chains) and the asynchronous one (decoder_async.hpp: decided on the device, droute of decoder_dplan.hpp) share is written
// here once: ICER_DEC_WAVE, the planes kernel by load, the chains it takes.  The ring classes are NOT shared: decode_batch's are relative
// to the widest chain of the call, droute's to a fixed maximum.  Host arithmetic, no HIP call: tests/emu/decoder_emu.cpp runs it under g++.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <vector>
#include "decoder_wave.hpp"
#include "decoder_planes.hpp"

namespace icer {

// ICER_DEC_WAVE, read once per call: -1 unset or empty (the choice goes by load), 0, 1, 2 = anything else
inline int dec_wave_mode() { const char *m = getenv("ICER_DEC_WAVE"); return (!m || !m[0]) ? -1 : m[0] == '0' ? 0 : m[0] == '1' ? 1 : 2; }
// bit planes and sign bit of the sign-magnitude words, by sample size
struct PlaneBits { int nplanes, sign_bit; };
inline PlaneBits plane_bits(int bits) { return bits == 8 ? PlaneBits{kPlanes8, 7} : PlaneBits{kPlanes, 15}; }

struct DRouteRule {
    int mode;                                      // dec_wave_mode()
    uint32_t planes_lds_limit;                     // dynamic LDS the planes kernel may take
    uint32_t ring_elems_max;                       // the largest row ring of the lane-per-plane kernel (droute's class 0)
    uint32_t nplanes;
};
// the planes kernel by load: unless pinned, only while the fast chains are at most 12 per compute unit (the measurements: below)
ICER_HD bool dwant_planes(int mode, uint32_t lut_ok, uint32_t n_fast, uint32_t n_cus)
{
    return mode != 0 && mode != 1 && lut_ok != 0u && (mode != -1 || n_fast <= 12u * n_cus);
}
// ... and the chains it takes then: every packet on the fast entropy path, control words + row ring inside the LDS limit
ICER_HD bool takes_planes(const DRouteRule &r, const ChainDesc &c, uint32_t stream_len, bool want_planes)
{
    return want_planes && c.fast && stream_len >= 4u && pw_lds_bytes(c.w, (int)r.nplanes) <= r.planes_lds_limit;
}
// may the lane-per-plane kernel take a row ring of this many elements?  Its per-lane state and its static DecoderTables block
// count against the same 64 KiB a launch gets without asking.
inline bool wave_ring_fits(size_t ring_elems) { return ring_elems * sizeof(uint16_t) + kStateBytes + sizeof(DecoderTables) + 256u <= 65536u; }

// decode_batch's order of the chains of a call, and what its launches need to know of it
constexpr int kRingClasses = 4;
struct BatchRoute {
    uint32_t n_fast;                               // chains [0, n_fast): the wave-per-plane kernel, one launch
    size_t planes_lds;                             // ... whose dynamic LDS is that of its widest chain
    uint32_t class_end[kRingClasses];              // chains [class_end[k - 1] (n_fast for k = 0), class_end[k]): ring class k
    size_t class_elems[kRingClasses];              // ... whose launch reserves this many ring elements: its widest chain's
    size_t rest_ring_elems;                        // the widest ring of the whole share behind n_fast
};
// Which kernel decodes a chain (ICER_DEC_WAVE: 0 = one thread per chain, 1 = one wavefront per chain with a lane per
// bit plane, anything else / unset = one wavefront per bit plane wherever it applies):
//   wave-per-plane   chains whose packets all take the fast entropy path (ChainDesc::fast) and whose row ring fits LDS
//   the rest         the lane-per-plane kernel if ITS ring fits, else one thread per chain
// Unset, the choice goes by load.  A wave per plane is the faster DECISION (303 against 634 ms for the 160 chains of
// the 4096 x 4096 headline stream), but a compute unit's throughput with it saturates near ONE long chain (what the
// waves of several chains share is the compute unit's scalar unit: 0.6-0.75 scalar instructions per cycle at 8-16
// streams, profiles/r04_logs/r04_l_planes_sq_counters.log; the wait loops are not it, r04_m), while the lane-per-plane
// kernel keeps seven long chains per compute unit going (LDS for their row rings), each at half the speed.  With the
// chains in longest-first order (below; profiles/r04_logs/r04_k_*.json, r04_m_*.json), streams per call -> Mpix/s:
//   wave per plane   4: 220   8: 437   16: 525-586   32: 537   64: 519
//   lane per plane   4: 107            16: 435       32: 922   64: 885-921   128: 1036
// -- the cross-over lies near 20 streams = 12 chains per compute unit (24 streams by this rule: 686).  ICER_DEC_WAVE=2
// pins the wave-per-plane kernel.
// stream_len_of_frame(f): the bytes of the stream of frame f (ChainDesc::frame).  The elements are chains or anything that
// carries one (a decode session's runs, decoder_session.hpp): chain_of(element) -> const ChainDesc &.
template <class T, class ChainOf, class StreamLenOf>
BatchRoute route_batch_chains(std::vector<T> &chains, ChainOf chain_of, StreamLenOf stream_len_of_frame, bool want_planes, size_t planes_lds_limit,
                              int nplanes)
{
    BatchRoute r = {};
    const DRouteRule rule = {-1, (uint32_t)std::min<size_t>(planes_lds_limit, 0xFFFFFFFFu), 0u, (uint32_t)nplanes};
    const auto rest = std::stable_partition(chains.begin(), chains.end(), [&](const T &e) {
        const ChainDesc &c = chain_of(e);
        return takes_planes(rule, c, stream_len_of_frame(c.frame), want_planes); });
    r.n_fast = (uint32_t)(rest - chains.begin());
    for (auto c = chains.begin(); c != rest; ++c) r.planes_lds = std::max(r.planes_lds, pw_lds_bytes(chain_of(*c).w, nplanes));
    // Longest chains first within either kernel's share (a chain's time goes with its samples): the level-1 chains of
    // every stream start at once, one or two per compute unit, and the short ones fill the gaps -- in stream order the
    // long chains of the later streams of a batch started when those of the first were half-way.
    auto longer = [&](const T &ea, const T &eb) {
        const ChainDesc &a = chain_of(ea), &b = chain_of(eb);
        return (uint32_t)a.w * a.h > (uint32_t)b.w * b.h; };
    std::stable_sort(chains.begin(), rest, longer);
    std::stable_sort(rest, chains.end(), longer);
    // The lane-per-plane kernel's share by size class of row ring (a launch reserves the LDS of its widest chain for every
    // workgroup, and LDS is what bounds the chains a compute unit holds: 7 of the headline stream's level-1 chains, but 14
    // of level 2 and 28 of level 3): class k = rings of at most limit >> k bytes, widest class first, each class a launch
    // of its own on a stream of its own, all of them side by side.
    r.rest_ring_elems = 2;
    for (auto c = rest; c != chains.end(); ++c) r.rest_ring_elems = std::max(r.rest_ring_elems, ring_elems_for(chain_of(*c).w, nplanes));
    auto cls = [&](const T &x) {
        const size_t e = ring_elems_for(chain_of(x).w, nplanes);
        int k = 0;
        while (k + 1 < kRingClasses && e * 2u <= (r.rest_ring_elems >> k)) k++;
        return k;
    };
    std::stable_sort(rest, chains.end(), [&](const T &a, const T &b) { return cls(a) < cls(b); });
    auto at = rest;
    for (int k = 0; k < kRingClasses; k++) {
        for (r.class_elems[k] = 2; at != chains.end() && cls(*at) == k; ++at)
            r.class_elems[k] = std::max(r.class_elems[k], ring_elems_for(chain_of(*at).w, nplanes));
        r.class_end[k] = (uint32_t)(at - chains.begin());
    }
    return r;
}
template <class StreamLenOf>
BatchRoute route_batch_chains(std::vector<ChainDesc> &chains, StreamLenOf stream_len_of_frame, bool want_planes, size_t planes_lds_limit, int nplanes)
{
    return route_batch_chains(chains, [](const ChainDesc &c) -> const ChainDesc & { return c; }, stream_len_of_frame, want_planes, planes_lds_limit,
                              nplanes);
}

}  // namespace icer
