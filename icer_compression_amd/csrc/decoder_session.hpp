// decoder_session.hpp -- progressive decode sessions (include/icer_hip_dec_session.h).  Included by decoder.hip behind
// decode_batch, whose stages it borrows: batch_packets in front, batch_samples and batch_results behind.
//
// A packet's context model starts fresh, and the only state a bit plane reads from the planes above it is the segment's
// sign-magnitude words (decode_chain, pw_step).  So a session keeps those words -- the STATE planes, uint16 in frame layout for
// 8-bit decoders too, zeroed at create and reset only, never transformed -- and a feed
//   1. finds and checks the feed's packets (batch_packets) and walks them on the host by the decoder's cursor rule;
//   2. accepts, per chain, the planes that continue what the slot holds (session_accept) and plans the slot with a table whose
//      held planes read kHeldPlane (plan_chains: the chains, levels and rc of the plain decode of everything accepted so far);
//   3. runs the chains that have new planes, in place on the state planes, routed like the plain decode (decoder_route.hpp;
//      ICER_DEC_WAVE = 0 / 1 / 2 pins a kernel): while the call's fast chains are at most 12 per compute unit, the wave-per-plane
//      kernel with a loader wave (pw_run_chain_resume) for chains that are `fast` and fit its LDS; above that load, and for every
//      chain under ICER_DEC_WAVE=1, the lane-per-plane kernel over a row ring that starts out holding the held words
//      (decode_chain_wave_resume) where the ring fits LDS; one thread per chain (decode_chain_resume) for what is left.  The last
//      two report where a chain stopped;
//   4. copies the fed slots' planes into the working buffer and runs batch_samples / batch_results on the copy as they are,
//      with the fed slots' chain table in d->chains for reconstruct_kernel (it counts planes from the top while
//      pkt != kNoPacket, so held planes count).
// Can a plane of the wave-per-plane kernel fail?  No: pw_decode_bin has no failing exit, as entropy_decode_fast has none -- every
// length test of the reference compares at most 11 bits with the packet's length, and the kernel takes packets of
// >= kFastPacketBits only.  So only the other two kernels write a status word.
#pragma once

namespace {

// one thread per chain, resuming below the held planes; lowest_ok[i]: decode_chain_resume
__global__ void __launch_bounds__(64)
decode_chains_resume_kernel(uint16_t *state, size_t frame_stride, int channels, const ChainDesc *__restrict__ chains, uint32_t n,
                            const uint8_t *__restrict__ data, const FrameInfo *__restrict__ frames,
                            const DecoderTables *__restrict__ tables, int nplanes, int sign_bit, uint32_t *__restrict__ lowest_ok)
{
    ICER_DYNAMIC_LDS(uint8_t, lds_state);                 // plane_block_bytes(64): the threads' per-bin arrays
    ICER_LDS_TABLES(lt, tables);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ChainDesc c = chains[i];
    const FrameInfo f = frames[c.frame];
    PlaneDecoder job;
    plane_attach_columns(job, lds_state, 64u, threadIdx.x);
    decode_chain_resume(job, chain_plane(state, c, channels, frame_stride), f.w, c, (int)c.subband, data + f.stream_off,
                        f.stream_len, lt, nplanes, sign_bit, lowest_ok + i);
}

// one wavefront per NEW bit plane and, for a chain that holds planes, a loader wave in front (pw_run_chain_resume); launch
// shape and LDS as decode_chains_planes_kernel
__global__ void __launch_bounds__(64 * kPwWaves)
decode_chains_planes_resume_kernel(uint16_t *state, size_t frame_stride, int channels, const ChainDesc *__restrict__ chains,
                                   const uint8_t *__restrict__ data, const FrameInfo *__restrict__ frames,
                                   const DecoderTables *__restrict__ tables, int nplanes, int sign_bit, uint32_t *__restrict__ err)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);
    const ChainDesc &c = chains[blockIdx.x];                  // (read in place: see pw_run_chain)
    const FrameInfo f = frames[c.frame];
    pw_workgroup_clear(lds, c, nplanes);
    const uint32_t wave = pw_workgroup_wave();
    (void)pw_run_chain_resume(lds, wave, c, nplanes, sign_bit, chain_plane(state, c, channels, frame_stride), f.w,
                              data + f.stream_off, f.stream_len, tables, err);
}

// one wavefront per chain and one lane per NEW bit plane, over a row ring that holds the held words (decode_chain_wave_resume);
// launch shape and LDS as decode_chains_wave_kernel, lowest_ok[chain of the launch]: decode_chain_resume
__global__ void __launch_bounds__(64)
decode_chains_wave_resume_kernel(uint16_t *state, size_t frame_stride, int channels, const ChainDesc *__restrict__ chains,
                                 const uint8_t *__restrict__ data, const FrameInfo *__restrict__ frames,
                                 const DecoderTables *__restrict__ tables, int nplanes, int sign_bit, uint32_t *__restrict__ lowest_ok)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                       // the lanes' per-bin arrays, then the chain's row ring
    ICER_LDS_TABLES(lt, tables);
    const ChainDesc c = chains[blockIdx.x];
    const FrameInfo f = frames[c.frame];
    uint16_t *ring = reinterpret_cast<uint16_t *>(lds + kStateBytes);
    decode_chain_wave_resume(ring, chain_plane(state, c, channels, frame_stride), f.w, c, (int)c.subband, data + f.stream_off,
                             f.stream_len, lt, nplanes, sign_bit, nullptr, lds, lowest_ok + blockIdx.x);
}

// the w * h words of every channel of row k's slot into row k of the working planes (grid.y = row * channels + channel)
__global__ void __launch_bounds__(256)
session_copy_kernel(const uint16_t *__restrict__ state, uint16_t *__restrict__ work, size_t frame_stride, int channels,
                    const FrameInfo *__restrict__ rows, const uint32_t *__restrict__ slot_of_row)
{
    const uint32_t row = blockIdx.y / (unsigned)channels, ch = blockIdx.y % (unsigned)channels;
    const FrameInfo f = rows[row];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)f.w * f.h) return;
    work[(size_t)blockIdx.y * frame_stride + i] = state[((size_t)slot_of_row[row] * channels + ch) * frame_stride + i];
}

}  // namespace

struct icerx_session {
    icerx_decoder *d = nullptr;
    int n_slots = 0;
    size_t frame_stride = 0;
    icerx_decoder::Buf state, frames, chains, status, rows;
    struct Slot {
        bool sized = false;
        size_t w = 0, h = 0;
        uint16_t mean[3] = {0, 0, 0};
        bool has_mean[3] = {false, false, false};
        std::vector<uint8_t> low, stopped;          // per PacketTable::chain_index: the lowest plane accepted (nplanes: none); stopped for good
    };
    std::vector<Slot> slots;
    uint64_t stats[4] = {0, 0, 0, 0};
    int lds_state = 0;                              // the resume planes kernel's dynamic LDS: 0 not asked yet, 1 granted, -1 refused
};

namespace {

size_t session_keys() { return PacketTable::chain_index(2, kMaxStages, 3, kMaxSegments) + 1u; }

void session_clear_slot(icerx_session *s, int slot)
{
    icerx_session::Slot &sl = s->slots[(size_t)slot];
    sl = icerx_session::Slot();
    sl.low.assign(session_keys(), (uint8_t)plane_bits(s->d->bits).nplanes);
    sl.stopped.assign(session_keys(), 0);
}

int session_reset_slot(icerx_session *s, int slot)
{
    const size_t per_slot = (size_t)s->d->channels * s->frame_stride;
    session_clear_slot(s, slot);
    if (per_slot && hipMemset((uint16_t *)s->state.p + (size_t)slot * per_slot, 0, sizeof(uint16_t) * per_slot) != hipSuccess)
        return fail("a session could not clear its state planes");
    return ICER_RESULT_OK;
}

// a chain of a feed that has new planes: hi .. lo
struct SessionRun { ChainDesc c; int slot; size_t key, recon_at; int hi, lo; };

// Feed k of a call, walked and accepted into its slot.  -> false: refused (rcs[k] says why; the slot is untouched, the row
// delivers nothing).  Else the slot's table has taken the feed's planes, pl is the plan of the plain decode of the slot's
// packets, and the chains with new planes are in `runs`, every chain of the plan in `recon` (frame = k).
bool session_accept(icerx_session *s, int k, int slot, const std::vector<PacketCandidate> &mine, DecodePlan &pl, int *rcs, size_t *ws,
                    size_t *hs, std::vector<SessionRun> &runs, std::vector<ChainDesc> &recon)
{
    const icerx_decoder *d = s->d;
    const int P = plane_bits(d->bits).nplanes;
    icerx_session::Slot &sl = s->slots[(size_t)slot];
    PacketTable feed;
    bool sized = sl.sized, refused = false, has_mean[3] = {sl.has_mean[0], sl.has_mean[1], sl.has_mean[2]};
    size_t w = sl.w, h = sl.h;
    uint16_t mean[3] = {sl.mean[0], sl.mean[1], sl.mean[2]};
    uint64_t walked = 0, accepted = 0;
    // every walked packet counts; one that names no table entry teaches the slot nothing, one that disagrees with the slot's
    // size or its channel's mean refuses the feed
    walk_packets(mine, d->channels, d->reduce, [&](const WalkedPacket &k) {
        walked++;
        if (!k.named()) return;
        if (!sized) { w = k.w; h = k.h; sized = true; }
        else if (k.w != w || k.h != h) refused = true;
        if (!has_mean[k.ch]) { mean[k.ch] = k.mean; has_mean[k.ch] = true; }
        else if (mean[k.ch] != k.mean) refused = true;
        k.enter(feed);
    });
    if (refused) {
        rcs[k] = ICER_INVALID_INPUT;
        if (sl.sized) { ws[k] = sl.w; hs[k] = sl.h; }
        return false;
    }
    // the slot's table: held planes, and below them what the feed continues them with
    PacketTable tab;
    const std::vector<uint8_t> before = sl.low;
    std::vector<uint8_t> low = sl.low;
    bool took[3] = {false, false, false};
    const size_t keys_per_channel = session_keys() / 3u;
    for (size_t key = 0; key < low.size(); key++) {
        for (int lsb = low[key]; lsb < P; lsb++) { tab.off[key * kPlanes + (size_t)lsb] = kHeldPlane; tab.bits[key * kPlanes + (size_t)lsb] = 0xFFFFFFFFu; }
        if (sl.stopped[key]) continue;
        int next = (int)low[key] - 1;
        for (; next >= 0 && feed.off[key * kPlanes + (size_t)next] != kNoPacket; next--, accepted++) {
            tab.off[key * kPlanes + (size_t)next] = feed.off[key * kPlanes + (size_t)next];
            tab.bits[key * kPlanes + (size_t)next] = feed.bits[key * kPlanes + (size_t)next];
            took[key / keys_per_channel] = true;
        }
        low[key] = (uint8_t)(next + 1);
    }
    // size and means are those of the packets the slot holds: a feed of which nothing is accepted teaches it nothing
    if (!sl.sized && accepted == 0) { w = ws[k]; h = hs[k]; }    // (nothing held: the caller's values, as the plain decode of no packet)
    ws[k] = w; hs[k] = h;
    if (s->frame_stride < w * h) { rcs[k] = ICER_BYTE_QUOTA_EXCEEDED; return false; }
    if (accepted) { sl.sized = true; sl.w = w; sl.h = h; }
    for (int c = 0; c < 3; c++)
        if (took[c]) { sl.mean[c] = mean[c]; sl.has_mean[c] = true; }
    sl.low = low;
    s->stats[3] += walked - accepted;
    pl = DecodePlan();
    pl.w = w; pl.h = h;
    for (int c = 0; c < 3; c++) pl.mean[c] = sl.has_mean[c] ? sl.mean[c] : (uint16_t)0;
    std::vector<size_t> keys;
    plan_chains(&pl, tab, d->channels, d->stages, d->segments, P, s->frame_stride, nullptr, &keys);
    rcs[k] = pl.rc;
    for (size_t i = 0; i < pl.chains.size(); i++) {
        ChainDesc c = pl.chains[i];
        const int hi = (int)before[keys[i]] - 1, lo = (int)sl.low[keys[i]];
        if (hi >= lo) {
            c.frame = (uint32_t)slot;
            runs.push_back(SessionRun{c, slot, keys[i], recon.size(), hi, lo});
        }
        c.frame = (uint32_t)k;
        recon.push_back(c);
    }
    return true;
}

int session_feed_run(icerx_session *s, BatchRun &r, const int *slot_of, const uint8_t *data, bool data_on_device, BatchOut out, int *rcs,
                     size_t *ws, size_t *hs, bool *touched)
{
    icerx_decoder *d = s->d;
    const int n = r.n, channels = d->channels, nplanes = r.pb.nplanes, sign_bit = r.pb.sign_bit;
    std::vector<PacketCandidate> mine;
    std::vector<SessionRun> runs;
    std::vector<ChainDesc> recon, upload;
    std::vector<FrameInfo> by_slot((size_t)s->n_slots);
    std::vector<uint32_t> slot_of_row((size_t)n), lowest;
    uint32_t n_fast = 0, n_ring = 0, nc = 0;        // runs [0, n_fast): wave per plane; [n_fast, n_ring): lane per plane; [n_ring, nc): threads
    size_t at = 0;
    int rc = batch_packets(r, data, data_on_device);
    if (rc != ICER_RESULT_OK) return rc;
    *touched = true;
    memset(by_slot.data(), 0, sizeof(FrameInfo) * by_slot.size());
    for (int k = 0; k < n; k++) {
        mine.clear();
        while (at < r.cands.size() && r.cands[at].frame == (uint32_t)k) mine.push_back(r.cands[at++]);
        FrameInfo &f = r.frames[k];
        slot_of_row[(size_t)k] = (uint32_t)slot_of[k];
        DecodePlan &pl = r.plans[k];
        if (!session_accept(s, k, slot_of[k], mine, pl, rcs, ws, hs, runs, recon)) { pl = DecodePlan(); continue; }      // (f.w = f.h = 0: nothing is delivered)
        (void)frame_of_plan(f, pl, d->stages);
        by_slot[(size_t)slot_of[k]] = f;
    }
    HIP_TRY(hipMemcpy(r.d_frames, r.frames.data(), sizeof(FrameInfo) * n, hipMemcpyHostToDevice));
    HIP_TRY(ensure(s->rows, sizeof(uint32_t) * n));
    HIP_TRY(hipMemcpy(s->rows.p, slot_of_row.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    // ---- the chains with new planes, in place on the state planes
    // (a slot that delivers nothing -- no samples, or a plan that stopped before its first chain -- has no chain here)
    runs.erase(std::remove_if(runs.begin(), runs.end(), [&](const SessionRun &x) { return by_slot[(size_t)x.slot].w == 0u; }), runs.end());
    if (!runs.empty()) {
        // Which kernel takes a run: the plain decode's rule (decoder_route.hpp).  The wave-per-plane kernel by load (dwant_planes),
        // for the chains it can take (takes_planes); of the others the lane-per-plane kernel those whose ring fits, by ring class on
        // the side streams, and one thread per chain what is left.  One thing is kept from before the load rule: while the planes
        // kernel is the choice by load (ICER_DEC_WAVE unset), the chains it leaves -- short packets, few and small -- stay on the
        // thread route, so a feed below the threshold takes the kernels it always took.
        const int mode = dec_wave_mode();
        uint32_t n_eligible = 0;
        for (const SessionRun &x : runs) n_eligible += x.c.fast ? 1u : 0u;
        const bool want_planes = dwant_planes(mode, d->tables.lut_ok, n_eligible, (uint32_t)d->n_cus);
        const bool want_lanes = mode != 0 && !(mode == -1 && want_planes);
        // (the dynamic LDS the resume planes kernel may take: the decoder's figure, granted to this kernel too)
        const size_t lds_limit = grant_dynamic_lds(reinterpret_cast<const void *>(decode_chains_planes_resume_kernel), resolve_planes_lds(d), &s->lds_state);
        const DRouteRule rule = {mode, (uint32_t)std::min<size_t>(lds_limit, 0xFFFFFFFFu), 0u, (uint32_t)nplanes};
        auto stream_len_of = [&](uint32_t slot) { return by_slot[(size_t)slot].stream_len; };       // (a run's chain names its slot as its frame)
        // the thread route's share goes to the back, longest first; the rest in the order and the classes of the plain decode
        const auto slow = std::stable_partition(runs.begin(), runs.end(), [&](const SessionRun &x) {
            return takes_planes(rule, x.c, stream_len_of(x.c.frame), want_planes) || (want_lanes && wave_ring_fits(ring_elems_for(x.c.w, nplanes))); });
        std::vector<SessionRun> threads(slow, runs.end());
        runs.erase(slow, runs.end());
        std::stable_sort(threads.begin(), threads.end(), [](const SessionRun &a, const SessionRun &b) { return (uint32_t)a.c.w * a.c.h > (uint32_t)b.c.w * b.c.h; });
        const BatchRoute route = route_batch_chains(runs, [](const SessionRun &x) -> const ChainDesc & { return x.c; }, stream_len_of, want_planes,
                                                    lds_limit, nplanes);
        n_fast = route.n_fast; n_ring = (uint32_t)runs.size();
        runs.insert(runs.end(), threads.begin(), threads.end());
        nc = (uint32_t)runs.size();
        for (const SessionRun &x : runs) upload.push_back(x.c);
        const DecoderTables *tables = (const DecoderTables *)d->dtables.p;
        if (n_fast < nc) {                                      // a status word per chain of the two routes that report where a chain stopped
            HIP_TRY(ensure(s->status, sizeof(uint32_t) * (nc - n_fast)));
            HIP_TRY(hipMemset(s->status.p, 0, sizeof(uint32_t) * (nc - n_fast)));
        }
        HIP_TRY(ensure(s->frames, sizeof(FrameInfo) * by_slot.size()));
        HIP_TRY(hipMemcpy(s->frames.p, by_slot.data(), sizeof(FrameInfo) * by_slot.size(), hipMemcpyHostToDevice));
        HIP_TRY(ensure(s->chains, sizeof(ChainDesc) * nc));
        HIP_TRY(hipMemcpy(s->chains.p, upload.data(), sizeof(ChainDesc) * nc, hipMemcpyHostToDevice));
        const ChainDesc *d_chains = (const ChainDesc *)s->chains.p;
        if (n_fast) {
            HIP_TRY(planes_err_begin(d));
            ICER_LAUNCH_PLANES(decode_chains_planes_resume_kernel, n_fast, route.planes_lds, (uint16_t *)s->state.p, s->frame_stride, channels, d_chains,
                               r.d_data, (const FrameInfo *)s->frames.p, tables, nplanes, sign_bit, (uint32_t *)d->err.p);
            HIP_TRY(hipGetLastError());
        }
        if (n_fast < n_ring) {
            if ((rc = ensure_side_streams(d)) != ICER_RESULT_OK) goto done;
            // (everything the null stream did so far is complete: the upload of the chains above was a blocking copy)
            uint32_t from = n_fast;
            for (int k = 0; k < kRingClasses; from = route.class_end[k++]) {
                if (route.class_end[k] == from) continue;
                ICER_LAUNCH_WAVE_ON(d->side[k], decode_chains_wave_resume_kernel, route.class_end[k] - from,
                                    route.class_elems[k] * sizeof(uint16_t) + kStateBytes, (uint16_t *)s->state.p, s->frame_stride, channels,
                                    d_chains + from, r.d_data, (const FrameInfo *)s->frames.p, tables, nplanes, sign_bit,
                                    (uint32_t *)s->status.p + (from - n_fast));
                HIP_TRY(hipGetLastError());
            }
        }
        if (n_ring < nc) {
            ICER_LAUNCH(decode_chains_resume_kernel, (nc - n_ring + 63u) / 64u, 64, plane_block_bytes(64u), (uint16_t *)s->state.p, s->frame_stride,
                        channels, d_chains + n_ring, nc - n_ring, r.d_data, (const FrameInfo *)s->frames.p, tables, nplanes, sign_bit,
                        (uint32_t *)s->status.p + (n_ring - n_fast));
            HIP_TRY(hipGetLastError());
        }
#ifndef ICER_HOST_MOCK
        if (n_fast < n_ring)
            for (hipStream_t st : d->side) HIP_TRY(hipStreamSynchronize(st));
#endif
        if (n_fast < nc) {
            lowest.resize(nc - n_fast);
            HIP_TRY(hipMemcpy(lowest.data(), s->status.p, sizeof(uint32_t) * (nc - n_fast), hipMemcpyDeviceToHost));
        }
        if (n_fast && (rc = planes_err_end(d, "a decode session")) != ICER_RESULT_OK) goto done;
        for (uint32_t i = 0; i < nc; i++) {
            const SessionRun &x = runs[i];
            int last = x.lo;                                    // the lowest plane that was started
            if (i < n_fast) s->stats[0] += x.hi + 1 < nplanes ? 1u : 0u;
            else {
                s->stats[1] += i >= n_ring ? 1u : 0u;
                const int ok = (int)lowest[i - n_fast];         // (either route: the lowest plane held or ended kOk)
                if (ok > x.lo) {                                // plane ok - 1 failed: the chain has stopped, what lay below never started
                    icerx_session::Slot &sl = s->slots[(size_t)x.slot];
                    last = ok - 1;
                    sl.low[x.key] = (uint8_t)last;
                    sl.stopped[x.key] = 1;
                    s->stats[3] += (uint64_t)(last - x.lo);
                    for (int lsb = 0; lsb < last; lsb++) recon[x.recon_at].pkt[lsb] = kNoPacket;
                }
            }
            s->stats[2] += (uint64_t)(x.hi - last + 1);
        }
    }
    // ---- the fed slots' planes into the working buffer, and from there as the plain decode
    HIP_TRY(batch_working_planes(r, out));
    ICER_LAUNCH(session_copy_kernel, r.grid_all(), 256, 0, (const uint16_t *)s->state.p, r.d_planes, s->frame_stride, channels, r.d_frames,
                (const uint32_t *)s->rows.p);
    HIP_TRY(hipGetLastError());
    r.chains.swap(recon);
    if (d->recon != 0 && !r.chains.empty()) {
        HIP_TRY(ensure(d->chains, sizeof(ChainDesc) * r.chains.size()));
        HIP_TRY(hipMemcpy(d->chains.p, r.chains.data(), sizeof(ChainDesc) * r.chains.size(), hipMemcpyHostToDevice));
    }
    rc = batch_samples(r);
    if (rc == ICER_RESULT_OK) rc = batch_results(r, out);
done:
    return rc;
}

int session_feed(icerx_session *s, int n, const int *slots, const uint8_t *data, bool data_on_device, const size_t *offsets,
                 const size_t *lens, BatchOut out, int *rcs, size_t *ws, size_t *hs)
{
    g_error.clear();
    if (!s || n < 0 || n > s->n_slots || (n && (!offsets || !lens || !rcs || !ws || !hs || !out.p))) return ICER_INVALID_INPUT;
    if (n == 0) return ICER_RESULT_OK;
    std::vector<int> slot_of((size_t)n);
    std::vector<char> seen((size_t)s->n_slots, 0);
    for (int k = 0; k < n; k++) {
        const int slot = slots ? slots[k] : k;
        if (slot < 0 || slot >= s->n_slots || seen[(size_t)slot]) return ICER_INVALID_INPUT;
        seen[(size_t)slot] = 1;
        slot_of[(size_t)k] = slot;
    }
    BatchRun r;
    bool touched = false;
    int rc = batch_open(r, s->d, n, data, offsets, lens, s->frame_stride, 0, "feeds of %zu bytes: 32-bit offsets only");
    if (rc != ICER_RESULT_OK) return rc;
    rc = session_feed_run(s, r, slot_of.data(), data, data_on_device, out, rcs, ws, hs, &touched);
    if (rc != ICER_RESULT_OK && touched) {                       // (the slots may hold half a feed: they start over)
        drain_after_error(s->d);
        for (int slot : slot_of) (void)session_reset_slot(s, slot);
    }
    return rc;
}

}  // namespace

extern "C" {

int icerx_session_create(icerx_session **out, icerx_decoder *dec, int n_slots, size_t frame_stride)
{
    g_error.clear();
    if (!out) return ICER_INVALID_INPUT;
    *out = nullptr;
    if (!dec || n_slots < 1) return ICER_INVALID_INPUT;
    if (frame_stride > 0xFFFFFFFFull) return fail("frames of %zu samples: 32-bit indices only", frame_stride);
    const size_t words = (size_t)n_slots * dec->channels * frame_stride;
    icerx_session *s = new icerx_session;
    s->d = dec; s->n_slots = n_slots; s->frame_stride = frame_stride;
    s->slots.resize((size_t)n_slots);
    for (int k = 0; k < n_slots; k++) session_clear_slot(s, k);
    if (ensure(s->state, sizeof(uint16_t) * std::max<size_t>(words, 1)) != hipSuccess || hipMemset(s->state.p, 0, sizeof(uint16_t) * words) != hipSuccess) {
        (void)hipGetLastError();
        icerx_session_destroy(s);
        return fail("a session of %d slots of %zu samples: no device memory for its state planes", n_slots, frame_stride);
    }
    *out = s;
    return ICER_RESULT_OK;
}

void icerx_session_destroy(icerx_session *s)
{
    if (!s) return;
    for (icerx_decoder::Buf *b : {&s->state, &s->frames, &s->chains, &s->status, &s->rows})
        if (b->p) (void)hipFree(b->p);
    delete s;
}

int icerx_session_reset(icerx_session *s, int slot)
{
    g_error.clear();
    if (!s || slot < -1 || slot >= s->n_slots) return ICER_INVALID_INPUT;
    for (int k = slot < 0 ? 0 : slot; k < (slot < 0 ? s->n_slots : slot + 1); k++) {
        const int rc = session_reset_slot(s, k);
        if (rc != ICER_RESULT_OK) return rc;
    }
    return ICER_RESULT_OK;
}

int icerx_session_feed_host(icerx_session *s, int n, const int *slots, const uint8_t *data, const size_t *offsets, const size_t *lens,
                            void *const *planes_out, int *rcs, size_t *ws, size_t *hs)
{
    return session_feed(s, n, slots, data, false, offsets, lens, {BatchOut::kHostPlanes, planes_out}, rcs, ws, hs);
}

int icerx_session_feed_device(icerx_session *s, int n, const int *slots, const void *d_data, const size_t *offsets, const size_t *lens,
                              void *d_out, int *rcs, size_t *ws, size_t *hs)
{
    return session_feed(s, n, slots, (const uint8_t *)d_data, true, offsets, lens, {BatchOut::kDevPlanes, d_out}, rcs, ws, hs);
}

int icerx_session_feed_device_display(icerx_session *s, int n, const int *slots, const void *d_data, const size_t *offsets,
                                      const size_t *lens, uint8_t *d_out, int *rcs, size_t *ws, size_t *hs)
{
    return session_feed(s, n, slots, (const uint8_t *)d_data, true, offsets, lens, {BatchOut::kDevDisplay, d_out}, rcs, ws, hs);
}

int icerx_session_planes_held(const icerx_session *s, int slot, int chan, int level, int subband, int segment)
{
    if (!s || slot < 0 || slot >= s->n_slots || chan < 0 || subband < 0 || segment < 0) return -2;
    const int lv = level - s->d->reduce;
    if (lv < 1 || !PacketTable::names(chan, lv, subband, segment, 0)) return -2;
    const icerx_session::Slot &sl = s->slots[(size_t)slot];
    const size_t key = PacketTable::chain_index(chan, lv, subband, segment);
    return sl.stopped[key] ? -1 : plane_bits(s->d->bits).nplanes - (int)sl.low[key];
}

int icerx_session_stats(const icerx_session *s, uint64_t out[4])
{
    if (!s || !out) return ICER_INVALID_INPUT;
    for (int i = 0; i < 4; i++) out[i] = s->stats[i];
    return ICER_RESULT_OK;
}

}  // extern "C"
