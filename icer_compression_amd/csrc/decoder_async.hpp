// decoder_async.hpp -- icerx_decode_device_async (include/icer_hip_dec.h): the batch decode of decode_batch with every step
// planned on the device and enqueued on the caller's stream.  No blocking copy, no synchronisation, no allocation: the
// caller owns the workspace (async_layout).  Included by decoder.hip after its kernels and decode_batch, whose helpers it uses.
//
//   blob       candidates over the whole blob: a bitmap of header candidates (one thread per 256 bytes), a scan of its
//              counts (per 256 groups, then one thread over those), the candidates compacted in offset order, their payload
//              CRCs (one wavefront per candidate, grid-stride over the device count).  enqueue_blob_stage, over a BlobLayout
//   frames     plan_frames_kernel, one workgroup per frame: the cursor walk (walk_frame, with decoder_dplan.hpp), the frame's
//              rc / size / FrameInfo, its chains in fixed slots
//   routing    every chain slot counted by (kernel, area bucket) for both answers of the by-load rule, the rule decided on
//              the device, then each chain placed in its kernel's list, largest area first
//   chains     persistent list-driven wrappers of the three chain kernels: wave per plane on the caller's stream, the lane-per-
//              plane ring classes on the decoder's side streams (forked and joined with events), thread per chain
//   samples    reconstruct_kernel if the decoder asks for it (decoder_recon.hpp), unsign_kernel, the inverse DWT with each frame's own size (the level loop on the host runs over `stages`),
//              finish_kernel; a wave-per-plane chain past its spin bound turns its frame's rc into ICER_FATAL_ERROR
// The blob stage and the walk are also the first two steps of a re-cut (recut.hpp), which has no copy of either.
#include "decoder_dplan.hpp"
#include "wavelet_core.hpp"

namespace {

#ifdef ICER_HOST_MOCK
constexpr uint32_t kPlanThreads = 1;               // (the mock runs a workgroup's threads one after the other: no barriers)
#define ICER_BARRIER()
#else
constexpr uint32_t kPlanThreads = 64;
#define ICER_BARRIER() __syncthreads()
#endif
constexpr uint32_t kPlanChunk = 64;                // candidates summarised per step of walk_frame
constexpr uint32_t kGroupBytes = 256, kGroupWords = kGroupBytes / 32u, kSuperGroups = 256;
#ifdef ICER_HOST_MOCK
constexpr uint32_t kGridCus = 2;                  // (the mock's persistent grids: a few workgroups, each looping)
#endif

// the head of the workspace: one call's counters (zeroed on the stream)
struct AsyncHead {
    uint32_t n_cands, n_fast, want_planes, pad;
    uint32_t start[kRouteKernels], count[kRouteKernels];
    uint32_t bucket[2][kRouteKernels][kRouteBuckets];      // chains by (planes wanted: 0 / not: 1, kernel, area bucket)
    uint32_t place[kRouteKernels][kRouteBuckets];          // next place of a bucket in the lists
};

// a workspace is carved in 256-byte steps
struct Carver {
    size_t at = 0;
    size_t take(size_t bytes) { const size_t p = at; at += (bytes + 255u) & ~(size_t)255u; return p; }
};

// what the blob stage (enqueue_blob_stage) fills and a frame walk reads: the call's head, the candidates and the buffers that
// lead to them, and every frame's packet table (tab_off / tab_bits, tab_slots entries a frame)
struct BlobLayout {
    size_t head, bitmap, gcount, scount, cands, tab_off, tab_bits;
    uint32_t groups, supers;
};
// `head`: where the caller has put the AsyncHead (the asynchronous decode keeps its frame records between it and the rest)
BlobLayout blob_layout(Carver &c, size_t head, size_t n, size_t data_bytes, size_t tab_slots)
{
    BlobLayout B;
    B.head = head;
    B.groups = (uint32_t)((data_bytes + kGroupBytes - 1u) / kGroupBytes);
    B.supers = (B.groups + kSuperGroups - 1u) / kSuperGroups;
    B.bitmap = c.take(sizeof(uint32_t) * kGroupWords * (size_t)B.groups);
    B.gcount = c.take(sizeof(uint32_t) * (size_t)B.groups);
    B.scount = c.take(sizeof(uint32_t) * (size_t)B.supers);
    B.cands = c.take(sizeof(DCandRec) * ((data_bytes + 1u) / 2u));     // (two preambles cannot overlap)
    B.tab_off = c.take(sizeof(uint32_t) * n * tab_slots);
    B.tab_bits = c.take(sizeof(uint32_t) * n * tab_slots);
    return B;
}

struct AsyncLayout {
    BlobLayout blob;
    size_t frames, ferr, chains, lists, tmp, work, pos, total;
    uint32_t chain_slots, tab_slots;
    size_t pos_words;                                       // per frame (uint8 only): odd-length interleave tables
};

DPlanGeom async_geom(const icerx_decoder *d)
{
    return DPlanGeom{(uint32_t)d->channels, (uint32_t)d->stages, d->segments, (uint32_t)(d->bits == 8 ? kPlanes8 : kPlanes),
                     (uint32_t)d->reduce};
}

// `display`: a display call (icerx_decode_device_display_async) -- its working planes live in the workspace whatever the sample
// width, as an 8-bit decoder's do
AsyncLayout async_layout(const icerx_decoder *d, int n, size_t data_bytes, size_t frame_stride, bool display = false)
{
    AsyncLayout L;
    const DPlanGeom g = async_geom(d);
    const size_t N = (size_t)n, planes_total = N * (size_t)d->channels * frame_stride;
    L.chain_slots = g.chain_slots();
    L.tab_slots = g.slots();
    // (the lines of a level are at most w + h <= frame_stride / 3 + 3 samples together when the transform runs: both sides >= 3)
    L.pos_words = d->bits == 8 ? 2u * (frame_stride / 3u + 4u) : 0u;
    Carver c;
    const size_t head = c.take(sizeof(AsyncHead));
    L.frames = c.take(sizeof(FrameInfo) * N);
    L.ferr = c.take(sizeof(uint32_t) * N);
    L.blob = blob_layout(c, head, N, data_bytes, L.tab_slots);
    L.chains = c.take(sizeof(ChainDesc) * N * L.chain_slots);
    L.lists = c.take(sizeof(uint32_t) * N * L.chain_slots);
    L.tmp = c.take(sizeof(uint16_t) * planes_total);
    L.work = c.take(d->bits == 8 || display ? sizeof(uint16_t) * planes_total : 0u);
    L.pos = c.take(sizeof(uint32_t) * N * L.pos_words);
    L.total = c.at;
    return L;
}

// ------------------------------------------------------------------------------------------ blob kernels
// one thread per group of 256 blob bytes: its 8 bitmap words of header candidates and their count
__global__ void __launch_bounds__(256)
mark_headers_kernel(const uint8_t *__restrict__ blob, uint32_t blob_len, const uint32_t *__restrict__ crc_tab,
                    uint32_t *__restrict__ bitmap, uint32_t *__restrict__ gcount, uint32_t groups)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    uint32_t total = 0;
    for (uint32_t w = 0; w < kGroupWords; w++) {
        uint32_t bits = 0;
        for (uint32_t b = 0; b < 32u; b++) {
            const uint32_t off = g * kGroupBytes + w * 32u + b;
            if (off < blob_len && dheader_at(crc_tab, blob, blob_len, off)) bits |= 1u << b;
        }
        bitmap[(size_t)g * kGroupWords + w] = bits;
        total += (uint32_t)__builtin_popcount(bits);
    }
    gcount[g] = total;
}

// one thread per 256 groups: their counts -> exclusive prefix inside the run, the run's total
__global__ void __launch_bounds__(256)
scan_groups_kernel(uint32_t *__restrict__ gcount, uint32_t groups, uint32_t *__restrict__ scount, uint32_t supers)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= supers) return;
    uint32_t sum = 0;
    const uint32_t end = (s + 1u) * kSuperGroups < groups ? (s + 1u) * kSuperGroups : groups;
    for (uint32_t g = s * kSuperGroups; g < end; g++) { const uint32_t c = gcount[g]; gcount[g] = sum; sum += c; }
    scount[s] = sum;
}

// one thread: the runs' totals -> exclusive prefix, the candidate count
__global__ void __launch_bounds__(64)
scan_supers_kernel(uint32_t *__restrict__ scount, uint32_t supers, AsyncHead *__restrict__ head)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t sum = 0;
    for (uint32_t s = 0; s < supers; s++) { const uint32_t c = scount[s]; scount[s] = sum; sum += c; }
    head->n_cands = sum;
}

// one thread per group: its candidates, in offset order, at their place
__global__ void __launch_bounds__(256)
compact_headers_kernel(const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ gcount, const uint32_t *__restrict__ scount,
                       uint32_t groups, DCandRec *__restrict__ recs)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= groups) return;
    uint32_t at = scount[g / kSuperGroups] + gcount[g];
    for (uint32_t w = 0; w < kGroupWords; w++)
        for (uint32_t bits = bitmap[(size_t)g * kGroupWords + w]; bits; bits &= bits - 1u) {
            recs[at].off = g * kGroupBytes + w * 32u + (uint32_t)__builtin_ctz(bits);
            recs[at].crc = 0;
            at++;
        }
}

// payload CRCs: one wavefront per candidate (payload_piece_crc, 64 pieces), grid-stride over the device count; a payload
// that does not fit the blob keeps 0 (it fits no frame: dplan_summary drops it before looking at the CRC)
__global__ void __launch_bounds__(256)
payload_crcs_kernel(const uint8_t *__restrict__ blob, uint32_t blob_len, const uint32_t *__restrict__ crc_tab,
                    DCandRec *__restrict__ recs, const AsyncHead *__restrict__ head)
{
    const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (blockDim.x / 64u);
    const uint32_t n = head->n_cands;
    for (uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) / 64u; i < n; i += nwaves) {
        PacketCandidate c;
        c.off = recs[i].off;
        const uint32_t bits = load_le32(blob + c.off + 16);
        c.payload_bytes = bits / 8u + ((bits % 8u) ? 1u : 0u);
        c.fits = c.payload_bytes <= blob_len - c.off - (uint32_t)kHeaderBytes;
        const uint32_t v = payload_piece_crc(crc_tab, blob, c, lane, 64u);
        if (v) atomicXor(&recs[i].crc, v);
    }
}

// ------------------------------------------------------------------------------------------ blob stage, enqueued
unsigned grid_blocks(size_t items, size_t per_block, size_t cap)
{
    return (unsigned)std::max<size_t>(1, std::min((items + per_block - 1) / per_block, cap));
}
uint32_t grid_cus(int n_cus)
{
#ifdef ICER_HOST_MOCK
    return (void)n_cus, kGridCus;
#else
    return (uint32_t)n_cus;
#endif
}

// the blob stage of a call on `st`: the head zeroed, the packet tables of the n frames emptied, the candidates of the blob
// with their payload CRCs in offset order (head->n_cands of them)
int enqueue_blob_stage(const BlobLayout &B, uint8_t *ws, size_t n, size_t tab_slots, const uint8_t *d_data, size_t data_bytes,
                       const uint32_t *crc_tab, int n_cus, hipStream_t st)
{
    int rc = ICER_RESULT_OK;
    AsyncHead *head = (AsyncHead *)(ws + B.head);
    DCandRec *recs = (DCandRec *)(ws + B.cands);
    uint32_t *bitmap = (uint32_t *)(ws + B.bitmap), *gcount = (uint32_t *)(ws + B.gcount), *scount = (uint32_t *)(ws + B.scount);
    const uint32_t blob_len = (uint32_t)data_bytes;
    HIP_TRY(hipMemsetAsync(head, 0, sizeof(AsyncHead), st));
    HIP_TRY(hipMemsetAsync(ws + B.tab_off, 0xFF, sizeof(uint32_t) * n * tab_slots, st));                // (kNoPacket)
    if (B.groups) {
        ICER_LAUNCH_ON(st, mark_headers_kernel, (B.groups + 255u) / 256u, 256, 0, d_data, blob_len, crc_tab, bitmap, gcount, B.groups);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(st, scan_groups_kernel, (B.supers + 255u) / 256u, 256, 0, gcount, B.groups, scount, B.supers);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(st, scan_supers_kernel, 1, 64, 0, scount, B.supers, head);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(st, compact_headers_kernel, (B.groups + 255u) / 256u, 256, 0, (const uint32_t *)bitmap, (const uint32_t *)gcount,
                       (const uint32_t *)scount, B.groups, recs);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(st, payload_crcs_kernel, grid_blocks((data_bytes + 1u) / 2u, 4, 8u * grid_cus(n_cus)), 256, 0, d_data, blob_len,
                       crc_tab, recs, head);
        HIP_TRY(hipGetLastError());
    }
done:
    return rc;
}

// ------------------------------------------------------------------------------------------ per-frame walk
// What a walk notes besides its DWalk.  other_size and max_level are the re-cut's (recut.hpp): an accepted packet had another
// image size than the w_in x h_in expected; the largest decomp_level of an accepted packet (0: none).  Accepted: a packet of
// the frame at or behind the cursor (end != 0 && rel >= cursor), the condition under which dplan_accept moves the cursor.
struct WalkNotes { uint32_t inside, other_size, max_level; };
// its dynamic LDS: kPlanChunk DCand, the final DWalk, then for each candidate of the chunk the cursor it met (a word) and its
// decomp_level (a byte)
constexpr uint32_t kWalkCursorAt = kPlanChunk * sizeof(DCand) + sizeof(DWalk), kWalkLevelsAt = kWalkCursorAt + kPlanChunk * sizeof(uint32_t);
constexpr uint32_t kWalkLds = kWalkLevelsAt + kPlanChunk;

// The decoder's cursor walk of frame [off, off + len) into its packet table `to` / `tb`, called by the WHOLE workgroup, of any
// size.  Per kPlanChunk candidates: the threads summarise them into LDS; thread 0 runs the cursor rule over the summaries,
// the one serial step, which takes nothing else along but a store of the cursor each candidate met; the threads then look at
// their own candidates for the notes.  Returns the final DWalk (in: w_in, h_in) and fills *notes, the same in every
// thread.  A frame outside the blob (notes->inside = 0) is not walked.  Which barriers a workgroup meets depends on the
// frame alone, never on the thread, so all threads reach every one of them.
ICER_DEV DWalk walk_frame(uint8_t *lds, const uint8_t *blob, uint32_t blob_len, uint64_t off, uint64_t len, const DCandRec *recs,
                          const AsyncHead *head, const DPlanGeom &geom, uint64_t w_in, uint64_t h_in, uint32_t *to, uint32_t *tb,
                          WalkNotes *notes)
{
    DCand *chunk = reinterpret_cast<DCand *>(lds);
    DWalk *shared_walk = reinterpret_cast<DWalk *>(lds + kPlanChunk * sizeof(DCand));
    uint32_t *cursor_at = reinterpret_cast<uint32_t *>(lds + kWalkCursorAt);
    uint8_t *levels = lds + kWalkLevelsAt;
    const uint32_t tid = threadIdx.x;
    const bool inside = off <= blob_len && len <= blob_len - off;
    DWalk s;
    dwalk_init(&s, w_in, h_in);
    uint32_t other = 0, top = 0;                               // over the accepted candidates that this thread summarised
    if (inside) {
        const uint32_t nc = head->n_cands, first = dlower_bound(recs, nc, (uint32_t)off), last = dlower_bound(recs, nc, (uint32_t)(off + len));
        for (uint32_t at = first; at < last; at += kPlanChunk) {
            const uint32_t m = last - at < kPlanChunk ? last - at : kPlanChunk;
            for (uint32_t t = tid; t < m; t += blockDim.x) {
                chunk[t] = dplan_summary(geom, blob, (uint32_t)off, (uint32_t)len, recs[at + t]);
                levels[t] = chunk[t].end != 0 ? blob[recs[at + t].off + 4u] : (uint8_t)0;
            }
            ICER_BARRIER();
            if (tid == 0)
                for (uint32_t t = 0; t < m; t++) {
                    cursor_at[t] = s.cursor;
                    dplan_accept(&s, chunk[t], to, tb);
                }
            ICER_BARRIER();
            // (candidate t is summarised and looked at by the same thread, and its cursor is written again behind the next barrier)
            for (uint32_t t = tid; t < m; t += blockDim.x)
                if (chunk[t].end != 0 && chunk[t].rel >= cursor_at[t]) {
                    if (chunk[t].w != w_in || chunk[t].h != h_in) other = 1;
                    if (levels[t] > top) top = levels[t];
                }
        }
    }
    // every thread's part through the chunk's LDS, free now: a word per thread that can have summarised a candidate
    static_assert(sizeof(uint32_t) <= sizeof(DCand), "a word per thread fits the chunk");
    uint32_t *part = reinterpret_cast<uint32_t *>(chunk);
    const uint32_t parts = blockDim.x < kPlanChunk ? blockDim.x : kPlanChunk;
    ICER_BARRIER();
    if (tid < parts) part[tid] = top | other << 31;
    if (tid == 0) *shared_walk = s;
    ICER_BARRIER();
    notes->inside = inside ? 1u : 0u; notes->other_size = 0; notes->max_level = 0;
    for (uint32_t i = 0; i < parts; i++) {
        const uint32_t v = part[i], lv = v & 0x7FFFFFFFu;
        notes->other_size |= v >> 31;
        if (lv > notes->max_level) notes->max_level = lv;
    }
    return *shared_walk;
}

// ------------------------------------------------------------------------------------------ per-frame plan
// one workgroup per frame.  Frame k = blob bytes [off, off + len), off = offsets[k] or k * stream_stride; a frame outside
// the blob gets ICER_INVALID_INPUT and no chains.  After the walk every thread builds chain slots.  Writes rcs / ws / hs
// (ws / hs: in = the values kept when the frame holds no valid packet), the FrameInfo and the frame's chain slots (kNoChain
// where plan_decode has none).
__global__ void __launch_bounds__(64)
plan_frames_kernel(const uint8_t *__restrict__ blob, uint32_t blob_len, const uint64_t *__restrict__ offsets, uint64_t stream_stride,
                   const uint64_t *__restrict__ lens, const DCandRec *__restrict__ recs, const AsyncHead *__restrict__ head,
                   DPlanGeom geom, uint64_t bufsize, uint32_t *__restrict__ tab_off, uint32_t *__restrict__ tab_bits,
                   ChainDesc *__restrict__ chains, FrameInfo *__restrict__ frames, int32_t *__restrict__ rcs,
                   uint64_t *__restrict__ ws, uint64_t *__restrict__ hs)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // kWalkLds
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const uint64_t off = offsets ? offsets[k] : (uint64_t)k * stream_stride, len = lens[k];
    uint32_t *to = tab_off + (size_t)k * geom.slots(), *tb = tab_bits + (size_t)k * geom.slots();
    ChainDesc *mine = chains + (size_t)k * geom.chain_slots();
    WalkNotes notes;
    const DWalk s = walk_frame(lds, blob, blob_len, off, len, recs, head, geom, ws[k], hs[k], to, tb, &notes);
    if (!notes.inside) {
        if (tid == 0) {
            const FrameInfo f = {};
            frames[k] = f;
            rcs[k] = kInvalidInput;
        }
        for (uint32_t j = tid; j < geom.chain_slots(); j += blockDim.x) mine[j].frame = kNoChain;
        return;
    }
    const DPlanResult res = dplan_finish(geom, s, bufsize);
    if (tid == 0) {
        FrameInfo f;
        f.stream_off = (uint32_t)off; f.stream_len = (uint32_t)len;
        f.w = res.runs ? (uint32_t)s.w : 0u;
        f.h = res.runs ? (uint32_t)s.h : 0u;
        f.ll_w = (uint32_t)((s.w + ((uint64_t(1) << geom.stages) - 1)) >> geom.stages);
        f.ll_h = (uint32_t)((s.h + ((uint64_t(1) << geom.stages) - 1)) >> geom.stages);
        for (int c = 0; c < 3; c++) f.mean[c] = s.mean[c];
        f.mean[3] = 0;
        f.transform = res.transform;
        frames[k] = f;
        rcs[k] = res.rc; ws[k] = s.w; hs[k] = s.h;
    }
    for (uint32_t j = tid; j < geom.chain_slots(); j += blockDim.x) {
        ChainDesc c;
        if (dplan_chain(geom, s, res, to, tb, j, k, &c)) mine[j] = c;
        else mine[j].frame = kNoChain;
    }
}

// ------------------------------------------------------------------------------------------ routing
__global__ void __launch_bounds__(256)
route_count_kernel(const ChainDesc *__restrict__ chains, uint32_t slots, const FrameInfo *__restrict__ frames, DRouteRule rule,
                   AsyncHead *__restrict__ head)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += gridDim.x * blockDim.x) {
        const ChainDesc &c = chains[i];
        if (c.frame == kNoChain) continue;
        const uint32_t len = frames[c.frame].stream_len;
        const int b = droute_bucket(c);
        atomicAdd(&head->bucket[0][droute(rule, c, len, true)][b], 1u);
        atomicAdd(&head->bucket[1][droute(rule, c, len, false)][b], 1u);
        if (c.fast) atomicAdd(&head->n_fast, 1u);
    }
}

// one thread: the by-load rule, then where each (kernel, bucket) starts in the lists
__global__ void __launch_bounds__(64)
route_scan_kernel(AsyncHead *__restrict__ head, int mode, uint32_t lut_ok, uint32_t n_cus)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t want = dwant_planes(mode, lut_ok, head->n_fast, n_cus) ? 1u : 0u;
    head->want_planes = want;
    uint32_t at = 0;
    for (int k = 0; k < kRouteKernels; k++) {
        head->start[k] = at;
        for (int b = 0; b < kRouteBuckets; b++) { head->place[k][b] = at; at += head->bucket[want ? 0 : 1][k][b]; }
        head->count[k] = at - head->start[k];
    }
}

__global__ void __launch_bounds__(256)
route_place_kernel(const ChainDesc *__restrict__ chains, uint32_t slots, const FrameInfo *__restrict__ frames, DRouteRule rule,
                   AsyncHead *__restrict__ head, uint32_t *__restrict__ lists)
{
    const bool want = head->want_planes != 0u;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += gridDim.x * blockDim.x) {
        const ChainDesc &c = chains[i];
        if (c.frame == kNoChain) continue;
        const int k = droute(rule, c, frames[c.frame].stream_len, want);
        lists[atomicAdd(&head->place[k][droute_bucket(c)], 1u)] = i;
    }
}

// ------------------------------------------------------------------------------------------ chain kernels, list-driven
// (the bodies of decode_chains_planes_kernel / _wave_kernel / decode_chains_kernel; each workgroup loops over its kernel's
// list, which the host does not know the length of)
__global__ void __launch_bounds__(64 * kPwWaves)
planes_list_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels, const ChainDesc *__restrict__ chains,
                   const uint32_t *__restrict__ lists, const AsyncHead *__restrict__ head, const uint8_t *__restrict__ data,
                   const FrameInfo *__restrict__ frames, const DecoderTables *__restrict__ tables, int nplanes, int sign_bit,
                   uint32_t *__restrict__ ferr)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);
    const uint32_t n = head->count[0], start = head->start[0];
    const uint32_t wave = pw_workgroup_wave();
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const ChainDesc &c = chains[lists[start + i]];
        const FrameInfo f = frames[c.frame];
        ICER_BARRIER();                                      // (every wave is done with the previous chain's LDS)
        pw_workgroup_clear(lds, c, nplanes);
        (void)pw_run_chain(lds, wave, c, nplanes, sign_bit, chain_plane(planes, c, channels, frame_stride), f.w,
                           data + f.stream_off, f.stream_len, tables, ferr + c.frame);
    }
}

__global__ void __launch_bounds__(64)
wave_list_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels, const ChainDesc *__restrict__ chains,
                 const uint32_t *__restrict__ lists, const AsyncHead *__restrict__ head, int list, const uint8_t *__restrict__ data,
                 const FrameInfo *__restrict__ frames, const DecoderTables *__restrict__ tables, int nplanes, int sign_bit)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);
    ICER_LDS_TABLES(lt, tables);
    const uint32_t n = head->count[list], start = head->start[list];
    uint16_t *ring = reinterpret_cast<uint16_t *>(lds + kStateBytes);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const ChainDesc c = chains[lists[start + i]];
        const FrameInfo f = frames[c.frame];
        ICER_BARRIER();
        decode_chain_wave(ring, chain_plane(planes, c, channels, frame_stride), f.w, c, (int)c.subband,
                          data + f.stream_off, f.stream_len, lt, nplanes, sign_bit, nullptr, lds);
    }
}

__global__ void __launch_bounds__(64)
thread_list_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels, const ChainDesc *__restrict__ chains,
                   const uint32_t *__restrict__ lists, const AsyncHead *__restrict__ head, const uint8_t *__restrict__ data,
                   const FrameInfo *__restrict__ frames, const DecoderTables *__restrict__ tables, int nplanes, int sign_bit)
{
    ICER_DYNAMIC_LDS(uint8_t, state);
    ICER_LDS_TABLES(lt, tables);
    const uint32_t n = head->count[kRouteThread], start = head->start[kRouteThread];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const ChainDesc c = chains[lists[start + i]];
        const FrameInfo f = frames[c.frame];
        PlaneDecoder job;
        plane_attach_columns(job, state, 64u, threadIdx.x);
        decode_chain(job, chain_plane(planes, c, channels, frame_stride), f.w, c, (int)c.subband,
                     data + f.stream_off, f.stream_len, lt, nplanes, sign_bit);
    }
}

// ------------------------------------------------------------------------------------------ inverse DWT, per-frame sizes
// level `it` (1 = deepest) of every frame that is transformed: region dim_low(w, stages - it) x dim_low(h, stages - it).
struct LevelRegion { uint32_t cw, ch; bool on; };
ICER_HD LevelRegion level_region(const FrameInfo &f, int stages, int it)
{
    LevelRegion r;
    r.on = f.transform && f.ll_w >= 3u && f.ll_h >= 3u;
    const int s = stages - it;
    r.cw = (uint32_t)(((uint64_t)f.w + ((uint64_t(1) << s) - 1)) >> s);
    r.ch = (uint32_t)(((uint64_t)f.h + ((uint64_t(1) << s) - 1)) >> s);
    return r;
}
// uint8: position tables of a level's odd line lengths, [columns | scratch | rows | scratch] per frame; one thread per table
__global__ void __launch_bounds__(64)
level_positions_kernel(const FrameInfo *__restrict__ frames, uint32_t n, int stages, int it, uint32_t *__restrict__ pos, size_t pos_words)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < 2u * n; i += gridDim.x * blockDim.x) {
        const LevelRegion r = level_region(frames[i / 2u], stages, it);
        const bool rows = (i & 1u) != 0;
        const uint32_t len = rows ? r.cw : r.ch;
        if (!r.on || !(len & 1u)) continue;
        uint32_t *t = pos + (size_t)(i / 2u) * pos_words + (rows ? 2u * r.ch : 0u);
        wl_interleave_positions_u8(len, t + len, t);
    }
}
ICER_HD DPos level_pos(const uint32_t *pos, size_t pos_words, uint32_t frame, const LevelRegion &r, bool rows, int bits)
{
    const uint32_t n = rows ? r.cw : r.ch;
    DPos p;
    p.nl = (n + 1u) / 2u;
    p.tab = (bits == 8 && (n & 1u)) ? pos + (size_t)frame * pos_words + (rows ? 2u * r.ch : 0u) : nullptr;
    return p;
}

// filter A (idwt_pair_at): one thread per output pair, grid-stride; grid = (x, frames * channels)
__global__ void __launch_bounds__(256)
idwt_pairs_frames_kernel(const int16_t *__restrict__ src, int16_t *__restrict__ dst, size_t frame_stride, int channels,
                         const FrameInfo *__restrict__ frames, int stages, int it, FilterTaps taps, int bits,
                         const uint32_t *__restrict__ pos, size_t pos_words, bool rows)
{
    const uint32_t frame = blockIdx.y / (unsigned)channels;
    const FrameInfo f = frames[frame];
    const LevelRegion r = level_region(f, stages, it);
    if (!r.on) return;
    const uint32_t n = rows ? r.cw : r.ch, nl = (n + 1u) / 2u, lines = rows ? r.ch : r.cw;
    const DPos p = level_pos(pos, pos_words, frame, r, rows, bits);
    const size_t base = (size_t)blockIdx.y * frame_stride, total = (size_t)lines * nl;
    const size_t stride = rows ? 1 : f.w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        // (consecutive threads along a row of the image in both passes)
        const uint32_t line = rows ? (uint32_t)(i / nl) : (uint32_t)(i % r.cw), k = rows ? (uint32_t)(i % nl) : (uint32_t)(i / r.cw);
        const size_t at = base + (rows ? (size_t)line * f.w : (size_t)line);
        idwt_pair_at(src + at, dst + at, n, stride, k, taps, bits, p);
    }
}

// other filters (idwt_line_at): one thread per line, grid-stride
__global__ void __launch_bounds__(64)
idwt_lines_frames_kernel(const int16_t *__restrict__ src, int16_t *__restrict__ dst, size_t frame_stride, int channels,
                         const FrameInfo *__restrict__ frames, int stages, int it, FilterTaps taps, int bits,
                         const uint32_t *__restrict__ pos, size_t pos_words, bool rows)
{
    const uint32_t frame = blockIdx.y / (unsigned)channels;
    const FrameInfo f = frames[frame];
    const LevelRegion r = level_region(f, stages, it);
    if (!r.on) return;
    const DPos p = level_pos(pos, pos_words, frame, r, rows, bits);
    const size_t base = (size_t)blockIdx.y * frame_stride;
    const uint32_t lines = rows ? r.ch : r.cw;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < lines; i += gridDim.x * blockDim.x) {
        if (rows) idwt_line_at(src + base + (size_t)i * f.w, dst + base + (size_t)i * f.w, r.cw, 1, taps, bits, p);
        else idwt_line_at(src + base + i, dst + base + i, r.ch, f.w, taps, bits, p);
    }
}

// a wave-per-plane chain that gave up on its spin bound: its frame fails
__global__ void __launch_bounds__(256)
fatal_frames_kernel(const uint32_t *__restrict__ ferr, int32_t *__restrict__ rcs, uint32_t n)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && ferr[k]) rcs[k] = ICER_FATAL_ERROR;
}

// ------------------------------------------------------------------------------------------ host side
int decode_async(icerx_decoder *d, int n, const uint8_t *d_data, size_t data_bytes, const uint64_t *d_offsets, size_t stream_stride,
                 const uint64_t *d_lens, void *d_out, size_t frame_stride, int32_t *d_rcs, uint64_t *d_ws, uint64_t *d_hs,
                 void *workspace, size_t workspace_bytes, hipStream_t st, uint8_t *d_display = nullptr, const WindowCall *win = nullptr)
{
    // (d_display: a display call -- d_out is null, the images go to d_display through display_finish_kernel)
    // (win: a window decode, decoder_window.hpp -- the working planes, win->full_stride samples each, live in the workspace;
    // d_out / d_display take the windows, of at most frame_stride samples)
    g_error.clear();
    if (!d || n < 0) return ICER_INVALID_INPUT;
    if (n == 0) return ICER_RESULT_OK;
    if (!d_lens || (!d_out && !d_display) || !d_rcs || !d_ws || !d_hs || !workspace || (data_bytes && !d_data)) return ICER_INVALID_INPUT;
    if (win && (!win->d_windows || !win->d_info)) return ICER_INVALID_INPUT;
    const size_t out_stride = frame_stride;
    if (win) {
        if (out_stride > 0xFFFFFFFFull) return fail("windows of %zu samples: 32-bit indices only", out_stride);
        frame_stride = win->full_stride;                     // (from here on: the stride of the working planes)
    }
    if (data_bytes >= 0xFFFFFFFFull - 64u) return fail("batch of %zu stream bytes: 32-bit offsets only", data_bytes);
    if (frame_stride > 0xFFFFFFFFull) return fail("frames of %zu samples: 32-bit indices only", frame_stride);
    const AsyncLayout L = async_layout(d, n, data_bytes, frame_stride, d_display != nullptr || win != nullptr);
    if (workspace_bytes < L.total + (win ? window_geom_bytes(n) : 0u)) return ICER_INVALID_INPUT;
    int rc = ICER_RESULT_OK;
    const int channels = d->channels, bits = d->bits, stages = d->stages;
    const int nplanes = plane_bits(bits).nplanes, sign_bit = plane_bits(bits).sign_bit;
    const int recon = d->recon;
    const DPlanGeom geom = async_geom(d);
    uint8_t *ws = (uint8_t *)workspace;
    AsyncHead *head = (AsyncHead *)(ws + L.blob.head);
    FrameInfo *frames = (FrameInfo *)(ws + L.frames);
    uint32_t *ferr = (uint32_t *)(ws + L.ferr);
    DCandRec *recs = (DCandRec *)(ws + L.blob.cands);
    ChainDesc *chains = (ChainDesc *)(ws + L.chains);
    uint32_t *lists = (uint32_t *)(ws + L.lists);
    uint32_t *pos = (uint32_t *)(ws + L.pos);
    const uint32_t *crc_tab = (const uint32_t *)d->crc.p;
    const DecoderTables *tables = (const DecoderTables *)d->dtables.p;
    const uint32_t blob_len = (uint32_t)data_bytes, slots = (uint32_t)n * L.chain_slots;
    const size_t planes_total = (size_t)n * channels * frame_stride;
    uint16_t *planes = bits == 16 && !d_display && !win ? (uint16_t *)d_out : (uint16_t *)(ws + L.work);
    WinGeom *win_geoms = (WinGeom *)(ws + L.total);           // (a window decode: behind everything else)
    const uint32_t cus = grid_cus(d->n_cus);
    const auto grid = grid_blocks;

    // which kernel decodes a chain: decode_batch's rule (decoder_route.hpp), decided on the device (ICER_DEC_WAVE read per call, as there)
    DRouteRule rule;
    {
        rule.mode = dec_wave_mode();
        rule.nplanes = (uint32_t)nplanes;
        rule.ring_elems_max = (uint32_t)((65536u - sizeof(DecoderTables) - 256u - kStateBytes) / sizeof(uint16_t));
        // (the list-driven planes kernel asks for the same grant; refused, it keeps what a launch gets without asking)
        rule.planes_lds_limit = (uint32_t)grant_dynamic_lds(reinterpret_cast<const void *>(planes_list_kernel), resolve_planes_lds(d), &d->async_lds_state);
    }

    if ((rc = ensure_side_streams(d)) != ICER_RESULT_OK) return rc;
    if (!d->events_ok) {
        bool made = hipEventCreateWithFlags(&d->fork, hipEventDisableTiming) == hipSuccess;
        for (hipEvent_t &e : d->join) made = made && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (!made) {
            if (d->fork) (void)hipEventDestroy(d->fork);
            for (hipEvent_t &e : d->join) { if (e) (void)hipEventDestroy(e); e = nullptr; }
            d->fork = nullptr;
            (void)hipGetLastError();
            return fail("the decoder could not create its events");
        }
        d->events_ok = true;
    }

    // 1. candidates over the blob
    HIP_TRY(hipMemsetAsync(ferr, 0, sizeof(uint32_t) * n, st));
    if ((rc = enqueue_blob_stage(L.blob, ws, (size_t)n, L.tab_slots, d_data, data_bytes, crc_tab, d->n_cus, st)) != ICER_RESULT_OK) goto done;

    // 2. plans
    ICER_LAUNCH_ON(st, plan_frames_kernel, (unsigned)n, kPlanThreads, kWalkLds, d_data, blob_len, d_offsets, (uint64_t)stream_stride,
                   d_lens, recs, head, geom, (uint64_t)frame_stride, (uint32_t *)(ws + L.blob.tab_off), (uint32_t *)(ws + L.blob.tab_bits),
                   chains, frames, d_rcs, d_ws, d_hs);
    HIP_TRY(hipGetLastError());
    if (win) {                                               // the chains the windows do not depend on leave their slots
        const FilterTaps taps = filter_taps(d->filt);
        ICER_LAUNCH_ON(st, window_frames_kernel, (unsigned)n, kPlanThreads, 0, win->d_windows, geom, (uint64_t)out_stride,
                       taps.be == 0 && taps.am1 == 0, bits, chains, frames, d_rcs, win_geoms, win->d_info);
        HIP_TRY(hipGetLastError());
    }
    if (planes_total == 0) goto done;

    // 3. bit planes
    HIP_TRY(hipMemsetAsync(planes, 0, sizeof(uint16_t) * planes_total, st));
    if (slots) {
        ICER_LAUNCH_ON(st, route_count_kernel, grid(slots, 256, 4u * cus), 256, 0, chains, slots, frames, rule, head);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(st, route_scan_kernel, 1, 64, 0, head, rule.mode, d->tables.lut_ok, (uint32_t)d->n_cus);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(st, route_place_kernel, grid(slots, 256, 4u * cus), 256, 0, chains, slots, frames, rule, head, lists);
        HIP_TRY(hipGetLastError());
        // the lane-per-plane ring classes side by side on the side streams, forked from `st` and joined back to it
        HIP_TRY(hipEventRecord(d->fork, st));
        for (int k = 0; k < kRouteClasses && rule.mode != 0; k++) {
#ifdef ICER_HOST_MOCK
            hipStream_t side = st;
#else
            hipStream_t side = d->side[k];
#endif
            HIP_TRY(hipStreamWaitEvent(side, d->fork, 0));
            const size_t lds = (size_t)(rule.ring_elems_max >> k) * sizeof(uint16_t) + kStateBytes;
            ICER_LAUNCH_WAVE_ON(side, wave_list_kernel, std::min<uint32_t>(slots, (2u << k) * cus), lds, planes, frame_stride, channels,
                                chains, lists, head, 1 + k, d_data, frames, tables, nplanes, sign_bit);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(d->join[k], side));
        }
        if (rule.mode != 1 && rule.mode != 0) {
            ICER_LAUNCH_PLANES_ON(st, planes_list_kernel, std::min<uint32_t>(slots, cus), rule.planes_lds_limit, planes, frame_stride,
                                  channels, chains, lists, head, d_data, frames, tables, nplanes, sign_bit, ferr);
            HIP_TRY(hipGetLastError());
        }
        ICER_LAUNCH_ON(st, thread_list_kernel, grid(slots, 64, 4u * cus), 64, plane_block_bytes(64u), planes, frame_stride, channels,
                       chains, lists, head, d_data, frames, tables, nplanes, sign_bit);
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < kRouteClasses && rule.mode != 0; k++) HIP_TRY(hipStreamWaitEvent(st, d->join[k], 0));
    }

    // 4. samples
    if (win) {
        rc = enqueue_window_samples(d, n, planes, (int16_t *)(ws + L.tmp), frame_stride, frames, win_geoms, pos, chains, slots, recon,
                                    d_display ? (void *)d_display : d_out, out_stride, d_display != nullptr, frame_stride, st);
        if (rc != ICER_RESULT_OK) goto done;
        ICER_LAUNCH_ON(st, fatal_frames_kernel, ((unsigned)n + 255u) / 256u, 256, 0, ferr, d_rcs, (uint32_t)n);
        HIP_TRY(hipGetLastError());
    } else {
        const dim3 grid_all((unsigned)((frame_stride + 255u) / 256u), (unsigned)(n * channels));
        if (recon != 0 && slots) {                           // (behind the joins: every chain kernel is complete)
            ICER_LAUNCH_ON(st, reconstruct_kernel, dim3(slots, kReconParts), kReconThreads, 0, planes, frame_stride, channels,
                           (const ChainDesc *)chains, slots, (const FrameInfo *)frames, (uint32_t)n, nplanes, sign_bit, recon);
            HIP_TRY(hipGetLastError());
        }
        ICER_LAUNCH_ON(st, unsign_kernel, grid_all, 256, 0, planes, frame_stride, channels, frames, sign_bit, bits);
        HIP_TRY(hipGetLastError());
        const FilterTaps taps = filter_taps(d->filt);
        const bool pairwise = taps.be == 0 && taps.am1 == 0;
        int16_t *tmp = (int16_t *)(ws + L.tmp);
        const unsigned per_frame = std::max(1u, 8u * cus / (unsigned)(n * channels));
        for (int it = 1; it <= stages; it++) {
            if (bits == 8) {
                ICER_LAUNCH_ON(st, level_positions_kernel, grid(2u * (size_t)n, 64, 4u * cus), 64, 0, frames, (uint32_t)n, stages, it, pos,
                               L.pos_words);
                HIP_TRY(hipGetLastError());
            }
            if (pairwise) {
                const dim3 g(grid(frame_stride / 2u + 1u, 256, per_frame), (unsigned)(n * channels));
                ICER_LAUNCH_ON(st, idwt_pairs_frames_kernel, g, 256, 0, (const int16_t *)planes, tmp, frame_stride, channels, frames, stages,
                               it, taps, bits, pos, L.pos_words, false);
                HIP_TRY(hipGetLastError());
                ICER_LAUNCH_ON(st, idwt_pairs_frames_kernel, g, 256, 0, (const int16_t *)tmp, (int16_t *)planes, frame_stride, channels,
                               frames, stages, it, taps, bits, pos, L.pos_words, true);
                HIP_TRY(hipGetLastError());
            } else {
                const dim3 g(grid(frame_stride / 3u + 4u, 64, 4u * per_frame), (unsigned)(n * channels));
                ICER_LAUNCH_ON(st, idwt_lines_frames_kernel, g, 64, 0, (const int16_t *)planes, tmp, frame_stride, channels, frames, stages,
                               it, taps, bits, pos, L.pos_words, false);
                HIP_TRY(hipGetLastError());
                ICER_LAUNCH_ON(st, idwt_lines_frames_kernel, g, 64, 0, (const int16_t *)tmp, (int16_t *)planes, frame_stride, channels,
                               frames, stages, it, taps, bits, pos, L.pos_words, true);
                HIP_TRY(hipGetLastError());
            }
        }
        if (d_display)
            ICER_LAUNCH_ON(st, display_finish_kernel, dim3((unsigned)(((frame_stride + 3u) / 4u + 255u) / 256u), (unsigned)n), 256, 0, planes,
                           frame_stride, channels, frames, bits, d_display);
        else
            ICER_LAUNCH_ON(st, finish_kernel, grid_all, 256, 0, planes, frame_stride, channels, frames, bits == 8 ? (uint8_t *)d_out : nullptr);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(st, fatal_frames_kernel, ((unsigned)n + 255u) / 256u, 256, 0, ferr, d_rcs, (uint32_t)n);
        HIP_TRY(hipGetLastError());
    }
done:
    return rc;
}

}  // namespace
