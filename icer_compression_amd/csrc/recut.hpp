// recut.hpp -- icerx_recut_device_async and icerx_recut_device_cuts_async (include/icer_hip_dec.h): stored streams ("masters")
// re-cut on the device, without the pixels and without re-coding.  A cut is (reduce r, quota): the master's derived stream at
// 1/2^r size, cut at that byte quota; the byte-quota call is the call whose every reduce is 0, in a smaller workspace.
// Included by decoder.hip after decoder_async.hpp, whose blob stage and frame walk are the first two steps here as well.
//
//   blob       enqueue_blob_stage: the candidate kernels of the asynchronous decode over the whole blob
//   frames     recut_plan_kernel, one workgroup per frame: the decoder's cursor walk (walk_frame) into the frame's packet
//              table, once; the units' bit counts of every geometry in use through that geometry's unit -> table slot map
//              (recut_core.hpp); then one wavefront per cut: the quota walk of the rate ladder (scan_ladder_wave) with the
//              tables of the geometry at 1/2^r size -> final offsets, size, return code
//   packets    recut_gather_kernel, one workgroup per (unit of the master, frame): the payload copied as it is to every cut
//              that keeps the packet (copy_unit_recut), the 28 header bytes written per cut (recut_cut_header; r = 0: a copy)
// Everything is enqueued on the caller's stream; the caller owns the workspace (recut_layout).
//
// What these two calls, the ROI call below, the two of recut_quality.hpp and (the first two) combine.hpp share is written once:
//   RecutMasters       where the masters lie and their packet tables go, by value with the launches: frame k's offset and rows
//   recut_walk         walk_frame and recut_frame_status: a frame's RecutFrameHead {status, max_level}
//   recut_frame_stage  recut_walk of frame k, then recut_unit_bits of every geometry in use: how every frame kernel starts
//   RecutWork          the cuts' part of the workspace: a frame's bit counts, a cut's offset row (cut_row, recut_row_by_master)
//   RecutCall, RecutRun   a call as its entry point hands it on, and what every driver derives of it.  A driver is the checks
//                      that are only its own, recut_check, recut_begin (workspace size, carving, blob stage), its own launches,
//                      and recut_finish (the gather).
//
// icerx_recut_device_roi_async: a cut is (reduce r, quota, ROI shift), the frames' rectangles lie in device memory.  The blob
// stage and the gather are the ones above; between them three launches stand in recut_plan_kernel's place, each as wide as
// its own work ("Region of interest from stored masters"):
//   frames     recut_roi_frame_kernel, one workgroup per frame: recut_frame_stage; the frame's rectangle clipped to the full
//              frame, once
//   ranks      recut_roi_rank_kernel, one workgroup per (frame, distinct (reduce, shift) of the call): the four roi_*_wave
//              phases of roi_core.hpp over the unit table and the priorities of the geometry at 1/2^r size, with the
//              rectangle scaled to it -> rank, order and the foreground count
//   cuts       recut_roi_scan_kernel, one wavefront per (frame, cut): scan_roi_wave along that order -> final offsets (for
//              r > 0 turned into the order of the master's units), size, return code, K
#include "recut_core.hpp"
#include "roi_core.hpp"

#ifdef ICER_WAVE_EMU
unsigned long long g_emu_chunks[4] = {0, 0, 0, 0};       // (coder_core.hpp's path counters of the CPU builds: unused here, defined by every emu build)
#endif

struct icerx_recutter {
    int device = 0;
    uint64_t w = 0, h = 0;
    DPlanGeom geom{};
    int n_cus = 256;
    std::vector<void *> owned;                        // every device table below, as recut_upload allocated it: the named pointers are views
    void *crc = nullptr;                              // CRC-32 table
    // device tables of the geometry at 1/2^r size, r = 0 .. max_reduce (0 unless icerx_recutter_create_reduced), uploaded once
    // and built by the planner on that geometry: table slot of every unit and the D7 final order (Plan::units order), the unit
    // table itself (scan_ladder_wave reads cap_is_bound of the unit at the cut: 0 here), and for r > 0 full_to_cut[u]: the unit
    // there that unit u of the full geometry stands for (kNoPacket: none)
    int max_reduce = 0;
    struct Reduced {
        uint32_t n_units = 0;
        void *unit_slot = nullptr, *final_order = nullptr, *units = nullptr, *full_to_cut = nullptr;
        void *prio = nullptr;                         // the priority of every unit's packet (roi_priorities): the ROI call's
    } red[kRecutMaxReduce + 1];
    uint32_t units_total = 0;                         // red[0 .. max_reduce].n_units together
    // a quality recutter (icerx_recutter_create_quality, recut_quality.hpp): the filter the masters were made with, and per
    // geometry what prepare_target of the encoder library gives an encoder of it -- every family's weight, channel and LL term --
    // and for r > 0 fam_map[g]: the family of the master that family g of that geometry is.  fam_cap: per family of the
    // master, the most its E[.][P] can be (coefficients x max_mag^2).  filt < 0: a plain recutter, none of this.
    int filt = -1;
    struct Quality {
        uint32_t n_families = 0;
        void *weight = nullptr, *chan = nullptr, *ll_term = nullptr, *fam_map = nullptr;
    } qual[kRecutMaxReduce + 1];
    void *fam_cap = nullptr;
    uint32_t families_total = 0;                      // qual[0 .. max_reduce].n_families together
};

namespace {

// the tables of a quality recutter on the host: built and checked before anything is allocated (recut_quality.hpp)
struct RecutQualityHost {
    std::vector<uint32_t> weight[kRecutMaxReduce + 1], chan[kRecutMaxReduce + 1], fam_map[kRecutMaxReduce + 1];
    std::vector<unsigned long long> ll_term[kRecutMaxReduce + 1], fam_cap;
};
int recut_quality_build(const std::vector<Plan> &plans, const DPlanGeom &geom, int filt, int sample_bits, RecutQualityHost *q);
int recut_quality_upload(icerx_recutter *r, const RecutQualityHost &q);

#ifdef ICER_HOST_MOCK
constexpr uint32_t kRecutPlanThreads = 1, kRecutGatherThreads = 3;    // (the mock runs a workgroup's threads one after the other)
#else
constexpr uint32_t kRecutPlanThreads = 256, kRecutGatherThreads = 256;
#endif
constexpr int kRecutMaxFrames = 65535;            // (frames are the y dimension of the gather's grid)

struct RecutLayout {
    BlobLayout blob;
    size_t bits, foff, by_unit, total;
    uint32_t bits_stride;                             // bit counts a frame
};

// the tables of every geometry and the cuts of a call, passed by value with the launches
struct RecutCutTables {
    const uint32_t *unit_slot[kRecutMaxReduce + 1], *final_order[kRecutMaxReduce + 1], *full_to_cut[kRecutMaxReduce + 1];
    const UnitDesc *units[kRecutMaxReduce + 1];
    uint32_t n_units[kRecutMaxReduce + 1], bits_at[kRecutMaxReduce + 1];     // bits_at: where a frame's bit counts at r start
};
struct RecutCuts {
    uint64_t quota[kMaxLadder];
    uint8_t reduce[kMaxLadder];
    uint32_t n;
};

// The byte-quota call: a frame's bit counts for the full geometry, each quota's final offsets (foff, rows of n_units entries).
// cuts: the workspace of icerx_recut_device_cuts_async -- bit counts for every geometry, and each cut's final offsets twice,
// in the order of its own geometry's units (by_unit) and in the order of the master's (foff); rows of n_units entries both
RecutLayout recut_layout(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts, bool cuts)
{
    RecutLayout L;
    const size_t N = (size_t)n, n_full = r->red[0].n_units;
    Carver c;
    const size_t head = c.take(sizeof(AsyncHead));
    L.blob = blob_layout(c, head, N, data_bytes, r->geom.slots());
    L.bits_stride = cuts ? r->units_total : r->red[0].n_units;
    L.bits = c.take(sizeof(uint32_t) * N * L.bits_stride);
    L.foff = c.take(sizeof(uint64_t) * N * n_full * (size_t)n_cuts);
    L.by_unit = cuts ? c.take(sizeof(uint64_t) * N * n_full * (size_t)n_cuts) : c.at;
    L.total = c.at;
    return L;
}

// Where the masters of a call lie -- frame k = blob bytes [offset(k), offset(k) + lens[k]) -- what the blob stage left of the
// blob (recs, head), what a frame must be (geom, image size), and where the frames' packet tables go (geom.slots() entries a
// frame).  By value with the launches.  (base: 0 but for the operands of combine.hpp.)
struct RecutTabRows { uint32_t *off, *bits; };
struct RecutMasters {
    const uint8_t *blob; uint32_t blob_len;
    const uint64_t *offsets, *lens; uint64_t base, stream_stride;
    const DCandRec *recs; const AsyncHead *head;
    DPlanGeom geom; uint64_t image_w, image_h;
    uint32_t *tab_off, *tab_bits;
    ICER_HD uint64_t offset(uint32_t k) const { return offsets ? offsets[k] : base + (uint64_t)k * stream_stride; }
    ICER_HD RecutTabRows rows(uint32_t k) const { return RecutTabRows{tab_off + (size_t)k * geom.slots(), tab_bits + (size_t)k * geom.slots()}; }
};

// The cuts' part of a call's workspace: frame k's bit counts (bits_stride a frame, a geometry's at tabs.bits_at[r]) and the
// cuts' final offsets in rows of n_full entries, row c * n + k.  A cut's walk leaves its row in the order of its own
// geometry's units: cut_row, which for r = 0 is the row of foff itself; recut_row_by_master then turns the row of a cut at
// r > 0 into the order of the master's units, which the gather goes by -- after a barrier of the caller's, thread `tid` of `nth`.
struct RecutWork {
    uint32_t *unit_bits;
    uint32_t bits_stride, n_full;
    uint64_t *foff, *by_unit;
    ICER_HD uint32_t *bits(uint32_t k) const { return unit_bits + (size_t)k * bits_stride; }
    ICER_HD uint64_t *cut_row(uint32_t r, size_t row) const { return (r ? by_unit : foff) + row * n_full; }
};
ICER_DEV void recut_row_by_master(const RecutWork &w, const RecutCutTables &tabs, uint32_t r, size_t row, uint32_t tid, uint32_t nth)
{
    if (r) recut_offsets_by_master_unit(w.by_unit + row * w.n_full, tabs.full_to_cut[r], w.n_full, w.foff + row * w.n_full, tid, nth);
}
// the outputs every call has: row c * n + k of `out`, entry c * n + k of sizes / rcs
struct RecutOut { uint8_t *out; size_t out_stride; unsigned long long *sizes; int32_t *rcs; };

// The decoder's cursor walk of frame [off, off + len) into the table rows `t`, by the whole workgroup (dynamic LDS: kWalkLds),
// and what it leaves of the frame.  Two walks of one workgroup need a barrier between them.
ICER_DEV RecutFrameHead recut_walk(uint8_t *lds, const RecutMasters &m, uint64_t off, uint64_t len, const RecutTabRows &t)
{
    WalkNotes notes;
    const DWalk s = walk_frame(lds, m.blob, m.blob_len, off, len, m.recs, m.head, m.geom, m.image_w, m.image_h, t.off, t.bits, &notes);
    return RecutFrameHead{recut_frame_status(notes.inside != 0u, s.cursor, notes.other_size != 0u), notes.max_level};
}
// How every frame kernel starts, one workgroup per frame: frame k's packet table, once, then the bit counts of every geometry
// in use (bit r of `used`) at which the frame has a stream, through that geometry's slot map.  No barrier behind it.
ICER_DEV RecutFrameHead recut_frame_stage(uint8_t *lds, const RecutMasters &m, uint32_t k, const RecutCutTables &tabs, const RecutWork &w,
                                          uint32_t used, uint32_t tid, uint32_t nth)
{
    const RecutTabRows t = m.rows(k);
    const RecutFrameHead f = recut_walk(lds, m, m.offset(k), m.lens[k], t);
    for (uint32_t r = 0; r <= (uint32_t)kRecutMaxReduce; r++)
        if (((used >> r) & 1u) && recut_cut_status(f, r) == kOk)
            recut_unit_bits(t.off, t.bits, tabs.unit_slot[r], tabs.n_units[r], w.bits(k) + tabs.bits_at[r], tid, nth);
    return f;
}

// one workgroup per frame: recut_frame_stage, and wavefront v takes the cuts v, v + waves, ...: the walk with the tables of
// the cut's geometry leaves the final offsets in the cut's row (cut_row), and the workgroup turns them into the order of the
// master's units.  A call whose every reduce is 0 touches neither by_unit nor a bit count past the full geometry's
// (bits_at[0] = 0).
__global__ void __launch_bounds__(256)
recut_plan_kernel(RecutMasters m, RecutCutTables tabs, RecutWork w, RecutCuts cuts, uint32_t used, RecutOut o)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // kWalkLds
    const uint32_t k = blockIdx.x, n = gridDim.x, tid = threadIdx.x;
    const RecutFrameHead f = recut_frame_stage(lds, m, k, tabs, w, used, tid, blockDim.x);
    ICER_BARRIER();
#ifdef ICER_HOST_MOCK
    const uint32_t wave = 0, waves = 1;
#else
    const uint32_t wave = tid >> 6, waves = blockDim.x >> 6;
#endif
    for (uint32_t c = wave; c < cuts.n; c += waves) {
        const size_t row = (size_t)c * n + k;
        const uint32_t r = cuts.reduce[c];
        recut_scan_wave(recut_cut_status(f, r), w.bits(k) + tabs.bits_at[r], tabs.final_order[r], tabs.n_units[r], cuts.quota[c], tabs.units[r],
                        w.cut_row(r, row), o.sizes + row, o.rcs + row);
    }
    ICER_BARRIER();
    for (uint32_t c = 0; c < cuts.n; c++) recut_row_by_master(w, tabs, cuts.reduce[c], (size_t)c * n + k, tid, blockDim.x);
}

// one workgroup per (unit of the master, frame): the unit's packet, wherever it lies in the master, to every cut's stream that
// keeps it.  The payload goes as it is, from byte 28 on; the header of cut c is written by thread c as it stands in the
// derived stream at the cut's reduce (recut_cut_header), so no two threads write the same byte.  (That the masters and the
// outputs do not overlap, which lets the copies load ahead of their stores, is said by the two copy functions' own parameters.)
__global__ void __launch_bounds__(256)
recut_gather_kernel(RecutMasters m, const uint32_t *__restrict__ unit_slot, uint32_t n_units, const uint64_t *__restrict__ foff, RecutCuts cuts,
                    const uint32_t *__restrict__ crc_tab, RecutOut o)
{
    const uint32_t ui = blockIdx.x, frame = blockIdx.y, n = gridDim.y, n_c = cuts.n;
    const size_t off_pitch = (size_t)n * n_units, q_pitch = (size_t)n * o.out_stride;
    const uint64_t *offs = foff + (size_t)frame * n_units + ui;
    // (a frame with a status, a unit without a packet, a unit behind every cut: nothing to copy, and nothing of it is looked at)
    bool any = false;
    for (uint32_t c = 0; c < n_c; c++) any |= offs[(size_t)c * off_pitch] != ~0ull;
    if (!any) return;
    const size_t slot = (size_t)frame * m.geom.slots() + unit_slot[ui];
    // (the walk accepted this packet: header and payload lie inside the frame, and the frame inside the blob)
    const uint8_t *src = m.blob + m.offset(frame) + m.tab_off[slot];
    uint8_t *rows = o.out + (size_t)frame * o.out_stride;
    for (uint32_t c = threadIdx.x; c < n_c; c += blockDim.x) {
        const uint64_t at = offs[(size_t)c * off_pitch];
        if (at != ~0ull) recut_cut_header(crc_tab, src, cuts.reduce[c], rows + (size_t)c * q_pitch + at);
    }
    copy_unit_recut(src + kHeaderBytes, (m.tab_bits[slot] + 7u) >> 3, offs, off_pitch, n_c, rows + kHeaderBytes, q_pitch, threadIdx.x, blockDim.x);
}

// ---- the call record and the driver ------------------------------------------------------------------------------------------
// A call as its entry point hands it on.  The cuts as the caller gave them: reduces null: every reduce 0.
struct RecutCall {
    int n; const uint8_t *d_data; size_t data_bytes;                              // the masters: the blob,
    const uint64_t *d_offsets; size_t stream_stride; const uint64_t *d_lens;      // and where frame k lies in it
    const int *reduces; const size_t *quotas; int n_cuts;                         // the cuts
    uint8_t *d_out; size_t out_stride; uint64_t *d_sizes; int32_t *d_rcs;         // the outputs every call has
    void *workspace; size_t workspace_bytes; hipStream_t st;
};
struct RecutRun {
    const icerx_recutter *r;
    RecutCall call;
    RecutCuts cuts;
    uint32_t used;                                    // bit r: a cut of the call has reduce r
    RecutCutTables tabs;
    RecutMasters masters;
    RecutWork work;
    RecutOut out;
};

hipError_t recut_upload(icerx_recutter *r, void **p, const void *src, size_t bytes)
{
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return e;
    r->owned.push_back(*p);
    return hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice);
}

RecutCutTables recut_cut_tables(const icerx_recutter *r)
{
    RecutCutTables tabs = {};
    uint32_t at = 0;
    for (int k = 0; k <= r->max_reduce; k++) {
        const icerx_recutter::Reduced &g = r->red[k];
        tabs.unit_slot[k] = (const uint32_t *)g.unit_slot; tabs.final_order[k] = (const uint32_t *)g.final_order;
        tabs.full_to_cut[k] = (const uint32_t *)g.full_to_cut; tabs.units[k] = (const UnitDesc *)g.units;
        tabs.n_units[k] = g.n_units; tabs.bits_at[k] = at;
        at += g.n_units;
    }
    return tabs;
}

// What every call checks first, in this order, and the cuts as the launches take them.  Every check of a call comes before
// the first thing enqueued: a refused call writes nothing.
int recut_check(const icerx_recutter *r, const RecutCall &c, RecutRun *run)
{
    if (!r || c.n < 1 || c.n > kRecutMaxFrames || c.n_cuts < 1 || c.n_cuts > kMaxLadder) return ICER_INVALID_INPUT;
    if (!c.quotas || !c.d_lens || !c.d_out || !c.d_sizes || !c.d_rcs || !c.workspace || (c.data_bytes && !c.d_data)) return ICER_INVALID_INPUT;
    size_t top = 0;
    run->cuts = {};
    run->cuts.n = (uint32_t)c.n_cuts;
    run->used = 0;
    for (int k = 0; k < c.n_cuts; k++) {
        const int reduce = c.reduces ? c.reduces[k] : 0;
        if (reduce < 0 || reduce > r->max_reduce) return ICER_INVALID_INPUT;
        run->cuts.quota[k] = c.quotas[k]; run->cuts.reduce[k] = (uint8_t)reduce;
        run->used |= 1u << reduce;
        top = std::max(top, c.quotas[k]);
    }
    if (c.out_stride < top) return ICER_INVALID_INPUT;
    if (c.data_bytes >= 0xFFFFFFFFull - 64u) return fail("batch of %zu stream bytes: 32-bit offsets only", c.data_bytes);
    return ICER_RESULT_OK;
}

// The last check of a checked call -- its workspace holds `total` bytes, of which L is the cuts' part --, then what every driver
// derives of the call, and the first thing enqueued: the candidates over the blob.
int recut_begin(const icerx_recutter *r, const RecutCall &c, const RecutLayout &L, size_t total, RecutRun *run)
{
    if (c.workspace_bytes < total) return ICER_INVALID_INPUT;
    uint8_t *ws = (uint8_t *)c.workspace;
    run->r = r; run->call = c;
    run->tabs = recut_cut_tables(r);
    run->masters = RecutMasters{c.d_data, (uint32_t)c.data_bytes, c.d_offsets, c.d_lens, 0, (uint64_t)c.stream_stride,
                                (const DCandRec *)(ws + L.blob.cands), (const AsyncHead *)(ws + L.blob.head), r->geom, r->w, r->h,
                                (uint32_t *)(ws + L.blob.tab_off), (uint32_t *)(ws + L.blob.tab_bits)};
    run->work = RecutWork{(uint32_t *)(ws + L.bits), L.bits_stride, r->red[0].n_units, (uint64_t *)(ws + L.foff),
                          (uint64_t *)(ws + L.by_unit)};
    run->out = RecutOut{c.d_out, c.out_stride, (unsigned long long *)c.d_sizes, c.d_rcs};
    return enqueue_blob_stage(L.blob, ws, (size_t)c.n, r->geom.slots(), c.d_data, c.data_bytes, (const uint32_t *)r->crc, r->n_cus, c.st);
}

// the last thing enqueued: the kept packets, each with its cut's header
int recut_finish(const RecutRun &run)
{
    int rc = ICER_RESULT_OK;
    ICER_LAUNCH_ON(run.call.st, recut_gather_kernel, dim3(run.work.n_full, (unsigned)run.call.n), kRecutGatherThreads, 0, run.masters,
                   run.tabs.unit_slot[0], run.work.n_full, (const uint64_t *)run.work.foff, run.cuts, (const uint32_t *)run.r->crc, run.out);
    HIP_TRY(hipGetLastError());
done:
    return rc;
}

// The byte-quota call and the cuts call.  by_resolution = false: the byte-quota call -- the call has no reduces, and the
// workspace is its own smaller one (recut_layout), outside of which the kernels then touch nothing.
int recut_async(icerx_recutter *r, const RecutCall &c, bool by_resolution)
{
    g_error.clear();
    if (by_resolution && !c.reduces) return ICER_INVALID_INPUT;
    RecutRun run;
    int rc = recut_check(r, c, &run);
    if (rc != ICER_RESULT_OK) return rc;
    const RecutLayout L = recut_layout(r, c.n, c.data_bytes, c.n_cuts, by_resolution);
    if ((rc = recut_begin(r, c, L, L.total, &run)) != ICER_RESULT_OK) return rc;
    // per frame: packet table, then every cut's walk with the tables of its geometry
    ICER_LAUNCH_ON(c.st, recut_plan_kernel, (unsigned)c.n, kRecutPlanThreads, kWalkLds, run.masters, run.tabs, run.work, run.cuts,
                   run.used, run.out);
    HIP_TRY(hipGetLastError());
    rc = recut_finish(run);
done:
    return rc;
}

// ---- icerx_recut_device_roi_async ----------------------------------------------------------------------------------------
// what the frame stage leaves of a frame: the walk's, and its rectangle clipped to the full frame
struct RecutRoiFrame {
    RecutFrameHead head;
    RoiBox box;
};
// the distinct (reduce, shift) of a call's cuts -- a rank each -- and the one every cut goes by; by value with the launches
struct RecutRoiCuts {
    uint8_t pair[kMaxLadder], pair_reduce[kMaxLadder], pair_shift[kMaxLadder];
    uint32_t n_pairs;
};
struct RecutRoiPrio {
    const uint64_t *p[kRecutMaxReduce + 1];
};
#ifdef ICER_HOST_MOCK
constexpr uint32_t kRecutRankThreads = 1, kRecutScanThreads = 1;
#else
constexpr uint32_t kRecutRankThreads = 64u * kRoiWaves, kRecutScanThreads = 64;
#endif

// The workspace of the cuts call, then: a record per frame; per frame and rank (at most one per cut) the sort keys, rank and
// order in rows of n_units[0] entries and the foreground count; per frame and cut the bit counts in ROI order (scan_roi_wave's
// scratch), rows alike.  RecutRoiWork: the same as pointers, by value with the launches.
struct RecutRoiLayout {
    RecutLayout cut;
    size_t frames, keys, rank, order, fg, pbits, total;
};
struct RecutRoiWork {
    RecutRoiFrame *frames;
    uint64_t *keys;
    uint32_t *rank, *order, *fg, *pbits;
};
RecutRoiLayout recut_roi_layout(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts)
{
    RecutRoiLayout L;
    L.cut = recut_layout(r, n, data_bytes, n_cuts, true);
    const size_t rows = (size_t)n * (size_t)n_cuts, per = rows * r->red[0].n_units;
    Carver c;
    c.at = L.cut.total;
    L.frames = c.take(sizeof(RecutRoiFrame) * (size_t)n);
    L.keys = c.take(sizeof(uint64_t) * per);
    L.rank = c.take(sizeof(uint32_t) * per);
    L.order = c.take(sizeof(uint32_t) * per);
    L.fg = c.take(sizeof(uint32_t) * rows);
    L.pbits = c.take(sizeof(uint32_t) * per);
    L.total = c.at;
    return L;
}

// one workgroup per frame: recut_frame_stage; and the frame's record, its rectangle rois[4 k ..] = x, y, w, h clipped to the
// full frame
__global__ void __launch_bounds__(256)
recut_roi_frame_kernel(RecutMasters m, RecutCutTables tabs, RecutWork w, uint32_t used, const uint32_t *__restrict__ rois,
                       RecutRoiFrame *__restrict__ frames)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // kWalkLds
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const RecutFrameHead f = recut_frame_stage(lds, m, k, tabs, w, used, tid, blockDim.x);
    if (tid == 0) frames[k] = RecutRoiFrame{f, roi_clip(rois + 4u * (size_t)k, (uint32_t)m.image_w, (uint32_t)m.image_h)};
}

// the clipped rectangle of the full frame at 1/2^r size: [x0 >> r, ceil(x1 / 2^r)) x [y0 >> r, ceil(y1 / 2^r)), never empty
// unless `b` is; an empty one stays as it is (roi_empty is all that is asked of it)
ICER_HD RoiBox recut_roi_box(const RoiBox &b, uint32_t r)
{
    if (r == 0u || b.x1 <= b.x0 || b.y1 <= b.y0) return b;
    RoiBox c;
    c.x0 = b.x0 >> r; c.y0 = b.y0 >> r;
    c.x1 = (uint32_t)reduced_dim(b.x1, (int)r); c.y1 = (uint32_t)reduced_dim(b.y1, (int)r);
    return c;
}

// one workgroup per (frame, rank p): roi_rank_kernel's four phases (kernels.hpp of the encoder library) over the units and
// priorities of the geometry at 1/2^r size.  Row p * n + k of keys / rank / order (pitch entries a row) and of fg.  A frame
// without a stream at r has no rank: fg 0, nothing else written.  Dynamic LDS: a RoiShared.
__global__ void __launch_bounds__(64 * kRoiWaves)
recut_roi_rank_kernel(RecutCutTables tabs, RecutRoiPrio prio, RecutRoiCuts rc, RecutRoiWork rw, uint64_t image_w, uint64_t image_h, uint32_t pitch)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);
    RoiShared &s = *reinterpret_cast<RoiShared *>(lds);
    const uint32_t k = blockIdx.x, p = blockIdx.y, n = gridDim.x, tid = threadIdx.x;
    const uint32_t r = rc.pair_reduce[p], shift = rc.pair_shift[p];
    const size_t row = (size_t)p * n + k;
    const RecutRoiFrame fr = rw.frames[k];
    if (recut_cut_status(fr.head, r) != kOk) {                 // (the whole workgroup: no barrier is left out by a part of it)
        if (tid == 0) rw.fg[row] = 0u;
        return;
    }
#ifdef ICER_HOST_MOCK
    const uint32_t wv = 0, nwv = 1;
#else
    const uint32_t wv = tid >> 6, nwv = blockDim.x >> 6;
#endif
    const RoiFrame f{tabs.units[r], tabs.n_units[r], (uint32_t)reduced_dim(image_w, (int)r), (uint32_t)reduced_dim(image_h, (int)r),
                     recut_roi_box(fr.box, r)};
    uint64_t *ky = rw.keys + row * pitch;
    roi_count_wave(s, f, wv, nwv);
    ICER_BARRIER();
    if (wv == 0) roi_scan_wave(s, f.n_units);
    ICER_BARRIER();
    roi_place_wave(s, f, prio.p[r], shift, ky, nullptr, nullptr, wv, nwv);
    ICER_BARRIER();
    roi_place_wave(s, f, prio.p[r], shift, ky, rw.rank + row * pitch, rw.order + row * pitch, wv, nwv);
    if (tid == 0) rw.fg[row] = s.n_fg;
}

// one wavefront per (frame, cut): the cut's walk along the frame's ROI order of the cut's (reduce, shift), with the tables of
// the geometry at 1/2^r size.  Rows c * n + k as recut_plan_kernel's; kept / foreground: K and the foreground count, 0 for a
// frame with a status, which otherwise gets what recut_scan_wave writes.
__global__ void __launch_bounds__(64)
recut_roi_scan_kernel(RecutCutTables tabs, RecutWork w, RecutCuts cuts, RecutRoiCuts rc, RecutRoiWork rw, RecutOut o,
                      uint32_t *__restrict__ kept, uint32_t *__restrict__ foreground)
{
    const uint32_t k = blockIdx.x, c = blockIdx.y, n = gridDim.x, tid = threadIdx.x, n_full = w.n_full;
    const uint32_t r = cuts.reduce[c];
    const size_t row = (size_t)c * n + k, prow = (size_t)rc.pair[c] * n + k;
    const int status = recut_cut_status(rw.frames[k].head, r);
    const uint32_t *bits = w.bits(k) + tabs.bits_at[r];
    uint64_t *cut_off = w.cut_row(r, row);
    if (status != kOk) {
        recut_scan_wave(status, bits, tabs.final_order[r], tabs.n_units[r], cuts.quota[c], tabs.units[r], cut_off, o.sizes + row, o.rcs + row);
        if (tid == 0) { kept[row] = 0u; foreground[row] = 0u; }
    } else {
        (void)scan_roi_wave(bits, tabs.final_order[r], tabs.n_units[r], cuts.quota[c], 0, tabs.units[r], rw.rank + prow * n_full,
                            rw.order + prow * n_full, rw.pbits + row * n_full, cut_off, o.sizes + row, o.rcs + row, kept + row);
        if (tid == 0) foreground[row] = rw.fg[prow];
    }
    if (r) {
        ICER_BARRIER();
        recut_row_by_master(w, tabs, r, row, tid, blockDim.x);
    }
}

// icerx_recut_device_roi_async: the cuts call with a shift per cut and the frames' rectangles
int recut_roi_async(icerx_recutter *r, const RecutCall &c, const uint32_t *d_rois, const int *shifts, uint32_t *d_kept, uint32_t *d_foreground)
{
    g_error.clear();
    if (!d_rois || !shifts || !d_kept || !d_foreground) return ICER_INVALID_INPUT;
    RecutRun run;
    int rc = recut_check(r, c, &run);
    if (rc != ICER_RESULT_OK) return rc;
    RecutRoiCuts pairs = {};
    for (int k = 0; k < c.n_cuts; k++) {
        if (shifts[k] < 0 || shifts[k] > kMaxRoiShift) return ICER_INVALID_INPUT;
        uint32_t p = 0;
        while (p < pairs.n_pairs && (pairs.pair_reduce[p] != run.cuts.reduce[k] || pairs.pair_shift[p] != (uint8_t)shifts[k])) p++;
        if (p == pairs.n_pairs) { pairs.pair_reduce[p] = run.cuts.reduce[k]; pairs.pair_shift[p] = (uint8_t)shifts[k]; pairs.n_pairs++; }
        pairs.pair[k] = (uint8_t)p;
    }
    const RecutRoiLayout L = recut_roi_layout(r, c.n, c.data_bytes, c.n_cuts);
    if ((rc = recut_begin(r, c, L.cut, L.total, &run)) != ICER_RESULT_OK) return rc;
    uint8_t *ws = (uint8_t *)c.workspace;
    const RecutRoiWork rw{(RecutRoiFrame *)(ws + L.frames), (uint64_t *)(ws + L.keys), (uint32_t *)(ws + L.rank), (uint32_t *)(ws + L.order),
                          (uint32_t *)(ws + L.fg), (uint32_t *)(ws + L.pbits)};
    RecutRoiPrio prio = {};
    for (int k = 0; k <= r->max_reduce; k++) prio.p[k] = (const uint64_t *)r->red[k].prio;

    // per frame: packet table, bit counts, the clipped rectangle
    ICER_LAUNCH_ON(c.st, recut_roi_frame_kernel, (unsigned)c.n, kRecutPlanThreads, kWalkLds, run.masters, run.tabs, run.work, run.used, d_rois,
                   rw.frames);
    HIP_TRY(hipGetLastError());
    // per frame and distinct (reduce, shift): the ROI order
    ICER_LAUNCH_ON(c.st, recut_roi_rank_kernel, dim3((unsigned)c.n, pairs.n_pairs), kRecutRankThreads, sizeof(RoiShared), run.tabs, prio, pairs, rw,
                   r->w, r->h, run.work.n_full);
    HIP_TRY(hipGetLastError());
    // per frame and cut: the walk along that order
    ICER_LAUNCH_ON(c.st, recut_roi_scan_kernel, dim3((unsigned)c.n, (unsigned)c.n_cuts), kRecutScanThreads, 0, run.tabs, run.work, run.cuts, pairs,
                   rw, run.out, d_kept, d_foreground);
    HIP_TRY(hipGetLastError());
    rc = recut_finish(run);
done:
    return rc;
}

// ---- the recutter ------------------------------------------------------------------------------------------------------------
// the three tables of a plan on the device; slot[u]: the slot of unit u in the packet table of the master's geometry, levels
// raised by `reduce`
int recut_upload_plan(icerx_recutter *r, const Plan &plan, uint32_t reduce, std::vector<uint32_t> *slot)
{
    int rc = ICER_RESULT_OK;
    icerx_recutter::Reduced &g = r->red[reduce];
    slot->resize(plan.units.size());
    for (size_t u = 0; u < plan.units.size(); u++) {
        const UnitDesc &d = plan.units[u];
        (*slot)[u] = r->geom.slot(d.chan, d.level + reduce, d.subband, d.seg, d.lsb);
    }
    HIP_TRY(recut_upload(r, &g.unit_slot, slot->data(), sizeof(uint32_t) * slot->size()));
    HIP_TRY(recut_upload(r, &g.final_order, plan.final_order.data(), sizeof(uint32_t) * plan.final_order.size()));
    HIP_TRY(recut_upload(r, &g.units, plan.units.data(), sizeof(UnitDesc) * plan.units.size()));
done:
    return rc;
}

// quality: a quality recutter for masters made with filter `filt` (recut_quality.hpp), whose tables are built and checked on
// the host before anything is allocated; a plain one has filt -1
struct RecutterOptions {
    int device, max_reduce;
    bool quality;
    int filt;
};
int recutter_create(icerx_recutter **out, size_t w, size_t h, int channels, int stages, unsigned segments, int sample_bits,
                    const RecutterOptions &opt)
{
    g_error.clear();
    if (!out) return ICER_INVALID_INPUT;
    *out = nullptr;
    if (sample_bits != 8 && sample_bits != 16) return ICER_INVALID_INPUT;
    const int device = opt.device, max_reduce = opt.max_reduce;
    const int segs = segments > (unsigned)kMaxSegments ? kMaxSegments + 1 : (int)segments;
    std::vector<Plan> plans(1);
    const int prc = build_plan(&plans[0], w, h, channels, stages, segs, sample_bits);
    if (prc != kOk) return prc;
    if (max_reduce < 0 || max_reduce >= stages) return ICER_INVALID_INPUT;
    plans.resize((size_t)max_reduce + 1);
    for (int k = 1; k <= max_reduce; k++) {
        const int krc = build_plan(&plans[k], (size_t)reduced_dim(w, k), (size_t)reduced_dim(h, k), channels, stages - k, segs, sample_bits);
        if (krc != kOk) return krc;
    }
    const DPlanGeom geom{(uint32_t)channels, (uint32_t)stages, segments, (uint32_t)(sample_bits == 8 ? kPlanes8 : kPlanes)};
    RecutQualityHost qual;
    if (opt.quality)
        if (const int qrc = recut_quality_build(plans, geom, opt.filt, sample_bits, &qual)) return qrc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no usable HIP device");
#ifndef ICER_HOST_MOCK
    if (device >= 0) {
        if (device >= ndev) return fail("device %d of %d", device, ndev);
        if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice(%d) failed", device);
    }
#endif
    icerx_recutter *r = new icerx_recutter;
    r->device = device; r->w = w; r->h = h; r->max_reduce = max_reduce;
    r->geom = geom;
#ifndef ICER_HOST_MOCK
    { int cur = 0; hipDeviceProp_t prop; if (hipGetDevice(&cur) == hipSuccess && hipGetDeviceProperties(&prop, cur) == hipSuccess && prop.multiProcessorCount > 0) r->n_cus = prop.multiProcessorCount; }
#endif
    uint32_t crc_tab[256];
    build_crc32_table(crc_tab);
    int rc = ICER_RESULT_OK;
    std::vector<uint32_t> slot0, slot;
    std::vector<uint64_t> prio;
    HIP_TRY(recut_upload(r, &r->crc, crc_tab, sizeof crc_tab));
    for (int k = 0; k <= max_reduce; k++) {
        icerx_recutter::Reduced &g = r->red[k];
        g.n_units = (uint32_t)plans[k].units.size();
        r->units_total += g.n_units;
        if ((rc = recut_upload_plan(r, plans[k], (uint32_t)k, &slot)) != ICER_RESULT_OK) goto done;
        if (!roi_priorities(plans[k], &prio)) {        // (no geometry the planner accepts gets here: make_packets keeps the bound and the order)
            rc = fail("recutter: the packet priorities of the geometry at 1/2^%d size do not fit the sort keys", k);
            goto done;
        }
        HIP_TRY(recut_upload(r, &g.prio, prio.data(), sizeof(uint64_t) * prio.size()));
        if (k == 0) { slot0 = slot; continue; }
        std::vector<uint32_t> of_slot(r->geom.slots(), kNoPacket), full_to_cut(slot0.size());
        for (size_t u = 0; u < slot.size(); u++) of_slot[slot[u]] = (uint32_t)u;
        for (size_t u = 0; u < slot0.size(); u++) full_to_cut[u] = of_slot[slot0[u]];
        HIP_TRY(recut_upload(r, &g.full_to_cut, full_to_cut.data(), sizeof(uint32_t) * full_to_cut.size()));
    }
    if (opt.quality) {
        r->filt = opt.filt;
        if ((rc = recut_quality_upload(r, qual)) != ICER_RESULT_OK) goto done;
    }
    *out = r;
    return ICER_RESULT_OK;
done:
    icerx_recutter_destroy(r);
    return rc;
}

// what every *_workspace_bytes entry point asks before it lays a workspace out; quality: the call needs a quality recutter
bool recut_sizable(const icerx_recutter *r, int n, int n_cuts, bool quality)
{
    return r && (!quality || r->filt >= 0) && n > 0 && n_cuts >= 1 && n_cuts <= kMaxLadder;
}

}  // namespace

extern "C" {

void icerx_recutter_destroy(icerx_recutter *r)
{
    if (!r) return;
    for (void *p : r->owned) (void)hipFree(p);
    delete r;
}

int icerx_recutter_create(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, unsigned segments,
                          int sample_bits)
{
    return recutter_create(out, w, h, channels, stages, segments, sample_bits, RecutterOptions{device, 0, false, -1});
}

int icerx_recutter_create_reduced(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, unsigned segments,
                                  int sample_bits, int max_reduce)
{
    return recutter_create(out, w, h, channels, stages, segments, sample_bits, RecutterOptions{device, max_reduce, false, -1});
}

int icerx_recutter_max_reduce(const icerx_recutter *r) { return r ? r->max_reduce : 0; }

size_t icerx_recut_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_quotas)
{
    return recut_sizable(r, n, n_quotas, false) ? recut_layout(r, n, data_bytes, n_quotas, false).total : 0;
}

int icerx_recut_device_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                             size_t stream_stride, const uint64_t *d_lens, const size_t *quotas, int n_quotas, uint8_t *d_out,
                             size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return recut_async(r, RecutCall{n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, nullptr, quotas, n_quotas, d_out,
                                    out_stride, d_sizes, d_rcs, d_workspace, workspace_bytes, (hipStream_t)stream}, false);
}

size_t icerx_recut_cuts_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts)
{
    return recut_sizable(r, n, n_cuts, false) ? recut_layout(r, n, data_bytes, n_cuts, true).total : 0;
}

int icerx_recut_device_cuts_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                  size_t stream_stride, const uint64_t *d_lens, const int *reduces, const size_t *quotas, int n_cuts,
                                  uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *d_workspace,
                                  size_t workspace_bytes, void *stream)
{
    return recut_async(r, RecutCall{n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, reduces, quotas, n_cuts, d_out,
                                    out_stride, d_sizes, d_rcs, d_workspace, workspace_bytes, (hipStream_t)stream}, true);
}

size_t icerx_recut_roi_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts)
{
    return recut_sizable(r, n, n_cuts, false) ? recut_roi_layout(r, n, data_bytes, n_cuts).total : 0;
}

int icerx_recut_device_roi_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                 size_t stream_stride, const uint64_t *d_lens, const uint32_t *d_rois, const int *reduces,
                                 const int *shifts, const size_t *quotas, int n_cuts, uint8_t *d_out, size_t out_stride,
                                 uint64_t *d_sizes, int32_t *d_rcs, uint32_t *d_kept, uint32_t *d_foreground, void *d_workspace,
                                 size_t workspace_bytes, void *stream)
{
    return recut_roi_async(r, RecutCall{n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, reduces, quotas, n_cuts, d_out,
                                        out_stride, d_sizes, d_rcs, d_workspace, workspace_bytes, (hipStream_t)stream},
                           d_rois, shifts, d_kept, d_foreground);
}

}  // extern "C"
