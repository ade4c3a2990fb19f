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
// icerx_recut_device_roi_async: a cut is (reduce r, quota, ROI shift), the frames' rectangles lie in device memory.  The blob
// stage and the gather are the ones above; between them three launches stand in recut_plan_kernel's place, each as wide as
// its own work ("Region of interest from stored masters"):
//   frames     recut_roi_frame_kernel, one workgroup per frame: walk_frame and recut_unit_bits as above; the frame's
//              rectangle clipped to the full frame, once
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

extern "C" void icerx_recutter_destroy(icerx_recutter *r);

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

// one workgroup per frame (frame k addressed as in plan_frames_kernel): the packet table once, then the bit counts of every
// geometry in use (bit r of `used`) through that geometry's slot map (bits_stride counts a frame), and wavefront v takes the
// cuts v, v + waves, ...: the walk with the tables of the cut's geometry leaves the final offsets in the order of that
// geometry's units (by_unit; reduce 0: foff at once), and the workgroup turns them into the order of the master's units,
// which the gather goes by.  Row c * n + k of sizes / rcs and of foff / by_unit (n_units[0] entries a row).  A call whose
// every reduce is 0 touches neither by_unit nor a bit count past the full geometry's (bits_at[0] = 0).
__global__ void __launch_bounds__(256)
recut_plan_kernel(const uint8_t *__restrict__ blob, uint32_t blob_len, const uint64_t *__restrict__ offsets, uint64_t stream_stride,
                  const uint64_t *__restrict__ lens, const DCandRec *__restrict__ recs, const AsyncHead *__restrict__ head,
                  DPlanGeom geom, uint64_t image_w, uint64_t image_h, RecutCutTables tabs, uint32_t bits_stride, RecutCuts cuts,
                  uint32_t n_c, uint32_t used, uint32_t *__restrict__ tab_off, uint32_t *__restrict__ tab_bits,
                  uint32_t *__restrict__ unit_bits, uint64_t *__restrict__ foff, uint64_t *__restrict__ by_unit,
                  unsigned long long *__restrict__ sizes, int32_t *__restrict__ rcs)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // kWalkLds
    const uint32_t k = blockIdx.x, n = gridDim.x, tid = threadIdx.x, n_full = tabs.n_units[0];
    const uint64_t off = offsets ? offsets[k] : (uint64_t)k * stream_stride, len = lens[k];
    uint32_t *to = tab_off + (size_t)k * geom.slots(), *tb = tab_bits + (size_t)k * geom.slots();
    uint32_t *bits = unit_bits + (size_t)k * bits_stride;
    WalkNotes notes;
    const DWalk s = walk_frame(lds, blob, blob_len, off, len, recs, head, geom, image_w, image_h, to, tb, &notes);
    const int status = recut_frame_status(notes.inside != 0u, s.cursor, notes.other_size != 0u);
    const uint32_t max_level = notes.max_level;
    for (uint32_t r = 0; r <= (uint32_t)kRecutMaxReduce; r++)
        if (((used >> r) & 1u) && recut_cut_status(status, max_level, r) == kOk)
            recut_unit_bits(to, tb, tabs.unit_slot[r], tabs.n_units[r], bits + tabs.bits_at[r], tid, blockDim.x);
    ICER_BARRIER();
#ifdef ICER_HOST_MOCK
    const uint32_t wave = 0, waves = 1;
#else
    const uint32_t wave = tid >> 6, waves = blockDim.x >> 6;
#endif
    for (uint32_t c = wave; c < n_c; c += waves) {
        const size_t row = (size_t)c * n + k;
        const uint32_t r = cuts.reduce[c];
        recut_scan_wave(recut_cut_status(status, max_level, r), bits + tabs.bits_at[r], tabs.final_order[r], tabs.n_units[r], cuts.quota[c],
                        tabs.units[r], (r ? by_unit : foff) + row * n_full, sizes + row, rcs + row);
    }
    ICER_BARRIER();
    for (uint32_t c = 0; c < n_c; c++) {
        const size_t row = (size_t)c * n + k;
        const uint32_t r = cuts.reduce[c];
        if (r) recut_offsets_by_master_unit(by_unit + row * n_full, tabs.full_to_cut[r], n_full, foff + row * n_full, tid, blockDim.x);
    }
}

// one workgroup per (unit of the master, frame): the unit's packet, wherever it lies in the master, to every cut's stream that
// keeps it.  The payload goes as it is, from byte 28 on; the header of cut c is written by thread c as it stands in the
// derived stream at the cut's reduce (recut_cut_header), so no two threads write the same byte.
__global__ void __launch_bounds__(256)
recut_gather_kernel(const uint8_t *__restrict__ blob, const uint64_t *__restrict__ offsets, uint64_t stream_stride, DPlanGeom geom,
                    const uint32_t *__restrict__ unit_slot, uint32_t n_units, const uint32_t *__restrict__ tab_off,
                    const uint32_t *__restrict__ tab_bits, const uint64_t *__restrict__ foff, RecutCuts cuts, uint32_t n_c,
                    const uint32_t *__restrict__ crc_tab, uint8_t *__restrict__ out, size_t out_stride)
{
    const uint32_t ui = blockIdx.x, frame = blockIdx.y, n = gridDim.y;
    const size_t off_pitch = (size_t)n * n_units, q_pitch = (size_t)n * out_stride;
    const uint64_t *offs = foff + (size_t)frame * n_units + ui;
    // (a frame with a status, a unit without a packet, a unit behind every cut: nothing to copy, and nothing of it is looked at)
    bool any = false;
    for (uint32_t c = 0; c < n_c; c++) any |= offs[(size_t)c * off_pitch] != ~0ull;
    if (!any) return;
    const uint64_t off = offsets ? offsets[frame] : (uint64_t)frame * stream_stride;
    const size_t slot = (size_t)frame * geom.slots() + unit_slot[ui];
    // (the walk accepted this packet: header and payload lie inside the frame, and the frame inside the blob)
    const uint8_t *src = blob + off + tab_off[slot];
    uint8_t *rows = out + (size_t)frame * out_stride;
    for (uint32_t c = threadIdx.x; c < n_c; c += blockDim.x) {
        const uint64_t at = offs[(size_t)c * off_pitch];
        if (at != ~0ull) recut_cut_header(crc_tab, src, cuts.reduce[c], rows + (size_t)c * q_pitch + at);
    }
    copy_unit_recut(src + kHeaderBytes, (tab_bits[slot] + 7u) >> 3, offs, off_pitch, n_c, rows + kHeaderBytes, q_pitch, threadIdx.x, blockDim.x);
}

// ---- icerx_recut_device_roi_async ----------------------------------------------------------------------------------------
// what the frame stage leaves of a frame: its status and top level (recut_cut_status), its rectangle clipped to the full frame
struct RecutRoiFrame {
    int32_t status;
    uint32_t max_level;
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
// scratch), rows alike.
struct RecutRoiLayout {
    RecutLayout cut;
    size_t frames, keys, rank, order, fg, pbits, total;
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

// one workgroup per frame, as recut_plan_kernel up to its first barrier: the packet table once, the bit counts of every
// geometry in use; and the frame's record, its rectangle rois[4 k ..] = x, y, w, h clipped to the full frame
__global__ void __launch_bounds__(256)
recut_roi_frame_kernel(const uint8_t *__restrict__ blob, uint32_t blob_len, const uint64_t *__restrict__ offsets, uint64_t stream_stride,
                       const uint64_t *__restrict__ lens, const DCandRec *__restrict__ recs, const AsyncHead *__restrict__ head,
                       DPlanGeom geom, uint64_t image_w, uint64_t image_h, RecutCutTables tabs, uint32_t bits_stride, uint32_t used,
                       const uint32_t *__restrict__ rois, uint32_t *__restrict__ tab_off, uint32_t *__restrict__ tab_bits,
                       uint32_t *__restrict__ unit_bits, RecutRoiFrame *__restrict__ frames)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // kWalkLds
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const uint64_t off = offsets ? offsets[k] : (uint64_t)k * stream_stride, len = lens[k];
    uint32_t *to = tab_off + (size_t)k * geom.slots(), *tb = tab_bits + (size_t)k * geom.slots();
    uint32_t *bits = unit_bits + (size_t)k * bits_stride;
    WalkNotes notes;
    const DWalk s = walk_frame(lds, blob, blob_len, off, len, recs, head, geom, image_w, image_h, to, tb, &notes);
    const int status = recut_frame_status(notes.inside != 0u, s.cursor, notes.other_size != 0u);
    for (uint32_t r = 0; r <= (uint32_t)kRecutMaxReduce; r++)
        if (((used >> r) & 1u) && recut_cut_status(status, notes.max_level, r) == kOk)
            recut_unit_bits(to, tb, tabs.unit_slot[r], tabs.n_units[r], bits + tabs.bits_at[r], tid, blockDim.x);
    if (tid == 0) {
        RecutRoiFrame f;
        f.status = status; f.max_level = notes.max_level;
        f.box = roi_clip(rois + 4u * (size_t)k, (uint32_t)image_w, (uint32_t)image_h);
        frames[k] = f;
    }
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
recut_roi_rank_kernel(RecutCutTables tabs, RecutRoiPrio prio, RecutRoiCuts rc, const RecutRoiFrame *__restrict__ frames, uint64_t image_w,
                      uint64_t image_h, uint32_t pitch, uint64_t *keys, uint32_t *__restrict__ rank, uint32_t *__restrict__ order,
                      uint32_t *__restrict__ fg)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);
    RoiShared &s = *reinterpret_cast<RoiShared *>(lds);
    const uint32_t k = blockIdx.x, p = blockIdx.y, n = gridDim.x, tid = threadIdx.x;
    const uint32_t r = rc.pair_reduce[p], shift = rc.pair_shift[p];
    const size_t row = (size_t)p * n + k;
    const RecutRoiFrame fr = frames[k];
    if (recut_cut_status(fr.status, fr.max_level, r) != kOk) {           // (the whole workgroup: no barrier is left out by a part of it)
        if (tid == 0) fg[row] = 0u;
        return;
    }
#ifdef ICER_HOST_MOCK
    const uint32_t wv = 0, nwv = 1;
#else
    const uint32_t wv = tid >> 6, nwv = blockDim.x >> 6;
#endif
    const RoiFrame f{tabs.units[r], tabs.n_units[r], (uint32_t)reduced_dim(image_w, (int)r), (uint32_t)reduced_dim(image_h, (int)r),
                     recut_roi_box(fr.box, r)};
    uint64_t *ky = keys + row * pitch;
    roi_count_wave(s, f, wv, nwv);
    ICER_BARRIER();
    if (wv == 0) roi_scan_wave(s, f.n_units);
    ICER_BARRIER();
    roi_place_wave(s, f, prio.p[r], shift, ky, nullptr, nullptr, wv, nwv);
    ICER_BARRIER();
    roi_place_wave(s, f, prio.p[r], shift, ky, rank + row * pitch, order + row * pitch, wv, nwv);
    if (tid == 0) fg[row] = s.n_fg;
}

// one wavefront per (frame, cut): the cut's walk along the frame's ROI order of the cut's (reduce, shift), with the tables of
// the geometry at 1/2^r size.  Rows c * n + k as recut_plan_kernel's; kept / foreground: K and the foreground count, 0 for a
// frame with a status, which otherwise gets what recut_scan_wave writes.
__global__ void __launch_bounds__(64)
recut_roi_scan_kernel(RecutCutTables tabs, uint32_t bits_stride, RecutCuts cuts, RecutRoiCuts rc, const RecutRoiFrame *__restrict__ frames,
                      const uint32_t *__restrict__ unit_bits, const uint32_t *__restrict__ rank, const uint32_t *__restrict__ order,
                      const uint32_t *__restrict__ fg, uint32_t *pbits, uint64_t *foff, uint64_t *by_unit,
                      unsigned long long *__restrict__ sizes, int32_t *__restrict__ rcs, uint32_t *__restrict__ kept,
                      uint32_t *__restrict__ foreground)
{
    const uint32_t k = blockIdx.x, c = blockIdx.y, n = gridDim.x, tid = threadIdx.x, n_full = tabs.n_units[0];
    const uint32_t r = cuts.reduce[c];
    const size_t row = (size_t)c * n + k, prow = (size_t)rc.pair[c] * n + k;
    const RecutRoiFrame fr = frames[k];
    const int status = recut_cut_status(fr.status, fr.max_level, r);
    const uint32_t *bits = unit_bits + (size_t)k * bits_stride + tabs.bits_at[r];
    uint64_t *cut_off = (r ? by_unit : foff) + row * n_full;
    if (status != kOk) {
        recut_scan_wave(status, bits, tabs.final_order[r], tabs.n_units[r], cuts.quota[c], tabs.units[r], cut_off, sizes + row, rcs + row);
        if (tid == 0) { kept[row] = 0u; foreground[row] = 0u; }
    } else {
        (void)scan_roi_wave(bits, tabs.final_order[r], tabs.n_units[r], cuts.quota[c], 0, tabs.units[r], rank + prow * n_full,
                            order + prow * n_full, pbits + row * n_full, cut_off, sizes + row, rcs + row, kept + row);
        if (tid == 0) foreground[row] = fg[prow];
    }
    if (r) {
        ICER_BARRIER();
        recut_offsets_by_master_unit(cut_off, tabs.full_to_cut[r], n_full, foff + row * n_full, tid, blockDim.x);
    }
}

hipError_t recut_upload(void **p, const void *src, size_t bytes)
{
    const hipError_t e = hipMalloc(p, bytes);
    return e != hipSuccess ? e : hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice);
}

// What every call checks first, in this order, and the cuts as the launches take them (`reduces` null: every reduce 0).  Every
// check of a call comes before the first thing enqueued: a refused call writes nothing.
int recut_check(const icerx_recutter *r, int n, const uint8_t *d_data, size_t data_bytes, const uint64_t *d_lens, const int *reduces,
                const size_t *quotas, int n_cuts, const uint8_t *d_out, size_t out_stride, const uint64_t *d_sizes, const int32_t *d_rcs,
                const void *workspace, RecutCuts *cuts, uint32_t *used)
{
    if (!r || n < 1 || n > kRecutMaxFrames || n_cuts < 1 || n_cuts > kMaxLadder) return ICER_INVALID_INPUT;
    if (!quotas || !d_lens || !d_out || !d_sizes || !d_rcs || !workspace || (data_bytes && !d_data)) return ICER_INVALID_INPUT;
    size_t top = 0;
    *used = 0;
    for (int c = 0; c < n_cuts; c++) {
        const int reduce = reduces ? reduces[c] : 0;
        if (reduce < 0 || reduce > r->max_reduce) return ICER_INVALID_INPUT;
        cuts->quota[c] = quotas[c]; cuts->reduce[c] = (uint8_t)reduce;
        *used |= 1u << reduce;
        top = std::max(top, quotas[c]);
    }
    if (out_stride < top) return ICER_INVALID_INPUT;
    if (data_bytes >= 0xFFFFFFFFull - 64u) return fail("batch of %zu stream bytes: 32-bit offsets only", data_bytes);
    return ICER_RESULT_OK;
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

// The byte-quota call and the cuts call.  by_resolution = false: the byte-quota call -- `reduces` is not looked at, every
// reduce is 0, and the workspace is its own smaller one (recut_layout), outside of which the kernels then touch nothing.
int recut_async(icerx_recutter *r, int n, const uint8_t *d_data, size_t data_bytes, const uint64_t *d_offsets, size_t stream_stride,
                const uint64_t *d_lens, bool by_resolution, const int *reduces, const size_t *quotas, int n_cuts, uint8_t *d_out,
                size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *workspace, size_t workspace_bytes, hipStream_t st)
{
    g_error.clear();
    if (by_resolution && !reduces) return ICER_INVALID_INPUT;
    RecutCuts cuts = {};
    uint32_t used = 0;
    int rc = recut_check(r, n, d_data, data_bytes, d_lens, by_resolution ? reduces : nullptr, quotas, n_cuts, d_out, out_stride, d_sizes,
                         d_rcs, workspace, &cuts, &used);
    if (rc != ICER_RESULT_OK) return rc;
    const RecutLayout L = recut_layout(r, n, data_bytes, n_cuts, by_resolution);
    if (workspace_bytes < L.total) return ICER_INVALID_INPUT;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *tab_off = (uint32_t *)(ws + L.blob.tab_off), *tab_bits = (uint32_t *)(ws + L.blob.tab_bits);
    uint64_t *foff = (uint64_t *)(ws + L.foff);
    const uint32_t n_full = r->red[0].n_units;
    const RecutCutTables tabs = recut_cut_tables(r);

    // 1. candidates over the blob
    if ((rc = enqueue_blob_stage(L.blob, ws, (size_t)n, r->geom.slots(), d_data, data_bytes, (const uint32_t *)r->crc, r->n_cus, st)) !=
        ICER_RESULT_OK)
        return rc;
    // 2. per frame: packet table, then every cut's walk with the tables of its geometry
    ICER_LAUNCH_ON(st, recut_plan_kernel, (unsigned)n, kRecutPlanThreads, kWalkLds, d_data, (uint32_t)data_bytes, d_offsets,
                   (uint64_t)stream_stride, d_lens, (const DCandRec *)(ws + L.blob.cands), (const AsyncHead *)(ws + L.blob.head), r->geom,
                   r->w, r->h, tabs, L.bits_stride, cuts, (uint32_t)n_cuts, used, tab_off, tab_bits, (uint32_t *)(ws + L.bits), foff,
                   by_resolution ? (uint64_t *)(ws + L.by_unit) : nullptr, (unsigned long long *)d_sizes, d_rcs);
    HIP_TRY(hipGetLastError());
    // 3. the kept packets, each with its cut's header
    ICER_LAUNCH_ON(st, recut_gather_kernel, dim3(n_full, (unsigned)n), kRecutGatherThreads, 0, d_data, d_offsets, (uint64_t)stream_stride,
                   r->geom, (const uint32_t *)r->red[0].unit_slot, n_full, tab_off, tab_bits, foff, cuts, (uint32_t)n_cuts,
                   (const uint32_t *)r->crc, d_out, out_stride);
    HIP_TRY(hipGetLastError());
done:
    return rc;
}

// icerx_recut_device_roi_async: the cuts call with a shift per cut and the frames' rectangles (`reduces` null: every reduce 0).
int recut_roi_async(icerx_recutter *r, int n, const uint8_t *d_data, size_t data_bytes, const uint64_t *d_offsets, size_t stream_stride,
                    const uint64_t *d_lens, const uint32_t *d_rois, const int *reduces, const int *shifts, const size_t *quotas, int n_cuts,
                    uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, uint32_t *d_kept, uint32_t *d_foreground,
                    void *workspace, size_t workspace_bytes, hipStream_t st)
{
    g_error.clear();
    if (!d_rois || !shifts || !d_kept || !d_foreground) return ICER_INVALID_INPUT;
    RecutCuts cuts = {};
    uint32_t used = 0;
    int rc = recut_check(r, n, d_data, data_bytes, d_lens, reduces, quotas, n_cuts, d_out, out_stride, d_sizes, d_rcs, workspace, &cuts, &used);
    if (rc != ICER_RESULT_OK) return rc;
    RecutRoiCuts pairs = {};
    for (int c = 0; c < n_cuts; c++) {
        if (shifts[c] < 0 || shifts[c] > kMaxRoiShift) return ICER_INVALID_INPUT;
        uint32_t p = 0;
        while (p < pairs.n_pairs && (pairs.pair_reduce[p] != cuts.reduce[c] || pairs.pair_shift[p] != (uint8_t)shifts[c])) p++;
        if (p == pairs.n_pairs) { pairs.pair_reduce[p] = cuts.reduce[c]; pairs.pair_shift[p] = (uint8_t)shifts[c]; pairs.n_pairs++; }
        pairs.pair[c] = (uint8_t)p;
    }
    const RecutRoiLayout L = recut_roi_layout(r, n, data_bytes, n_cuts);
    if (workspace_bytes < L.total) return ICER_INVALID_INPUT;
    uint8_t *ws = (uint8_t *)workspace;
    uint32_t *tab_off = (uint32_t *)(ws + L.cut.blob.tab_off), *tab_bits = (uint32_t *)(ws + L.cut.blob.tab_bits);
    uint32_t *unit_bits = (uint32_t *)(ws + L.cut.bits), *rank = (uint32_t *)(ws + L.rank), *order = (uint32_t *)(ws + L.order);
    uint32_t *fg = (uint32_t *)(ws + L.fg);
    uint64_t *foff = (uint64_t *)(ws + L.cut.foff);
    RecutRoiFrame *frames = (RecutRoiFrame *)(ws + L.frames);
    const uint32_t n_full = r->red[0].n_units;
    const RecutCutTables tabs = recut_cut_tables(r);
    RecutRoiPrio prio = {};
    for (int k = 0; k <= r->max_reduce; k++) prio.p[k] = (const uint64_t *)r->red[k].prio;

    // 1. candidates over the blob
    if ((rc = enqueue_blob_stage(L.cut.blob, ws, (size_t)n, r->geom.slots(), d_data, data_bytes, (const uint32_t *)r->crc, r->n_cus, st)) !=
        ICER_RESULT_OK)
        return rc;
    // 2. per frame: packet table, bit counts, the clipped rectangle
    ICER_LAUNCH_ON(st, recut_roi_frame_kernel, (unsigned)n, kRecutPlanThreads, kWalkLds, d_data, (uint32_t)data_bytes, d_offsets,
                   (uint64_t)stream_stride, d_lens, (const DCandRec *)(ws + L.cut.blob.cands), (const AsyncHead *)(ws + L.cut.blob.head),
                   r->geom, r->w, r->h, tabs, L.cut.bits_stride, used, d_rois, tab_off, tab_bits, unit_bits, frames);
    HIP_TRY(hipGetLastError());
    // 3. per frame and distinct (reduce, shift): the ROI order
    ICER_LAUNCH_ON(st, recut_roi_rank_kernel, dim3((unsigned)n, pairs.n_pairs), kRecutRankThreads, sizeof(RoiShared), tabs, prio, pairs,
                   (const RecutRoiFrame *)frames, r->w, r->h, n_full, (uint64_t *)(ws + L.keys), rank, order, fg);
    HIP_TRY(hipGetLastError());
    // 4. per frame and cut: the walk along that order
    ICER_LAUNCH_ON(st, recut_roi_scan_kernel, dim3((unsigned)n, (unsigned)n_cuts), kRecutScanThreads, 0, tabs, L.cut.bits_stride, cuts, pairs,
                   (const RecutRoiFrame *)frames, (const uint32_t *)unit_bits, (const uint32_t *)rank, (const uint32_t *)order,
                   (const uint32_t *)fg, (uint32_t *)(ws + L.pbits), foff, (uint64_t *)(ws + L.cut.by_unit),
                   (unsigned long long *)d_sizes, d_rcs, d_kept, d_foreground);
    HIP_TRY(hipGetLastError());
    // 5. the kept packets, each with its cut's header
    ICER_LAUNCH_ON(st, recut_gather_kernel, dim3(n_full, (unsigned)n), kRecutGatherThreads, 0, d_data, d_offsets, (uint64_t)stream_stride,
                   r->geom, (const uint32_t *)r->red[0].unit_slot, n_full, tab_off, tab_bits, foff, cuts, (uint32_t)n_cuts,
                   (const uint32_t *)r->crc, d_out, out_stride);
    HIP_TRY(hipGetLastError());
done:
    return rc;
}

// the three tables of a plan on the device; slot[u]: the slot of unit u in the packet table of `geom`, levels raised by `reduce`
int recut_upload_plan(const Plan &plan, const DPlanGeom &geom, uint32_t reduce, std::vector<uint32_t> *slot, void **unit_slot,
                      void **final_order, void **units)
{
    int rc = ICER_RESULT_OK;
    slot->resize(plan.units.size());
    for (size_t u = 0; u < plan.units.size(); u++) {
        const UnitDesc &d = plan.units[u];
        (*slot)[u] = geom.slot(d.chan, d.level + reduce, d.subband, d.seg, d.lsb);
    }
    HIP_TRY(recut_upload(unit_slot, slot->data(), sizeof(uint32_t) * slot->size()));
    HIP_TRY(recut_upload(final_order, plan.final_order.data(), sizeof(uint32_t) * plan.final_order.size()));
    HIP_TRY(recut_upload(units, plan.units.data(), sizeof(UnitDesc) * plan.units.size()));
done:
    return rc;
}

// quality: a quality recutter for masters made with filter `filt` (recut_quality.hpp); its tables are built and checked on the
// host before anything is allocated
int recutter_create(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, unsigned segments, int sample_bits,
                    int max_reduce, bool quality = false, int filt = -1)
{
    g_error.clear();
    if (!out) return ICER_INVALID_INPUT;
    *out = nullptr;
    if (sample_bits != 8 && sample_bits != 16) return ICER_INVALID_INPUT;
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
    if (quality)
        if (const int qrc = recut_quality_build(plans, geom, filt, sample_bits, &qual)) return qrc;
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
    HIP_TRY(recut_upload(&r->crc, crc_tab, sizeof crc_tab));
    for (int k = 0; k <= max_reduce; k++) {
        icerx_recutter::Reduced &g = r->red[k];
        g.n_units = (uint32_t)plans[k].units.size();
        r->units_total += g.n_units;
        if ((rc = recut_upload_plan(plans[k], r->geom, (uint32_t)k, &slot, &g.unit_slot, &g.final_order, &g.units)) != ICER_RESULT_OK) goto done;
        if (!roi_priorities(plans[k], &prio)) {        // (no geometry the planner accepts gets here: make_packets keeps the bound and the order)
            rc = fail("recutter: the packet priorities of the geometry at 1/2^%d size do not fit the sort keys", k);
            goto done;
        }
        HIP_TRY(recut_upload(&g.prio, prio.data(), sizeof(uint64_t) * prio.size()));
        if (k == 0) { slot0 = slot; continue; }
        std::vector<uint32_t> of_slot(r->geom.slots(), kNoPacket), full_to_cut(slot0.size());
        for (size_t u = 0; u < slot.size(); u++) of_slot[slot[u]] = (uint32_t)u;
        for (size_t u = 0; u < slot0.size(); u++) full_to_cut[u] = of_slot[slot0[u]];
        HIP_TRY(recut_upload(&g.full_to_cut, full_to_cut.data(), sizeof(uint32_t) * full_to_cut.size()));
    }
    if (quality) {
        r->filt = filt;
        if ((rc = recut_quality_upload(r, qual)) != ICER_RESULT_OK) goto done;
    }
    *out = r;
    return ICER_RESULT_OK;
done:
    icerx_recutter_destroy(r);
    return rc;
}

}  // namespace

extern "C" {

void icerx_recutter_destroy(icerx_recutter *r)
{
    if (!r) return;
    if (r->crc) (void)hipFree(r->crc);
    for (int k = 0; k <= kRecutMaxReduce; k++)
        for (void *p : {r->red[k].unit_slot, r->red[k].final_order, r->red[k].units, r->red[k].full_to_cut, r->red[k].prio})
            if (p) (void)hipFree(p);
    for (int k = 0; k <= kRecutMaxReduce; k++)
        for (void *p : {r->qual[k].weight, r->qual[k].chan, r->qual[k].ll_term, r->qual[k].fam_map})
            if (p) (void)hipFree(p);
    if (r->fam_cap) (void)hipFree(r->fam_cap);
    delete r;
}

int icerx_recutter_create(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, unsigned segments,
                          int sample_bits)
{
    return recutter_create(out, device, w, h, channels, stages, segments, sample_bits, 0);
}

int icerx_recutter_create_reduced(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, unsigned segments,
                                  int sample_bits, int max_reduce)
{
    return recutter_create(out, device, w, h, channels, stages, segments, sample_bits, max_reduce);
}

int icerx_recutter_max_reduce(const icerx_recutter *r) { return r ? r->max_reduce : 0; }

size_t icerx_recut_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_quotas)
{
    if (!r || n <= 0 || n_quotas < 1 || n_quotas > kMaxLadder) return 0;
    return recut_layout(r, n, data_bytes, n_quotas, false).total;
}

int icerx_recut_device_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                             size_t stream_stride, const uint64_t *d_lens, const size_t *quotas, int n_quotas, uint8_t *d_out,
                             size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return recut_async(r, n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, false, nullptr, quotas, n_quotas, d_out,
                       out_stride, d_sizes, d_rcs, d_workspace, workspace_bytes, (hipStream_t)stream);
}

size_t icerx_recut_cuts_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts)
{
    if (!r || n <= 0 || n_cuts < 1 || n_cuts > kMaxLadder) return 0;
    return recut_layout(r, n, data_bytes, n_cuts, true).total;
}

int icerx_recut_device_cuts_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                  size_t stream_stride, const uint64_t *d_lens, const int *reduces, const size_t *quotas, int n_cuts,
                                  uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *d_workspace,
                                  size_t workspace_bytes, void *stream)
{
    return recut_async(r, n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, true, reduces, quotas, n_cuts, d_out,
                       out_stride, d_sizes, d_rcs, d_workspace, workspace_bytes, (hipStream_t)stream);
}

size_t icerx_recut_roi_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts)
{
    if (!r || n <= 0 || n_cuts < 1 || n_cuts > kMaxLadder) return 0;
    return recut_roi_layout(r, n, data_bytes, n_cuts).total;
}

int icerx_recut_device_roi_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                 size_t stream_stride, const uint64_t *d_lens, const uint32_t *d_rois, const int *reduces,
                                 const int *shifts, const size_t *quotas, int n_cuts, uint8_t *d_out, size_t out_stride,
                                 uint64_t *d_sizes, int32_t *d_rcs, uint32_t *d_kept, uint32_t *d_foreground, void *d_workspace,
                                 size_t workspace_bytes, void *stream)
{
    return recut_roi_async(r, n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, d_rois, reduces, shifts, quotas, n_cuts,
                           d_out, out_stride, d_sizes, d_rcs, d_kept, d_foreground, d_workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
