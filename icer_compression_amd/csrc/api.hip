// api.hip -- C ABI of libicer_hip.so (declared in include/icer_hip.h) and the host-side pipeline
// driver.  The reference's drivers icer_compress_image_uint16 (lib_icer/src/icer_compress.c:279-426)
// and icer_compress_image_yuv_uint16 (icer_color.c:343-530) become: upload -> DWT stages -> LL mean
// -> sign-magnitude -> one launch that codes every (frame, unit) -> quota scan -> gather.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <sched.h>
#include <time.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/icer_hip.h"
#include "kernels.hpp"
#include "launch_plan.hpp"
#include "subband_gain.hpp"

using namespace icer;

namespace {
bool want_priority_streams();      // (defined with the host-fed batch, below)
}
namespace {

thread_local std::string g_last_error;
static std::atomic<uint64_t> g_stats[3];      // unit time-outs, fallback batches, slot re-runs (icerx_process_stats)
CoderTables g_tables;
bool g_tables_ready = false;
std::recursive_mutex g_mutex;

void set_error(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    fprintf(stderr, "icer_hip: %s\n", buf);
}

// polite spin (the wait for a batch is tens of milliseconds; see wait_event)
static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#endif
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return ICER_FATAL_ERROR;                                                          \
        }                                                                                     \
    } while (0)

template <class T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0;      // elements
    int ensure(size_t want)
    {
        if (want <= n) return 0;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e));
            return ICER_FATAL_ERROR;
        }
        n = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// Logical devices.  ICER_HIP_VIRTUAL_DEVICES=<N> makes the library present N devices whatever the node has: logical device
// d runs on physical device d % (devices present).  A dry run of every multi-device code path -- N host threads, N sets of
// pooled encoders / streams / staging buffers, error aggregation -- on a box with a single GPU (tests, bench.py --gpus N
// on one GPU); the streams are the same as with real devices, only slower.  Unset: logical = physical.
int physical_device_count()
{
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}
int virtual_device_count()
{
    const char *v = getenv("ICER_HIP_VIRTUAL_DEVICES");
    const int n = v ? atoi(v) : 0;
    return n >= 1 && n <= 64 ? n : 0;
}
int logical_device_count()
{
    const int phys = physical_device_count(), virt = virtual_device_count();
    return phys > 0 && virt > 0 ? virt : phys;
}
int physical_of(int logical)
{
    const int phys = physical_device_count();
    return phys > 0 && virtual_device_count() > 0 ? logical % phys : logical;
}

// The host cores next to a GPU: the NUMA node of its PCI function (/sys/bus/pci/devices/<bus id>/numa_node) and that
// node's cpulist.  A per-device worker thread of a host batch pins itself there before it allocates its page-locked
// staging words, so that first touch puts them on that node and its polling does not cross sockets
// (ICER_HIP_NUMA=0: off).  Best effort: any failure leaves the thread where it was.
bool pin_thread_near_device(int physical)
{
    if (const char *v = getenv("ICER_HIP_NUMA")) if (atoi(v) == 0) return false;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, physical) != hipSuccess) { (void)hipGetLastError(); return false; }
    for (char *c = bus; *c; c++) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return false;
    int node = -1;
    const int got = fscanf(f, "%d", &node);
    fclose(f);
    if (got != 1 || node < 0) return false;           // (-1: the platform reports no affinity)
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return false;
    char list[1024] = {0};
    const bool ok = fgets(list, sizeof list, f) != nullptr;
    fclose(f);
    if (!ok) return false;
    cpu_set_t set;
    CPU_ZERO(&set);
    int n_set = 0;
    for (const char *c = list; *c;) {                   // "0-15,64-79"
        char *end = nullptr;
        const long lo = strtol(c, &end, 10);
        if (end == c) break;
        long hi = lo;
        c = end;
        if (*c == '-') { hi = strtol(c + 1, &end, 10); c = end; }
        for (long k = lo; k <= hi && k < CPU_SETSIZE; k++) { CPU_SET((int)k, &set); n_set++; }
        while (*c == ',' || *c == '\n' || *c == ' ') c++;
    }
    if (n_set == 0) return false;
    // never widen what the caller was given (taskset, numactl, cgroup cpusets, isolcpus): the node's cores AND the thread's
    // current mask; an empty intersection leaves the thread where it is
    cpu_set_t cur;
    CPU_ZERO(&cur);
    if (sched_getaffinity(0, sizeof cur, &cur) != 0) return false;
    CPU_AND(&set, &set, &cur);
    if (CPU_COUNT(&set) == 0) return false;
    return sched_setaffinity(0, sizeof set, &set) == 0;
}

// The quotas of a rate ladder call (icerx_encode_device_ladder): the batch is planned and coded for the largest one, and each
// quota's stream is cut from it (assemble_ladder.hpp).  A ladder of one quota is an ordinary call at that quota.
struct Ladder {
    LadderQuotas quotas;
    int n = 0;              // quotas
    int pitch = 0;          // frames of the call: the rows of one quota's block of the output
};
static_assert(kMaxLadder == ICERX_MAX_LADDER, "assemble_ladder.hpp and include/icer_hip.h agree on the ladder's length");
static_assert(kMaxRoiShift == ICERX_MAX_ROI_SHIFT, "roi_core.hpp and include/icer_hip.h agree on the largest shift");

// The targets of a quality-targeted call (icerx_encode_device_target): the batch is planned and coded as a call at the byte cap, and
// each target's stream is cut from it where the target is met (distortion_core.hpp).  Output rows are target-major, as a ladder's.
struct Target {
    TargetList thresholds;
    int n = 0;              // targets
    int pitch = 0;          // frames of the call
    int32_t *d_reached = nullptr;                   // per (target, frame), of the call's first frame
    unsigned long long *d_dist = nullptr, *d_equiv = nullptr;
};

// The budgets of a budget call (icerx_encode_device_budget): planned and coded as a target call at the byte cap; the frames' cuts at each
// budget come from one search over all frames of the call (budget_core.hpp).  Output rows are budget-major.  Every pointer is of the
// call's first frame: the search runs once, whatever parts the call is enqueued in.
struct Budget {
    BudgetList budgets;
    int n = 0;              // budgets
    int n_frames = 0;       // frames of the call
    int32_t *d_at_cap = nullptr;
    unsigned long long *d_dist = nullptr, *d_equiv = nullptr, *d_threshold = nullptr, *d_total = nullptr;
};

// A region-of-interest call (icerx_encode_device_roi): a ladder call -- planned and coded for the largest quota, with every unit coded --
// whose streams are cut along each frame's ROI order (roi_core.hpp).  Output rows are quota-major.  Every pointer is of the call's first frame.
struct Roi {
    LadderQuotas quotas;
    int n = 0;              // quotas
    int pitch = 0;          // frames of the call
    uint32_t shift = 0;
    const uint32_t *d_rois = nullptr;               // per frame: x, y, w, h
    uint32_t *d_kept = nullptr, *d_foreground = nullptr;
};

// One encode call, as every layer between the C ABI and the kernels takes it: device pointers of its first frame, everything on `stream`.
struct EncodeCall {
    const uint16_t *d_frames; int n_frames; size_t quota;               // (a ladder call: its largest quota)
    uint8_t *d_out; size_t out_stride; uint64_t *d_sizes; int32_t *d_rcs;
    hipStream_t stream;
    bool overlap_ok;                    // the call may be enqueued in parts on two streams (the synchronous entry points; plan_launch)
    const Ladder *ladder = nullptr;     // a rate ladder call: the frames are cut at each of its quotas, into their rows of every quota's block.  It lives on the
                                        // stack of icerx_encode_device_ladder, a synchronous call: a call left in icerx_encoder::Pending never has one
    const Target *target = nullptr;     // a quality-targeted call (quota = its byte cap): the same, on the stack of icerx_encode_device_target
    const Budget *budget = nullptr;     // a budget call (quota = its byte cap): the same, on the stack of icerx_encode_device_budget
    const Roi *roi = nullptr;           // a region-of-interest call (quota = its largest quota): the same, on the stack of icerx_encode_device_roi
    // the same call for its frames [f0, f0 + n), `frame_elems` samples each
    EncodeCall frames(int f0, int n, size_t frame_elems) const
    {
        return EncodeCall{d_frames + (size_t)f0 * frame_elems, n, quota, d_out + (size_t)f0 * out_stride, out_stride, d_sizes + f0, d_rcs + f0, stream, overlap_ok, ladder, target, budget, roi};
    }
};

}  // namespace

struct icerx_encoder {
    int device = 0;                     // physical HIP device (hipSetDevice)
    int logical_device = 0;             // what the caller named (ICER_HIP_VIRTUAL_DEVICES maps several onto one)
    size_t w = 0, h = 0;
    int channels = 1, stages = 0, filt = 0, segments = 0, max_frames = 0;
    int sample_bits = 16;               // 8: the uint8 twins (int8 storage, 7 bit planes)
    Plan plan;
    Tuning tuning;                      // read from the environment at create (launch_plan.hpp)
    size_t slot_quota = (size_t)-1;     // quota the current slot table was built for
    unsigned bits_per_pixel = 3;        // slot bound; doubled on overflow
    bool units_uploaded = false;
    bool wg_once = false;               // the next enqueue uses the window coder whatever the mode (after a unit time-out)
    int n_cus = 256;                    // compute units of the device
    uint64_t n_timeouts = 0, n_fallbacks = 0, n_slot_retries = 0;   // icerx_encoder_stats
    uint64_t n_routed_units = 0, n_routed_launches = 0;             // icerx_encoder_routing
    LaunchPlan last_plan;               // what the last enqueue launched

    DevBuf<int16_t> coef, tmp;
    DevBuf<unsigned long long> sums;
    DevBuf<uint16_t> means;
    DevBuf<int> flags;                  // status words of a batch: dwt_ovf .. bound_ovf below
    DevBuf<UnitDesc> units;
    DevBuf<uint32_t> work_order, final_order, unit_bits, done_bytes;
    DevBuf<uint64_t> final_off;
    DevBuf<uint8_t> slots;
    DevBuf<uint8_t> sig;                // chunk tables (family_events_kernel), max_frames * plan.sig_bytes
    DevBuf<uint32_t> sig_hist;          // per frame and family: chunks by the bit plane from which they are blank, 16 entries (family_events_kernel -> route_units_kernel)
    DevBuf<uint32_t> sig_blocks;        // Plan::sig_blocks on the device
    DevBuf<uint8_t> events;             // event bytes (events.hpp): max_frames x bit planes x plan.sig_bytes chunks x 64, allocated at create unless ICER_HIP_CODER=wg
    DevBuf<uint8_t> route;              // max_frames * units: the coder of each unit when both share a launch
    DevBuf<uint32_t> route_list, route_ctl;   // the units of the workgroup coder (frame * units + unit), [length, cursor]
    // sub-range splitting (coder_core.hpp "Sub-ranges"): a launch of one gray frame cuts its dense units into pieces, one workgroup each
    DevBuf<SubDesc> subs;
    DevBuf<uint32_t> sub_order, snap_valid;
    DevBuf<Snapshot> snaps;
    DevBuf<SubRecord> sub_recs;
    hipStream_t side_stream = nullptr;  // the list kernel runs beside the pipeline kernel
    bool side_stream_borrowed = false;  // ... on a stream another encoder owns (the pooled encoders of a host batch share one)
    hipEvent_t fork[kMaxParts] = {}, join[kMaxParts] = {};   // per part of a batch (enqueue): list kernel on the side stream
    hipStream_t half_stream = nullptr;  // the odd parts of a batch coded by a synchronous call (enqueue)
    hipEvent_t part_fork = nullptr, part_join = nullptr;
    hipEvent_t coef_ready = nullptr;    // the transform of the last enqueue is complete (coef, means, frame status): recorded before the coder
    hipStream_t io_stream = nullptr, copy_stream = nullptr;   // lib_icer-shaped entry points: their encode stream, and the coefficient write-back beside the coder
    DevBuf<CoderTables> tables;
    // host-API staging
    DevBuf<uint16_t> in;
    DevBuf<uint8_t> in8;
    DevBuf<uint8_t> out;
    DevBuf<unsigned long long> sizes;
    DevBuf<int32_t> rcs;
    DevBuf<uint64_t> prof;              // profiling build only (-DICER_PHASE_TIMERS): per-phase cycle sums
    // quality-targeted calls (distortion_core.hpp): made by the first icerx_encode_device_target, nothing before
    DevBuf<unsigned long long> dist;    // E[max_frames][plan.n_families][planes + 1]: the families' residual energies of the last target call
    DevBuf<uint32_t> fam_weight;        // the subband weight of each family (subband_gain.hpp)
    DevBuf<uint32_t> fam_chan;          // its channel
    DevBuf<unsigned long long> fam_ll_term;   // weight x coefficients of an LL family of a 16-bit encoder, else 0 (distortion_core.hpp mean_loss)
    hipEvent_t energy_fork[kMaxParts] = {}, energy_join[kMaxParts] = {};   // per part: the energy pass on the side stream
    int dist_frames = 0;                // frames of the last target or budget call (icerx_get_distortion_table)
    // budget calls (budget_core.hpp): made by the first icerx_encode_device_budget, nothing before
    DevBuf<unsigned long long> curve;   // D_k, then used_k: 2 x max_frames x (units + 1)
    DevBuf<uint32_t> curve_head;        // max_frames x kCurveHeadWords
    DevBuf<BudgetState> budget_state;   // the search's scratch for calls of more than kBudgetLdsFrames frames: kMaxLadder x max_frames

    // region-of-interest calls (roi_core.hpp): made by the first icerx_encode_device_roi, nothing before
    DevBuf<uint64_t> roi_prio;          // the priority of every unit's packet
    DevBuf<uint64_t> roi_keys;          // roi_rank_kernel's scratch: max_frames x units
    DevBuf<uint32_t> roi_rank, roi_order;   // max_frames x units
    DevBuf<uint32_t> roi_bits;          // scan_roi_kernel's scratch, laid out as final_off: quotas x max_frames x units

    int *h_flag = nullptr;              // pinned host words: slot-bound overflow flag of the last batch, units on its route list
    hipEvent_t done = nullptr;          // end of the last batch on its stream
    bool wg_available = true;           // the workgroup coder's LDS block (> 64 KiB) was granted: progressive mode, hybrid launches, time-out fall-back
    bool sleepy_wait = false;           // waits yield the core between polls (the per-device workers of a host batch) instead of spinning
    struct Pending {                    // icerx_encode_device_async .. icerx_encoder_wait
        bool active = false;
        EncodeCall call = {};
    } pend;

    bool timing = false;
    hipEvent_t ev[ICERX_NUM_STAGES + 1] = {};
    double ms[ICERX_NUM_STAGES] = {};
    uint64_t timed_calls = 0;
    bool ev_pending = false;

    // `flags`, with P = max_frames * channels planes and F = max_frames frames:
    //     [0, P) the transform left the sample range   [P, 2P) the LL mean did   [2P, 2P + F) the frame is skipped (either of the two, any channel)
    //     [2P + F] a coding unit of the batch outgrew its slot (bit 0) or timed out (bit 1)
    // per plane / frame from frame f0 on
    int *dwt_ovf(int f0) const { return flags.p + (size_t)f0 * channels; }
    int *mean_ovf(int f0) const { return flags.p + (size_t)max_frames * channels + (size_t)f0 * channels; }
    int *skip(int f0) const { return flags.p + 2 * (size_t)max_frames * channels + f0; }
    int *bound_ovf() const { return flags.p + 2 * (size_t)max_frames * channels + max_frames; }
};

namespace {

// What a launch must find zeroed -- status flags, LL sums, histograms, list cursors, sub-range records -- in ONE small kernel instead
// of a fill per range (round 6: a lone frame had nine fills of ~ 4 us each in front of its transform, + their dispatch gaps).
struct ClearList {
    static constexpr int kMax = 10;
    uint32_t *p[kMax];
    uint32_t words[kMax];
    int n = 0;
    bool add(void *ptr, size_t bytes)         // false: the range does not fit (whole words, at most kMax ranges of fewer than 2^32 words)
    {
        if (bytes && (n == kMax || bytes % 4 || bytes / 4 > UINT32_MAX)) return false;
        if (bytes) { p[n] = static_cast<uint32_t *>(ptr); words[n] = (uint32_t)(bytes / 4); n++; }
        return true;
    }
};
__global__ void __launch_bounds__(256) clear_ranges_kernel(ClearList cl)
{
    uint32_t *p = cl.p[blockIdx.y];
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < cl.words[blockIdx.y]; i += gridDim.x * 256u) p[i] = 0u;
}
static void launch_clears(const ClearList &cl, hipStream_t st)
{
    if (cl.n) hipLaunchKernelGGL(clear_ranges_kernel, dim3(8, (unsigned)cl.n), dim3(256), 0, st, cl);
}

__global__ void frame_status_kernel(const int *dwt_ovf, const int *mean_ovf, int channels, int n_frames, int *skip)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    int s = 0;
    for (int c = 0; c < channels; c++) s |= dwt_ovf[f * channels + c] | mean_ovf[f * channels + c];
    skip[f] = s;
}

// uint8 twins: the samples are int8 storage (icer_wavelet.c:231 `int8_t *signed_data = (int8_t *) data`); the kernels
// work on them sign-extended to int16
__global__ void __launch_bounds__(256) widen_s8_kernel(const uint8_t *__restrict__ src, uint16_t *__restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = (uint16_t)(int16_t)(int8_t)src[i];
}

// uint8 twins, the way back: the coder's 16-bit sign-magnitude words as the int8 sign-magnitude bytes the reference leaves in
// the caller's image (icer_wavelet.c:852-858)
__global__ void __launch_bounds__(256) narrow_sm8_kernel(const uint16_t *__restrict__ src, uint8_t *__restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t v = src[i];
        dst[i] = (uint8_t)(((v >> 8) & 0x80u) | (v & 0x7Fu));
    }
}

// 8-bit gray -> uint16 (what the reference's CLI does on the host, example/src/icer_util.c:163-168)
__global__ void __launch_bounds__(256) widen_u8_kernel(const uint8_t *__restrict__ src, uint16_t *__restrict__ dst, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// packed RGB888 -> Y, Cb, Cr planes, integer formulas of the reference's callers (color_util.h:8,27-29)
__global__ void __launch_bounds__(256)
rgb8_to_ycbcr_kernel(const uint8_t *__restrict__ rgb, uint16_t *__restrict__ planes, size_t npix, int n_frames)
{
    const size_t total = npix * (size_t)n_frames;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t f = i / npix, p = i - f * npix;
        const int r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        auto clip = [](int v) { return v > 255 ? 255 : (v < 0 ? 0 : v); };
        const int y = clip((19595 * r + 38470 * g + 7471 * b) >> 16);
        const int cb = clip(((36962 * (b - y)) >> 16) + 128);
        const int cr = clip(((46727 * (r - y)) >> 16) + 128);
        uint16_t *o = planes + f * 3 * npix + p;
        o[0] = (uint16_t)y;
        o[npix] = (uint16_t)cb;
        o[2 * npix] = (uint16_t)cr;
    }
}

LaunchShape launch_shape(const icerx_encoder *e) { return LaunchShape{e->channels, e->max_frames, e->w, e->h, e->n_cus, (uint32_t)e->plan.subs.size()}; }

int upload_units(icerx_encoder *e, size_t quota, hipStream_t st)
{
    if (e->units_uploaded && e->slot_quota == quota) return 0;
    uint32_t split_chunks = 0;          // (ICER_HIP_SPLIT unset: by geometry)
    if (plans_sub_ranges(launch_shape(e), e->tuning, e->wg_available))
        split_chunks = e->tuning.split_chunks == 1 ? auto_split_chunks(e->plan.units, e->n_cus, e->sample_bits == 8 ? kPlanes8 : kPlanes) : (uint32_t)e->tuning.split_chunks;
    assign_slots(&e->plan, quota, e->bits_per_pixel, split_chunks);
    const size_t n = e->plan.units.size();
    if (!e->plan.subs.empty()) {
        if (e->subs.ensure(e->plan.subs.size()) || e->sub_order.ensure(e->plan.split_launch.size())) return ICER_FATAL_ERROR;
        HIP_TRY(hipMemcpyAsync(e->subs.p, e->plan.subs.data(), e->plan.subs.size() * sizeof(SubDesc), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(e->sub_order.p, e->plan.split_launch.data(), e->plan.split_launch.size() * 4, hipMemcpyHostToDevice, st));
    }
    if (e->units.ensure(n) || e->work_order.ensure(n) || e->final_order.ensure(n)) return ICER_FATAL_ERROR;
    HIP_TRY(hipMemcpyAsync(e->units.p, e->plan.units.data(), n * sizeof(UnitDesc), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->work_order.p, e->plan.work_order.data(), n * 4, hipMemcpyHostToDevice, st));
    if (e->sig_blocks.ensure(e->plan.sig_blocks.size() + 1)) return ICER_FATAL_ERROR;
    HIP_TRY(hipMemcpyAsync(e->sig_blocks.p, e->plan.sig_blocks.data(), e->plan.sig_blocks.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->final_order.p, e->plan.final_order.data(), n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));       // the host vectors may change on the next re-plan
    e->slot_quota = quota;
    e->units_uploaded = true;
    return 0;
}

int accumulate_timing(icerx_encoder *e)
{
    if (!e->ev_pending) return 0;
    HIP_TRY(hipEventSynchronize(e->ev[ICERX_NUM_STAGES]));
    for (int i = 0; i < ICERX_NUM_STAGES; i++) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, e->ev[i], e->ev[i + 1]));
        e->ms[i] += t;
    }
    e->timed_calls++;
    e->ev_pending = false;
    return 0;
}

// The forward DWT of a batch: one fused tile pass per stage.  Stage 0 reads the caller's frames; every stage writes
// HL/LH/HH to their final place in `coef` (as the coder's sign-magnitude words when `sm` != 0) and its LL band to a
// compact side buffer in `tmp` that the next stage reads (the last stage writes LL into `coef`), so no workgroup reads
// what another one of the same stage writes.  *cw, *ch: in the frame size, out the LL size.
void launch_dwt(icerx_encoder *e, const uint16_t *d_frames, int n_frames, hipStream_t st, int sm, int *dwt_ovf, size_t *cw_io, size_t *ch_io,
                int16_t *coef = nullptr, int16_t *tmp = nullptr)
{
    if (!coef) coef = e->coef.p;            // (a part of a batch: its own planes of the encoder's buffers, enqueue_part)
    if (!tmp) tmp = e->tmp.p;
    const size_t W = e->w, plane = W * e->h;
    const int P = n_frames * e->channels;
    size_t cw = *cw_io, ch = *ch_io, ll_off = 0;
    DwtStageArgs da;
    da.f = filter_taps(e->filt);
    da.lim = e->sample_bits == 8 ? 127 : 32767;
    da.sm = sm;
    da.coef = coef; da.coef_stride = (uint32_t)W;
    da.src = reinterpret_cast<const int16_t *>(d_frames); da.src_stride = (uint32_t)W;
    size_t src_plane = plane;
    for (int s = 0; s < e->stages; s++) {
        const int nlw = (int)((cw + 1) / 2), nlh = (int)((ch + 1) / 2);
        da.cw = (int)cw; da.ch = (int)ch;
        size_t ll_plane;
        if (s == e->stages - 1) { da.ll = coef; da.ll_stride = (uint32_t)W; ll_plane = plane; }
        else { da.ll = tmp + ll_off; da.ll_stride = (uint32_t)nlw; ll_plane = plane; }
        hipLaunchKernelGGL(dwt_tile_kernel, dim3((nlw + kTileKX - 1) / kTileKX, (nlh + kTileKY - 1) / kTileKY, P),
                           dim3(kTileThreads), 0, st, da, src_plane, plane, ll_plane, dwt_ovf);
        da.src = da.ll; da.src_stride = da.ll_stride; src_plane = ll_plane;
        ll_off += (size_t)nlw * nlh;
        cw = nlw;
        ch = nlh;
    }
    *cw_io = cw; *ch_io = ch;
}

// The stream the list kernel runs on beside the pipeline kernel of the same launch: the two must not share a hardware queue.  With
// hardware queues to spare (GPU_MAX_HW_QUEUES >= 6) a plain stream; otherwise a HIGH-priority one -- the runtime keeps a pool of queues
// per priority level, so it can never be given the queue of the caller's (normal-priority) stream, however many streams the process
// has alive (want_priority_streams).
// a stream of the level `which` names ("high" / "low"; anything else, or a runtime without levels: a plain stream)
hipError_t create_level_stream(hipStream_t *st, const char *which)
{
    int least = 0, greatest = 0;
    if (which && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least) {
        const bool hi = !strcmp(which, "high"), lo = !strcmp(which, "low");
        if ((hi || lo) && hipStreamCreateWithPriority(st, hipStreamNonBlocking, hi ? greatest : least) == hipSuccess) return hipSuccess;
    }
    (void)hipGetLastError();
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}
hipError_t create_side_stream(hipStream_t *st)
{
    return create_level_stream(st, want_priority_streams() ? "high" : nullptr);
}
// the per-part events of an encoder and, for encoders of several frames, the stream of a batch's odd parts (enqueue)
hipError_t create_part_events(icerx_encoder *e)
{
    for (int k = 0; k < kMaxParts; k++) {
        hipError_t r = hipEventCreateWithFlags(&e->fork[k], hipEventDisableTiming);
        if (r == hipSuccess) r = hipEventCreateWithFlags(&e->join[k], hipEventDisableTiming);
        if (r != hipSuccess) return r;
    }
    if (wants_half_stream(launch_shape(e), e->tuning)) {
        hipError_t r = hipEventCreateWithFlags(&e->part_fork, hipEventDisableTiming);
        if (r == hipSuccess) r = hipEventCreateWithFlags(&e->part_join, hipEventDisableTiming);
        if (r == hipSuccess) r = hipStreamCreateWithFlags(&e->half_stream, hipStreamNonBlocking);
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}
// The host-fed pipeline of a device has four streams whose kernels must overlap (three encoders + the side stream they share).  When
// hardware queues are scarce they go to the LOW level's pool together: measured with the runtime's default queues on C4 / C5, quiet
// process or crowded -- low 0.93-0.95 x the device-resident rate (what 8 queues and plain streams give), high 0.89-0.90 x (high-priority
// compute gets in the way of the copy streams' transfers), plain streams 0.68-0.71 x; the copy streams stay plain
// (profiles/r05_logs/r05_r.log, r05_t.log).  Low priority also means what it says: kernels of the host program's own streams go first.
const char *pool_compute_level() { const char *v = getenv("ICER_HIP_COMPUTE_LEVEL"); return v ? v : "low"; }

#ifndef ICER_LONE_PAD_BYTES
#define ICER_LONE_PAD_BYTES 12288
#endif
constexpr int kLonePadBytes = ICER_LONE_PAD_BYTES;      // LDS padding of the pipeline's workgroups in a split launch (launch_plan.hpp PipeKernel::Lone)
static_assert(kUnitWavesSmall == 8 && kUnitWavesLarge == 11, "launch_plan.hpp names the pipeline's shapes by these wave counts");

// The end of a budget call, once per call on its stream behind the curve passes of all its parts: the search -- one workgroup per budget
// over all frames -- and the gather of every budget's streams.  `c`: the whole call.
int enqueue_budget_tail(icerx_encoder *e, const EncodeCall &c)
{
    const Budget &b = *c.budget;
    const uint32_t n_units = (uint32_t)e->plan.units.size();
    const size_t off_pitch = (size_t)e->max_frames * n_units, curve_pitch = (size_t)n_units + 1u;
    hipLaunchKernelGGL(budget_search_kernel, dim3(b.n), dim3(64 * kBudgetWaves), 0, c.stream, e->curve.p, e->curve.p + (size_t)e->max_frames * curve_pitch,
                       e->curve_head.p, n_units, (uint32_t)b.n_frames, b.budgets, (uint64_t)c.quota, e->unit_bits.p, e->final_order.p, e->skip(0), e->units.p,
                       e->final_off.p, off_pitch, reinterpret_cast<unsigned long long *>(c.d_sizes), c.d_rcs, b.d_at_cap, b.d_dist, b.d_equiv, b.d_threshold,
                       b.d_total, e->bound_ovf(), e->budget_state.p);
    hipLaunchKernelGGL(gather_ladder_kernel, dim3(n_units, b.n_frames), dim3(256), 0, c.stream, e->slots.p, e->plan.slot_bytes, e->units.p, n_units,
                       e->unit_bits.p, e->final_off.p, off_pitch, (uint32_t)b.n, c.d_out, c.out_stride, (uint32_t)b.n_frames);
    HIP_TRY(hipGetLastError());
    return 0;
}

// enqueue the whole pipeline for part `part` of the launch `lp` -- the frames [f0, f0 + n_frames) of a batch; `c` is the call for those
// frames, on the part's stream -- ; every per-frame buffer of the encoder is used from frame f0 on, so that parts of a batch can
// be in flight on different streams (enqueue).  `part` also names the set of per-launch resources (route list cursor, fork / join
// events) it takes; `timed`: it records the stage events.  Returns 0 or ICER_FATAL_ERROR.
int enqueue_part(icerx_encoder *e, const LaunchPlan &lp, int part, bool timed, const EncodeCall &c, bool clear_bound)
{
    const PartPlan &pp = lp.part[part];
    const int f0 = pp.f0, n_frames = pp.n_frames;
    const uint16_t *const d_frames = c.d_frames; uint8_t *const d_out = c.d_out; int32_t *const d_rcs = c.d_rcs;
    unsigned long long *const d_sizes = reinterpret_cast<unsigned long long *>(c.d_sizes);
    const size_t quota = c.quota, out_stride = c.out_stride;
    const hipStream_t st = c.stream; const Ladder *const ladder = c.ladder; const Target *const target = c.target; const Budget *const budget = c.budget;
    const Roi *const roi = c.roi;
    const bool energy = target || budget;       // the call cuts by distortion: it needs the families' residual energies
    const bool progressive = lp.progressive, use_wg = lp.use_wg, split = pp.split, hybrid = pp.hybrid;
    const size_t W = e->w, H = e->h, plane = W * H;
    const int C = e->channels, P = n_frames * C;
    const uint32_t n_units = (uint32_t)e->plan.units.size();
    int *dwt_ovf = e->dwt_ovf(f0), *mean_ovf = e->mean_ovf(f0), *skip = e->skip(f0), *bound_ovf = e->bound_ovf();
    // this part's planes of the encoder's per-frame buffers
    int16_t *const coef = e->coef.p + (size_t)f0 * C * plane, *const tmp = e->tmp.p + (size_t)f0 * C * plane;
    unsigned long long *const sums = e->sums.p + (size_t)f0 * C;
    uint16_t *const means = e->means.p + (size_t)f0 * C;
    uint8_t *const sig = e->sig.p + (size_t)f0 * e->plan.sig_bytes;
    uint32_t *const sig_hist = e->sig_hist.p + (size_t)f0 * e->plan.n_families * 16;
    uint8_t *const route_buf = e->route.p + (size_t)f0 * n_units;
    uint32_t *const route_list = e->route_list.p + 2 * (size_t)f0 * n_units,       /* (a part's list: light entries, then heavy ones) */ *const route_ctl = e->route_ctl.p + 4 * (size_t)part;
    uint8_t *const slots = e->slots.p + (size_t)f0 * e->plan.slot_bytes;
    uint32_t *const unit_bits = e->unit_bits.p + (size_t)f0 * n_units, *const done_bytes = e->done_bytes.p + (size_t)f0 * n_units;
    uint64_t *const final_off = e->final_off.p + (size_t)f0 * n_units;
    const size_t sub_entries = e->plan.sub_entries;
    if (split && (e->snaps.ensure((size_t)e->max_frames * sub_entries * kMaxSnaps) || e->snap_valid.ensure((size_t)e->max_frames * sub_entries * kMaxSnaps) ||
                  e->sub_recs.ensure((size_t)e->max_frames * sub_entries))) return ICER_FATAL_ERROR;
    {
        ClearList cl;
        const char *bad = nullptr;
        auto clear = [&](const char *what, void *ptr, size_t bytes) { if (!bad && !cl.add(ptr, bytes)) bad = what; };
        if (f0 == 0 && n_frames == e->max_frames && clear_bound) clear("frame flags", e->flags.p, e->flags.n * sizeof(int));       // (the whole block at once)
        else {
            clear("transform flags", dwt_ovf, (size_t)P * sizeof(int)); clear("mean flags", mean_ovf, (size_t)P * sizeof(int)); clear("skip flags", skip, (size_t)n_frames * sizeof(int));
            if (clear_bound) clear("slot bound flag", bound_ovf, sizeof(int));
        }
        clear("LL sums", sums, (size_t)P * sizeof(unsigned long long));
        if (progressive) clear("unit byte counts", done_bytes, (size_t)n_frames * n_units * 4);
        if (hybrid) { clear("chunk histograms", sig_hist, (size_t)n_frames * e->plan.n_families * 16 * sizeof(uint32_t)); clear("route list cursor", route_ctl, 4 * sizeof(uint32_t)); }
        if (split) { clear("snapshot flags", e->snap_valid.p, (size_t)n_frames * sub_entries * kMaxSnaps * sizeof(uint32_t)); clear("sub-range records", e->sub_recs.p, (size_t)n_frames * sub_entries * sizeof(SubRecord)); }
        if (bad) { set_error("enqueue: the clear kernel cannot take the %s range (%d ranges queued)", bad, cl.n); return ICER_FATAL_ERROR; }
        launch_clears(cl, st);
    }
    if (timed && e->timing) HIP_TRY(hipEventRecord(e->ev[0], st));

    size_t cw = W, ch = H;
    launch_dwt(e, d_frames, n_frames, st, e->sample_bits, dwt_ovf, &cw, &ch, coef, tmp);
    if (timed && e->timing) HIP_TRY(hipEventRecord(e->ev[1], st));

    // ---- LL mean, frame status, sign-magnitude
    const uint32_t llw = (uint32_t)cw, llh = (uint32_t)ch;
    unsigned sum_blocks = (llw * llh + 255) / 256;
    if (sum_blocks > 64) sum_blocks = 64;
    hipLaunchKernelGGL(ll_sum_kernel, dim3(sum_blocks, P), dim3(256), 0, st, reinterpret_cast<const uint16_t *>(coef),
                       plane, (uint32_t)W, llw, llh, sums, e->sample_bits == 8 ? 0xFFu : 0xFFFFu);
    hipLaunchKernelGGL(ll_mean_kernel, dim3((P + 63) / 64), dim3(64), 0, st, sums, (uint32_t)P, llw * llh,
                       means, mean_ovf, e->sample_bits);
    hipLaunchKernelGGL(frame_status_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, st, dwt_ovf, mean_ovf, C, n_frames, skip);
    hipLaunchKernelGGL(finalize_ll_kernel, dim3((llw + 63u) / 64u, (llh + 3u) / 4u, P), dim3(256), 0, st,
                       reinterpret_cast<uint16_t *>(coef), plane, (uint32_t)W, llw, llh, means, skip, C, e->sample_bits);
    if (timed && e->timing) HIP_TRY(hipEventRecord(e->ev[2], st));
    if (e->coef_ready && f0 == 0) HIP_TRY(hipEventRecord(e->coef_ready, st));

    // ---- coding units
    // the stateless half of the context modeller, once per family: event bytes for the pipeline coder's pixel waves, the chunk
    // table for both coders (family_events_kernel; the window coder on its own reads the coefficients itself: table only)
    const int n_planes = e->sample_bits == 8 ? kPlanes8 : kPlanes;
    const size_t ev_frame_bytes = (size_t)n_planes * e->plan.sig_bytes * 64u;
    {
        hipLaunchKernelGGL(family_events_kernel, dim3((unsigned)(e->plan.sig_blocks.size() / 2), n_frames), dim3(256), 0, st,
                           reinterpret_cast<const uint16_t *>(coef), plane, (uint32_t)W, C, e->units.p, e->sig_blocks.p, skip, sig,
                           e->plan.sig_bytes, hybrid ? sig_hist : nullptr, e->plan.n_families,
                           use_wg ? nullptr : e->events.p + (size_t)f0 * ev_frame_bytes, ev_frame_bytes, (uint32_t)n_planes);
    }
    const uint8_t *route = nullptr;
    if (hybrid) {
        hipLaunchKernelGGL(route_units_kernel, dim3((unsigned)((n_units + 255) / 256), n_frames), dim3(256), 0, st, e->units.p, n_units, sig_hist, e->plan.n_families,
                           pp.route_percent, 16u, route_buf, route_list, route_ctl, kNoSplitPercent, (uint32_t)n_frames * n_units, kListHeavyMin);
        route = route_buf;
        // the workgroup coder takes its list on a second stream, beside the pipeline kernel (it is submitted first: its
        // workgroups need most of a compute unit's LDS, which they would not find once the pipeline's have spread out)
        HIP_TRY(hipEventRecord(e->fork[part], st));
        HIP_TRY(hipStreamWaitEvent(e->side_stream, e->fork[part], 0));
#define ICER_LAUNCH_LIST(I, NS)                                                                                                          \
        hipLaunchKernelGGL((code_units_list_kernel<I>), dim3(pp.list_grid), dim3(64 * NS::kWgWaves), sizeof(NS::Shared), e->side_stream, \
                           reinterpret_cast<const uint16_t *>(coef), plane, (uint32_t)W, (uint32_t)H, C, e->units.p, n_units,     \
                           e->tables.p, means, skip, slots, e->plan.slot_bytes, unit_bits, sig,                     \
                           e->plan.sig_bytes, route_list, route_ctl, e->prof.p ? e->prof.p + kProfWgsOffset : nullptr, (uint32_t)n_frames * n_units)
        if (pp.list == ListKernel::One) ICER_LAUNCH_LIST(WgOne, wg1); else if (pp.list == ListKernel::Four) ICER_LAUNCH_LIST(WgFour, wg4); else ICER_LAUNCH_LIST(WgSmall, wgs);
#undef ICER_LAUNCH_LIST
        HIP_TRY(hipEventRecord(e->join[part], e->side_stream));
    }
    // a quality-targeted call: the families' residual energies, from the coefficients the coder kernels are about to read.  On the side
    // stream, behind the list kernel if there is one: beside the coder kernels, not in front of them.  (No side stream: before the scan.)
    const uint32_t tgt_planes = (uint32_t)n_planes;
    unsigned long long *const dist = energy ? e->dist.p + (size_t)f0 * e->plan.n_families * (tgt_planes + 1u) : nullptr;
    auto launch_energy = [&](hipStream_t es) -> int {
        HIP_TRY(hipMemsetAsync(dist, 0, (size_t)n_frames * e->plan.n_families * (tgt_planes + 1u) * sizeof(unsigned long long), es));
        hipLaunchKernelGGL(family_energy_kernel, dim3((unsigned)(e->plan.sig_blocks.size() / 2), n_frames), dim3(64 * kEnergyWaves), 0, es,
                           reinterpret_cast<const uint16_t *>(coef), plane, (uint32_t)W, C, e->units.p, e->sig_blocks.p, dist, e->plan.n_families, tgt_planes);
        return 0;
    };
    if (energy && e->side_stream) {
        HIP_TRY(hipEventRecord(e->energy_fork[part], st));
        HIP_TRY(hipStreamWaitEvent(e->side_stream, e->energy_fork[part], 0));
        if (launch_energy(e->side_stream)) return ICER_FATAL_ERROR;
        HIP_TRY(hipEventRecord(e->energy_join[part], e->side_stream));
    }
    SplitLaunch sp;
    if (split) {
        sp.subs = e->subs.p; sp.launch = e->sub_order.p; sp.n_subs = pp.subs; sp.entries = (uint32_t)sub_entries;
        sp.snaps = e->snaps.p; sp.snap_valid = e->snap_valid.p; sp.recs = e->sub_recs.p;
    }
    // TEST HOOK (ICER_HIP_TEST_FAIL_UNIT=<frame>:<unit>[:<calls>]): the pipeline kernel of the next <calls> (default 1) calls reports a time-out for
    // that unit of that frame of the batch; nothing else changes.  tests/test_gpu_recovery.py.
    uint32_t fail_inject = ~0u;
    if (Tuning &t = e->tuning; t.fail_calls > 0 && !use_wg && t.fail_frame >= f0 && t.fail_frame < f0 + n_frames && t.fail_unit < (int)n_units) {
        fail_inject = ((uint32_t)(t.fail_frame - f0) << 20) | (uint32_t)t.fail_unit;
        t.fail_calls--;
    }
    if (!use_wg) {
        const dim3 pipe_grid = pp.position_major ? dim3((unsigned)((n_units + sp.n_subs) * (unsigned)n_frames), 1) : dim3(n_units + sp.n_subs, n_frames);
#define ICER_LAUNCH_PIPE(NW, OCC, PAD)                                                                                                       \
        hipLaunchKernelGGL((code_units_kernel<NW, OCC, PAD>), pipe_grid, dim3(64 * NW), 0, st,                                               \
                           reinterpret_cast<const uint16_t *>(coef), plane, (uint32_t)W, (uint32_t)H, C, e->units.p,                 \
                           progressive ? nullptr : e->work_order.p, n_units, e->tables.p, means, skip, slots,                  \
                           e->plan.slot_bytes, unit_bits, e->prof.p, done_bytes, progressive ? (uint64_t)quota : 0ull, route, sp, \
                           pp.position_major ? (uint32_t)n_frames : 1u, e->events.p + (size_t)f0 * ev_frame_bytes, ev_frame_bytes, sig, e->plan.sig_bytes, fail_inject)
        if (pp.pipe == PipeKernel::Large) ICER_LAUNCH_PIPE(kUnitWavesLarge, 1, 0);
        else if (pp.pipe == PipeKernel::Lone) ICER_LAUNCH_PIPE(kUnitWavesSmall, 1, kLonePadBytes);
        else ICER_LAUNCH_PIPE(kUnitWavesSmall, 8, 0);
#undef ICER_LAUNCH_PIPE
        if (split)
            hipLaunchKernelGGL(splice_units_kernel, dim3(n_units, n_frames), dim3(64 * kSpliceWaves), 0, st, e->units.p, n_units, e->tables.p, means, skip, C,
                               (uint32_t)W, (uint32_t)H, slots, e->plan.slot_bytes, unit_bits, route, sp);
        if (hybrid) HIP_TRY(hipStreamWaitEvent(st, e->join[part], 0));
    } else {
#define ICER_LAUNCH_WG(I, NS)                                                                                                       \
        hipLaunchKernelGGL((code_units_wg_kernel<I>), dim3(n_units, n_frames), dim3(64 * NS::kWgWaves), sizeof(NS::Shared), st,  \
                           reinterpret_cast<const uint16_t *>(coef), plane, (uint32_t)W, (uint32_t)H, C, e->units.p,              \
                           progressive ? nullptr : e->work_order.p, n_units, e->tables.p, means, skip, slots,                      \
                           e->plan.slot_bytes, unit_bits, e->prof.p, done_bytes, progressive ? (uint64_t)quota : 0ull,              \
                           sig, e->plan.sig_bytes)
        if (pp.window == WindowKernel::Four) ICER_LAUNCH_WG(WgFour, wg4); else ICER_LAUNCH_WG(WgFull, wg);
#undef ICER_LAUNCH_WG
    }
    if (timed && e->timing) HIP_TRY(hipEventRecord(e->ev[3], st));

    // ---- quota scan + gather into final stream order
    if (energy) {
        if (e->side_stream) HIP_TRY(hipStreamWaitEvent(st, e->energy_join[part], 0));
        else if (launch_energy(st)) return ICER_FATAL_ERROR;
    }
    if (budget) {
        // this part's curves; the search over all frames and the gather come once per call (enqueue_budget_tail)
        const size_t curve_pitch = (size_t)n_units + 1u;
        hipLaunchKernelGGL(curve_kernel, dim3(n_frames), dim3(64), 0, st, unit_bits, n_units, (uint64_t)quota, skip, e->units.p, dist, e->fam_weight.p,
                           e->plan.n_families, tgt_planes, e->fam_ll_term.p, e->fam_chan.p, means, C, e->curve.p + (size_t)f0 * curve_pitch,
                           e->curve.p + ((size_t)e->max_frames + f0) * curve_pitch, e->curve_head.p + (size_t)f0 * kCurveHeadWords);
        if (lp.n_parts == 1 && enqueue_budget_tail(e, c)) return ICER_FATAL_ERROR;
    } else if (target) {
        const size_t off_pitch = (size_t)e->max_frames * n_units;
        hipLaunchKernelGGL(scan_target_kernel, dim3(n_frames, target->n), dim3(64), 0, st, unit_bits, e->final_order.p, n_units, target->thresholds,
                           (uint64_t)quota, skip, final_off, off_pitch, d_sizes, d_rcs, (uint32_t)target->pitch, e->units.p, bound_ovf, dist,
                           e->fam_weight.p, e->plan.n_families, tgt_planes, e->fam_ll_term.p, e->fam_chan.p, means, C, target->d_reached + f0, target->d_dist + f0, target->d_equiv + f0);
        hipLaunchKernelGGL(gather_ladder_kernel, dim3(n_units, n_frames), dim3(256), 0, st, slots, e->plan.slot_bytes,
                           e->units.p, n_units, unit_bits, final_off, off_pitch, (uint32_t)target->n, d_out, out_stride, (uint32_t)target->pitch);
    } else if (roi) {
        // the frames' ROI orders from their rectangles, then the ladder's scan along them; the gather is the ladder's
        const size_t off_pitch = (size_t)e->max_frames * n_units;
        uint32_t *const rank = e->roi_rank.p + (size_t)f0 * n_units, *const order = e->roi_order.p + (size_t)f0 * n_units;
        hipLaunchKernelGGL(roi_rank_kernel, dim3(n_frames), dim3(64 * kRoiWaves), 0, st, e->units.p, n_units, e->roi_prio.p, roi->d_rois + 4 * (size_t)f0,
                           roi->shift, (uint32_t)W, (uint32_t)H, e->roi_keys.p + (size_t)f0 * n_units, rank, order, roi->d_foreground + f0);
        hipLaunchKernelGGL(scan_roi_kernel, dim3(n_frames, roi->n), dim3(64), 0, st, unit_bits, e->final_order.p, n_units, roi->quotas, skip, rank, order,
                           e->roi_bits.p + (size_t)f0 * n_units, final_off, off_pitch, d_sizes, d_rcs, roi->d_kept + f0, (uint32_t)roi->pitch, e->units.p, bound_ovf);
        hipLaunchKernelGGL(gather_ladder_kernel, dim3(n_units, n_frames), dim3(256), 0, st, slots, e->plan.slot_bytes,
                           e->units.p, n_units, unit_bits, final_off, off_pitch, (uint32_t)roi->n, d_out, out_stride, (uint32_t)roi->pitch);
    } else if (!ladder || ladder->n == 1) {
        hipLaunchKernelGGL(scan_kernel, dim3(n_frames), dim3(64), 0, st, unit_bits, e->final_order.p, n_units,
                           (uint64_t)quota, skip, final_off, d_sizes, d_rcs, e->units.p, bound_ovf);
        hipLaunchKernelGGL(gather_kernel, dim3(n_units, n_frames), dim3(256), 0, st, slots, e->plan.slot_bytes,
                           e->units.p, n_units, unit_bits, final_off, d_out, out_stride);
    } else {
        // (the final offsets of quota q: the q-th block of max_frames x units entries, icerx_encode_device_ladder sized them)
        const size_t off_pitch = (size_t)e->max_frames * n_units;
        hipLaunchKernelGGL(scan_ladder_kernel, dim3(n_frames, ladder->n), dim3(64), 0, st, unit_bits, e->final_order.p, n_units,
                           ladder->quotas, skip, final_off, off_pitch, d_sizes, d_rcs, (uint32_t)ladder->pitch, e->units.p, bound_ovf);
        hipLaunchKernelGGL(gather_ladder_kernel, dim3(n_units, n_frames), dim3(256), 0, st, slots, e->plan.slot_bytes,
                           e->units.p, n_units, unit_bits, final_off, off_pitch, (uint32_t)ladder->n, d_out, out_stride, (uint32_t)ladder->pitch);
    }
    if (timed && e->timing) {
        HIP_TRY(hipEventRecord(e->ev[4], st));
        e->ev_pending = true;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// One call = one batch, launched as plan_launch (launch_plan.hpp) decides.  A batch of several frames coded by the SYNCHRONOUS entry
// points is enqueued in parts on two streams -- the caller's and one of the encoder's own --, so that a part's transform and event pass
// run beside the coder kernels of the part before it and the tail of a coder kernel (its last long units, most of the chip idle) hides
// behind the next part's: what a caller gets from two encoders and the asynchronous calls, inside one call.  Not for
// the asynchronous entry points (the caller overlaps whole batches itself), progressive mode, or single frames: `overlap_ok`.  A part is
// the call for its frames (EncodeCall::frames) on its stream.
int enqueue(icerx_encoder *e, const EncodeCall &c, bool overlap_ok)
{
    const hipStream_t st = c.stream;
    const CoderState cs{e->wg_available, e->wg_once, e->half_stream != nullptr};
    const LaunchPlan &lp = e->last_plan = plan_launch(launch_shape(e), e->tuning, cs, c.n_frames, c.quota, overlap_ok, c.roi != nullptr);
    if (lp.n_parts == 1) return enqueue_part(e, lp, 0, true, c, true);
    HIP_TRY(hipMemsetAsync(e->bound_ovf(), 0, sizeof(int), st));        // (shared by the parts: before the second stream forks off)
    HIP_TRY(hipEventRecord(e->part_fork, st));                          // (the second stream starts behind whatever the caller's stream holds)
    HIP_TRY(hipStreamWaitEvent(e->half_stream, e->part_fork, 0));
    // (the stages of the parts overlap: the call's span is booked on the coder stage -- bench.py's roofline divides the call's bytes by it)
    if (e->timing) { HIP_TRY(hipEventRecord(e->ev[0], st)); HIP_TRY(hipEventRecord(e->ev[1], st)); HIP_TRY(hipEventRecord(e->ev[2], st)); }
    for (int k = 0; k < lp.n_parts; k++) {
        EncodeCall pc = c.frames(lp.part[k].f0, lp.part[k].n_frames, (size_t)e->channels * e->w * e->h);
        pc.stream = (k & 1) ? e->half_stream : st;
        if (int rc = enqueue_part(e, lp, k, false, pc, false)) return rc;
    }
    HIP_TRY(hipEventRecord(e->part_join, e->half_stream));
    HIP_TRY(hipStreamWaitEvent(st, e->part_join, 0));
    if (c.budget && enqueue_budget_tail(e, c)) return ICER_FATAL_ERROR;     // (the allocation needs the curves of every part)
    if (e->timing) {
        HIP_TRY(hipEventRecord(e->ev[3], st)); HIP_TRY(hipEventRecord(e->ev[4], st));
        e->ev_pending = true;
    }
    return 0;
}

}  // namespace

extern "C" {

const char *icerx_last_error(void) { return g_last_error.c_str(); }

int icer_init(void)
{
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (!g_tables_ready) {
        build_coder_tables(&g_tables);
        g_tables_ready = true;
    }
    return ICER_RESULT_OK;
}

int icer_init_output_struct(icer_output_data_buf_typedef *out, uint8_t *data, size_t buf_len, size_t byte_quota)
{
    if (byte_quota * 2 > buf_len) return ICER_OUTPUT_BUF_TOO_SMALL;
    out->size_used = 0;
    out->data_start = data;
    out->size_allocated = byte_quota;
    out->rearrange_start = data + byte_quota;
    return ICER_RESULT_OK;
}

int icerx_encoder_create(icerx_encoder **out, int device, size_t w, size_t h, int channels, int stages, int filt,
                         int segments, int max_frames)
{
    return icerx_encoder_create_ex(out, device, w, h, channels, stages, filt, segments, max_frames, 16);
}

int icerx_encoder_create_ex(icerx_encoder **out, int device, size_t w, size_t h, int channels, int stages, int filt,
                            int segments, int max_frames, int sample_bits)
{
    *out = nullptr;
    icer_init();
    if (filt < 0 || filt > 6 || max_frames < 1 || (sample_bits != 8 && sample_bits != 16)) return ICER_INVALID_INPUT;
    icerx_encoder *e = new icerx_encoder();
    e->device = device; e->w = w; e->h = h; e->channels = channels; e->stages = stages; e->filt = filt;
    e->segments = segments; e->max_frames = max_frames; e->sample_bits = sample_bits;
    const int rc = build_plan(&e->plan, w, h, channels, stages, segments, sample_bits);
    if (rc != kOk) { delete e; return rc; }
    e->tuning = parse_tuning(getenv);
    e->bits_per_pixel = (unsigned)e->tuning.slot_bpp;

    int count = 0;
    hipError_t he = hipGetDeviceCount(&count);
    const int logical_count = he == hipSuccess && count > 0 ? logical_device_count() : 0;
    if (he != hipSuccess || count <= 0 || device < 0 || device >= logical_count) {
        set_error("no usable HIP device (hipGetDeviceCount: %s, count=%d, requested=%d); this library has no CPU path",
                  hipGetErrorString(he), count, device);
        delete e;
        return ICER_FATAL_ERROR;
    }
    e->logical_device = device;
    device = physical_of(device);
    e->device = device;
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) e->n_cus = prop.multiProcessorCount; }
    // (a failing HIP call below must not leak the object and what it has allocated so far)
#define CREATE_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); icerx_encoder_destroy(e); return ICER_FATAL_ERROR; } } while (0)
    CREATE_TRY(hipSetDevice(device));
    const size_t P = (size_t)max_frames * channels, plane = w * h, n_units = e->plan.units.size();
    if (e->coef.ensure(P * plane) || e->tmp.ensure(P * plane) || e->sums.ensure(P) || e->means.ensure(P) ||
        e->flags.ensure(2 * P + 2 * max_frames + 1) || e->unit_bits.ensure((size_t)max_frames * n_units) ||
        e->done_bytes.ensure((size_t)max_frames * n_units) || e->route.ensure((size_t)max_frames * n_units) || e->route_list.ensure(2 * (size_t)max_frames * n_units) || e->route_ctl.ensure(4 * kMaxParts) || e->sig.ensure((size_t)max_frames * e->plan.sig_bytes + 64) || e->sig_hist.ensure((size_t)max_frames * e->plan.n_families * 16 + 16) ||
        e->final_off.ensure((size_t)max_frames * n_units) || e->tables.ensure(1) || e->sizes.ensure(max_frames) ||
        e->rcs.ensure(max_frames)) {
        icerx_encoder_destroy(e);
        return ICER_FATAL_ERROR;
    }
    // event bytes of the pipeline coder (events.hpp): one per pixel and bit plane, in chunk order
    if (e->tuning.coder != 2 && e->events.ensure((size_t)max_frames * (size_t)(sample_bits == 8 ? kPlanes8 : kPlanes) * e->plan.sig_bytes * 64u + 64)) {
        icerx_encoder_destroy(e);
        return ICER_FATAL_ERROR;
    }
    CREATE_TRY(hipMemcpy(e->tables.p, &g_tables, sizeof g_tables, hipMemcpyHostToDevice));
    // the workgroup coder's LDS block is above the 64 KiB a kernel gets without asking
    // A device / runtime that refuses it loses only the paths that need that coder (progressive mode then runs on the
    // pipeline, launches are not shared, a unit time-out becomes an error) -- reported by icerx_encoder_stats.
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(code_units_wg_kernel<WgFull>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(wg::Shared)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(code_units_wg_kernel<WgFour>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(wg4::Shared)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(code_units_list_kernel<WgSmall>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(wgs::Shared)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(code_units_list_kernel<WgOne>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(wg1::Shared)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void *>(code_units_list_kernel<WgFour>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(wg4::Shared)) != hipSuccess ||
        create_side_stream(&e->side_stream) != hipSuccess ||
        create_part_events(e) != hipSuccess) {
        (void)hipGetLastError();
        e->wg_available = false;
        if (e->tuning.coder == 2) { set_error("ICER_HIP_CODER=wg, but this device does not grant the workgroup coder its LDS block"); icerx_encoder_destroy(e); return ICER_FATAL_ERROR; }
        fprintf(stderr, "libicer_hip: the workgroup coder is not available on this device; the wave pipeline codes everything\n");
    }
#ifdef ICER_PHASE_TIMERS
    if (e->prof.ensure(kProfWords)) { icerx_encoder_destroy(e); return ICER_FATAL_ERROR; }
    CREATE_TRY(hipMemset(e->prof.p, 0, kProfWords * sizeof(uint64_t)));
#endif
    for (auto &ev : e->ev) CREATE_TRY(hipEventCreate(&ev));
    CREATE_TRY(hipHostMalloc((void **)&e->h_flag, (2 + kMaxParts) * sizeof(int), hipHostMallocDefault));
    CREATE_TRY(hipEventCreateWithFlags(&e->done, hipEventDisableTiming));
#undef CREATE_TRY
    *out = e;
    return 0;
}

void icerx_encoder_destroy(icerx_encoder *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    e->coef.release(); e->tmp.release(); e->sums.release(); e->means.release(); e->flags.release();
    e->units.release(); e->work_order.release(); e->final_order.release(); e->unit_bits.release(); e->done_bytes.release(); e->sig.release(); e->events.release(); e->sig_hist.release(); e->sig_blocks.release(); e->route.release(); e->route_list.release(); e->route_ctl.release();
    e->final_off.release(); e->slots.release(); e->tables.release(); e->in.release(); e->in8.release(); e->out.release();
    e->sizes.release(); e->rcs.release(); e->prof.release();
    e->subs.release(); e->sub_order.release(); e->snap_valid.release(); e->snaps.release(); e->sub_recs.release();
    e->dist.release(); e->fam_weight.release(); e->fam_chan.release(); e->fam_ll_term.release();
    e->curve.release(); e->curve_head.release(); e->budget_state.release();
    e->roi_prio.release(); e->roi_keys.release(); e->roi_rank.release(); e->roi_order.release(); e->roi_bits.release();
    for (auto &ev : e->energy_fork) if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : e->energy_join) if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : e->ev) if (ev) (void)hipEventDestroy(ev);
    if (e->done) (void)hipEventDestroy(e->done);
    for (auto &ev : e->fork) if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : e->join) if (ev) (void)hipEventDestroy(ev);
    if (e->part_fork) (void)hipEventDestroy(e->part_fork);
    if (e->part_join) (void)hipEventDestroy(e->part_join);
    if (e->half_stream) (void)hipStreamDestroy(e->half_stream);
    if (e->side_stream && !e->side_stream_borrowed) (void)hipStreamDestroy(e->side_stream);
    if (e->coef_ready) (void)hipEventDestroy(e->coef_ready);
    if (e->io_stream) (void)hipStreamDestroy(e->io_stream);
    if (e->copy_stream) (void)hipStreamDestroy(e->copy_stream);
    if (e->h_flag) (void)hipHostFree(e->h_flag);
    delete e;
}

}  // extern "C"

namespace {      // the host driver of an encode call, between the entry points below and enqueue

// diagnostics of a unit time-out (rare error path): which unit, which wave at which wait, and the unit's hand-off counters
// (the record code_units_kernel leaves in the failed unit's payload slot)
static void report_timeouts(icerx_encoder *e, int n_frames)
{
    const size_t n_units = e->plan.units.size();
    std::vector<uint32_t> bits((size_t)n_frames * n_units);
    if (!n_units || hipMemcpy(bits.data(), e->unit_bits.p, bits.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return;
    int shown = 0;
    for (size_t i = 0; i < bits.size() && shown < 4; i++) {
        if (bits[i] != kUnitFailed) continue;
        const size_t frame = i / n_units, ui = i % n_units;
        const UnitDesc &u = e->plan.units[ui];
        uint32_t dbg[kFailWords] = {0};
        if (u.cap_words >= kFailWords)
            (void)hipMemcpy(dbg, e->slots.p + frame * e->plan.slot_bytes + u.slot_off + kHeaderBytes, sizeof dbg, hipMemcpyDeviceToHost);
        fprintf(stderr, "libicer_hip: time-out in frame %zu unit %zu (chan %u level %u subband %u lsb %u seg %u, %u x %u)", frame, ui,
                (unsigned)u.chan, (unsigned)u.level, (unsigned)u.subband, (unsigned)u.lsb, (unsigned)u.seg, (unsigned)u.w, (unsigned)u.h);
        if (dbg[0] == kFailMagic)
            fprintf(stderr, ": wave %u gave up at coder_core.hpp:%u; chunks %u, done pixel/count/compact/merge %u/%u/%u/%u, ring alloc/popped "
                    "%u/%u, hold seq/ack %u/%u, generation %u (last exact %u), bitpos %u, flushed words %u, drain_exit %u",
                    dbg[1] >> 16, dbg[1] & 0xFFFFu, dbg[2], dbg[3], dbg[4], dbg[5], dbg[6], dbg[7], dbg[8], dbg[9], dbg[10], dbg[11],
                    dbg[12], dbg[13], dbg[14], dbg[15]);
        fprintf(stderr, "\n");
        shown++;
    }
}

// The device row that holds the longest stream a frame can have at `quota` with the current slot table (upload_units) -- the rows an entry
// point stages for its caller, stage_rows --, and whether a caller's rows `out_stride` apart do.  A retry that enlarges the slots changes both.
size_t row_stride(const icerx_encoder *e, size_t quota) { return std::min(quota, e->plan.slot_bytes) + 4; }
bool stride_admissible(const icerx_encoder *e, size_t out_stride, size_t quota) { return out_stride >= quota || out_stride >= e->plan.slot_bytes; }

// One encode call (EncodeCall) = encode_begin (everything enqueued on the call's stream, nothing waited for) + encode_finish (wait,
// then the rare re-runs).  `flag` = pinned host words that receive the batch's verdict: [0] bit 0 a coding unit outgrew its
// provisioned slot, bit 1 a unit timed out; [1] units on the route list; `done` is recorded behind them.
int encode_begin(icerx_encoder *e, const EncodeCall &c, int *flag, hipEvent_t done)
{
    if (upload_units(e, c.quota, c.stream)) return ICER_FATAL_ERROR;
    if (e->slots.ensure((size_t)e->max_frames * e->plan.slot_bytes)) return ICER_FATAL_ERROR;
    if (!stride_admissible(e, c.out_stride, c.quota)) {
        set_error("icerx_encode_device: out_stride %zu smaller than the byte quota %zu", c.out_stride, c.quota);
        return ICER_INVALID_INPUT;
    }
    if (enqueue(e, c, c.overlap_ok && flag == e->h_flag)) return ICER_FATAL_ERROR;
    HIP_TRY(hipMemcpyAsync(flag, e->bound_ovf(), sizeof(int), hipMemcpyDeviceToHost, c.stream));
    // the list length of each part that routed (a batch in parts: the other parts' behind the two words every caller has -- e->h_flag)
    for (int k = 0; k < e->last_plan.n_parts; k++)
        if (e->last_plan.part[k].hybrid) HIP_TRY(hipMemcpyAsync(flag + 1 + k, e->route_ctl.p + 4 * k, sizeof(int), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipEventRecord(done, c.stream));
    return 0;
}

// Wait for an event.  The synchronous entry points spin on a query instead of blocking in hipStreamSynchronize: an
// encode call is milliseconds and the wake-up latency of a blocking wait (measured: up to 3 ms per call on a busy host)
// would be charged to every frame.  The per-device workers of a host batch (sleepy) give the core away between polls:
// eight of them must not burn eight cores, and their waits are hidden behind the next sub-batch anyway.
static int wait_event(hipEvent_t ev, bool sleepy)
{
    for (uint32_t polls = 0;; polls++) {
        const hipError_t q = hipEventQuery(ev);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) { set_error("hipEventQuery failed: %s", hipGetErrorString(q)); return ICER_FATAL_ERROR; }
        if (sleepy && polls > 64u) { const struct timespec ts = {0, 50000}; nanosleep(&ts, nullptr); }
        else cpu_relax();
    }
}

// The verdict of a finished batch (encode_begin's flag words), read once per run (encode_finish): 0 = done, 1 = run it again (the encoder
// has been adjusted: larger slots at the next upload_units, or the barrier-only coder for the next run), or an error code.
static int encode_verdict(icerx_encoder *e, int n_frames, const int *flag)
{
    const int ovf = flag[0];
    if (!ovf) {
        bool routed = false;
        for (int k = 0; k < e->last_plan.n_parts; k++) if (e->last_plan.part[k].hybrid) { routed = true; e->n_routed_units += (uint64_t)(uint32_t)flag[1 + k]; }
        if (routed) e->n_routed_launches++;
        return 0;
    }
    if (ovf & 2) {
        // A wave of some coding unit of the eight-wave pipeline waited longer than its spin bound (seconds) and gave
        // the unit up (seen once in ~60 000 randomised encodes in round 1, never reproduced).  The batch is coded again
        // by the workgroup-window coder, which has no wave-to-wave hand-offs to wait for (barriers only) and produces
        // the same streams: the caller gets its result, the event is counted (icerx_encoder_stats) and reported.
        report_timeouts(e, n_frames);
        e->n_timeouts++; g_stats[0]++;
        if (e->wg_once || !e->wg_available) {          // (the window coder never reports a time-out)
            e->wg_once = false;
            set_error(e->wg_available ? "a coding unit timed out in the workgroup-window coder"
                                      : "a coding unit timed out and the barrier-only coder is not available on this device");
            return ICER_FATAL_ERROR;
        }
        e->n_fallbacks++; g_stats[1]++;
        e->wg_once = true;
        fprintf(stderr, "libicer_hip: a coding unit timed out; coding the batch again with the barrier-only coder\n");
        e->ev_pending = false;
        return 1;
    }
    e->n_slot_retries++; g_stats[2]++;
    if (e->bits_per_pixel >= 24) {
        set_error("coding-unit slot overflow at the theoretical bound");
        return ICER_FATAL_ERROR;
    }
    // a unit produced more than the provisioned bits per pixel: enlarge the slots and redo the batch
    e->ev_pending = false;
    e->bits_per_pixel = e->bits_per_pixel * 2 > 24 ? 24 : e->bits_per_pixel * 2;
    e->units_uploaded = false;
    return 1;
}

// Everything after encode_begin: wait for `done` and read the verdict; while it is "again", plan the slots anew (a no-op after a time-out),
// let the owner of the output rows adjust them -- resize(c) may point the call at new rows; the device API passes caller_rows: its caller's
// rows are what they are, and encode_begin refuses a stride that larger slots have made too small --, begin again and wait.
int caller_rows(EncodeCall &) { return 0; }
template <class Resize> int encode_finish(icerx_encoder *e, EncodeCall &c, int *flag, hipEvent_t done, Resize resize)
{
    for (;;) {
        if (wait_event(done, e->sleepy_wait)) return ICER_FATAL_ERROR;
        const int v = encode_verdict(e, c.n_frames, flag);
        if (v < 0) return v;
        if (v == 0) break;
        if (upload_units(e, c.quota, c.stream)) return ICER_FATAL_ERROR;
        if (int rc = resize(c)) return rc;
        if (int rc = encode_begin(e, c, flag, done)) return rc;
    }
    e->wg_once = false;
    return 0;
}

// The rows of the entry points that stage the streams on the device for their caller (icerx_encode_host, the lib_icer drop-ins): the
// encoder's own `out`, a row of row_stride for each of its frames, re-made when a retry has enlarged the slots
int stage_rows(icerx_encoder *e, EncodeCall &c)
{
    c.out_stride = row_stride(e, c.quota);
    if (e->out.ensure((size_t)e->max_frames * c.out_stride)) return ICER_FATAL_ERROR;
    c.d_out = e->out.p;
    return 0;
}

// a synchronous call on the encoder's own flag words and event (the caller has been through enter_encode or owns the encoder)
template <class Resize> int encode_sync(icerx_encoder *e, EncodeCall &c, Resize resize)
{
    if (accumulate_timing(e)) return ICER_FATAL_ERROR;
    e->wg_once = false;
    if (int rc = encode_begin(e, c, e->h_flag, e->done)) return rc;
    return encode_finish(e, c, e->h_flag, e->done, resize);
}
int encode_staged(icerx_encoder *e, EncodeCall &c)      // ... into the encoder's own rows
{
    if (upload_units(e, c.quota, c.stream) || stage_rows(e, c)) return ICER_FATAL_ERROR;
    return encode_sync(e, c, [e](EncodeCall &again) { return stage_rows(e, again); });
}

// The front door of the icerx_encode_* entry points: the arguments (`pointers`: none of the entry's is null), what the entry needs of
// its encoder (`bits`, `channels`; 0 = any -- `needs` says it in the message), no asynchronous call pending, the device selected.
// Returns 0, or what the entry returns (the error is set).
const char kPendingAsync[] = "an asynchronous encode is pending on this encoder (icerx_encoder_wait)";
int enter_encode(const char *entry, icerx_encoder *e, bool pointers, int n_frames, int bits, int channels, const char *needs, const char *pending = kPendingAsync)
{
    if (!e || !pointers || n_frames < 1 || n_frames > e->max_frames || (bits && e->sample_bits != bits) || (channels && e->channels != channels)) {
        set_error("%s: invalid arguments%s", entry, needs);
        return ICER_INVALID_INPUT;
    }
    if (e->pend.active) { set_error("%s: %s", entry, pending); return ICER_INVALID_INPUT; }
    HIP_TRY(hipSetDevice(e->device));
    return 0;
}

// Widening and narrowing between the callers' 8-bit samples and the encoder's 16-bit planes, in the encoder's staging buffers:
// U8 8-bit gray -> uint16; S8 the uint8 twins' int8 storage -> int16; Rgb8 packed RGB888 -> Y, Cb, Cr planes (n = pixels); all from
// `src` into e->in.  NarrowSm8: the coefficient planes (e->coef) -> int8 sign-magnitude bytes in e->in8.  n = samples of the call.
enum class Convert { U8, S8, Rgb8, NarrowSm8 };
int convert_samples(icerx_encoder *e, Convert how, const uint8_t *src, size_t n, hipStream_t st)
{
    const size_t room = (size_t)e->max_frames * e->channels * e->w * e->h;
    if (how == Convert::NarrowSm8 ? e->in8.ensure(room) : e->in.ensure(room)) return ICER_FATAL_ERROR;
    const dim3 grid((unsigned)std::min<size_t>((n + 255) / 256, 4096));
    switch (how) {
    case Convert::U8: hipLaunchKernelGGL(widen_u8_kernel, grid, dim3(256), 0, st, src, e->in.p, n); break;
    case Convert::S8: hipLaunchKernelGGL(widen_s8_kernel, grid, dim3(256), 0, st, src, e->in.p, n); break;
    case Convert::Rgb8: hipLaunchKernelGGL(rgb8_to_ycbcr_kernel, grid, dim3(256), 0, st, src, e->in.p, e->w * e->h, (int)(n / (e->w * e->h))); break;
    case Convert::NarrowSm8: hipLaunchKernelGGL(narrow_sm8_kernel, grid, dim3(256), 0, st, reinterpret_cast<const uint16_t *>(e->coef.p), e->in8.p, n); break;
    }
    return 0;
}

}  // namespace

extern "C" {

int icerx_encode_device(icerx_encoder *e, const uint16_t *d_frames, int n_frames, size_t byte_quota, uint8_t *d_out,
                        size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream)
{
    if (int rc = enter_encode("icerx_encode_device", e, d_frames && d_out && d_sizes && d_rcs, n_frames, 16, 0,
                              " (needs a 16-bit encoder; 8-bit samples: icerx_encode_device_s8)")) return rc;
    EncodeCall c{d_frames, n_frames, byte_quota, d_out, out_stride, d_sizes, d_rcs, (hipStream_t)stream, true};
    return encode_sync(e, c, caller_rows);
}

// The same call in two halves, so that a caller can overlap its own copies (or another encoder's work) with the coding:
// icerx_encode_device_async returns as soon as everything is enqueued on `stream`; icerx_encoder_wait returns once the
// batch is complete there (and has re-run it in the rare cases icerx_encode_device does).  One pending call per encoder.
int icerx_encode_device_async(icerx_encoder *e, const uint16_t *d_frames, int n_frames, size_t byte_quota, uint8_t *d_out,
                              size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream)
{
    if (int rc = enter_encode("icerx_encode_device_async", e, d_frames && d_out && d_sizes && d_rcs, n_frames, 16, 0, "",
                              "the previous asynchronous encode has not been waited for")) return rc;
    if (accumulate_timing(e)) return ICER_FATAL_ERROR;
    e->wg_once = false;
    const EncodeCall c{d_frames, n_frames, byte_quota, d_out, out_stride, d_sizes, d_rcs, (hipStream_t)stream, false};
    if (int rc = encode_begin(e, c, e->h_flag, e->done)) return rc;
    e->pend.active = true;
    e->pend.call = c;
    return 0;
}

int icerx_encoder_wait(icerx_encoder *e)
{
    if (!e) return ICER_INVALID_INPUT;
    if (!e->pend.active) return 0;
    e->pend.active = false;
    HIP_TRY(hipSetDevice(e->device));
    return encode_finish(e, e->pend.call, e->h_flag, e->done, caller_rows);
}

// Rate ladder (include/icer_hip.h): checked here in full -- out_stride against the slot table of the largest quota -- before anything
// is enqueued, then an ordinary synchronous call at the largest quota whose assembly cuts every quota's streams.
int icerx_encode_device_ladder(icerx_encoder *e, const void *d_frames, int n_frames, const size_t *quotas, int n_quotas, uint8_t *d_out,
                               size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream)
{
    if (int rc = enter_encode("icerx_encode_device_ladder", e, d_frames && quotas && d_out && d_sizes && d_rcs && n_quotas >= 1 && n_quotas <= ICERX_MAX_LADDER,
                              n_frames, 0, 0, " (1 <= n_quotas <= ICERX_MAX_LADDER, 1 <= n_frames <= max_frames)")) return rc;
    Ladder lq;
    lq.n = n_quotas;
    lq.pitch = n_frames;
    size_t top = 0;
    for (int q = 0; q < n_quotas; q++) { lq.quotas.q[q] = quotas[q]; top = std::max(top, quotas[q]); }
    hipStream_t st = (hipStream_t)stream;
    if (upload_units(e, top, st)) return ICER_FATAL_ERROR;
    if (!stride_admissible(e, out_stride, top)) {
        set_error("icerx_encode_device_ladder: out_stride %zu smaller than the largest byte quota %zu", out_stride, top);
        return ICER_INVALID_INPUT;
    }
    if (n_quotas > 1 && e->final_off.ensure((size_t)n_quotas * e->max_frames * e->plan.units.size())) return ICER_FATAL_ERROR;
    const uint16_t *planes = static_cast<const uint16_t *>(d_frames);
    if (e->sample_bits == 8) {          // (as icerx_encode_device_s8)
        if (convert_samples(e, Convert::S8, static_cast<const uint8_t *>(d_frames), (size_t)n_frames * e->channels * e->w * e->h, st)) return ICER_FATAL_ERROR;
        planes = e->in.p;
    }
    EncodeCall c{planes, n_frames, top, d_out, out_stride, d_sizes, d_rcs, st, true, &lq};
    return encode_sync(e, c, caller_rows);
}

// Region-of-interest encode (include/icer_hip.h): checked in full before anything is enqueued, as the ladder is; then a synchronous call at
// the largest quota, planned with every unit coded, whose assembly cuts every quota's streams along the frames' ROI orders.  What the
// first such call of an encoder makes: the units' priorities on the device and the rank arrays.
static int prepare_roi(icerx_encoder *e, int n_quotas)
{
    const size_t n_units = e->plan.units.size(), per_call = (size_t)e->max_frames * n_units;
    if (!e->roi_prio.p) {
        std::vector<uint64_t> prio;
        if (!roi_priorities(e->plan, &prio)) {         // (no geometry the planner accepts gets here: make_packets keeps the bound and the order)
            set_error("icerx_encode_device_roi: the packet priorities of this geometry do not fit the sort keys");
            return ICER_FATAL_ERROR;
        }
        if (e->roi_keys.ensure(per_call) || e->roi_rank.ensure(per_call) || e->roi_order.ensure(per_call)) return ICER_FATAL_ERROR;
        DevBuf<uint64_t> p;
        if (p.ensure(n_units)) return ICER_FATAL_ERROR;
        if (hipMemcpy(p.p, prio.data(), n_units * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess) { p.release(); set_error("icerx_encode_device_roi: uploading the priorities failed"); return ICER_FATAL_ERROR; }
        e->roi_prio = p;            // (last: its presence says that everything above exists)
    }
    if (e->roi_bits.ensure((size_t)n_quotas * per_call) || e->final_off.ensure((size_t)n_quotas * per_call)) return ICER_FATAL_ERROR;
    return 0;
}

int icerx_encode_device_roi(icerx_encoder *e, const void *d_frames, int n_frames, const uint32_t *d_rois, int shift, const size_t *quotas, int n_quotas,
                            uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, uint32_t *d_kept, uint32_t *d_foreground, void *stream)
{
    if (int rc = enter_encode("icerx_encode_device_roi", e, d_frames && d_rois && quotas && d_out && d_sizes && d_rcs && d_kept && d_foreground &&
                              n_quotas >= 1 && n_quotas <= ICERX_MAX_LADDER && shift >= 0 && shift <= ICERX_MAX_ROI_SHIFT, n_frames, 0, 0,
                              " (1 <= n_quotas <= ICERX_MAX_LADDER, 0 <= shift <= ICERX_MAX_ROI_SHIFT, 1 <= n_frames <= max_frames)")) return rc;
    Roi rq;
    rq.n = n_quotas;
    rq.pitch = n_frames;
    rq.shift = (uint32_t)shift;
    rq.d_rois = d_rois;
    rq.d_kept = d_kept;
    rq.d_foreground = d_foreground;
    size_t top = 0;
    for (int q = 0; q < n_quotas; q++) { rq.quotas.q[q] = quotas[q]; top = std::max(top, quotas[q]); }
    hipStream_t st = (hipStream_t)stream;
    if (upload_units(e, top, st)) return ICER_FATAL_ERROR;
    if (!stride_admissible(e, out_stride, top)) {
        set_error("icerx_encode_device_roi: out_stride %zu smaller than the largest byte quota %zu", out_stride, top);
        return ICER_INVALID_INPUT;
    }
    if (int rc = prepare_roi(e, n_quotas)) return rc;
    const uint16_t *planes = static_cast<const uint16_t *>(d_frames);
    if (e->sample_bits == 8) {          // (as icerx_encode_device_s8)
        if (convert_samples(e, Convert::S8, static_cast<const uint8_t *>(d_frames), (size_t)n_frames * e->channels * e->w * e->h, st)) return ICER_FATAL_ERROR;
        planes = e->in.p;
    }
    EncodeCall c{planes, n_frames, top, d_out, out_stride, d_sizes, d_rcs, st, true, nullptr, nullptr, nullptr, &rq};
    return encode_sync(e, c, caller_rows);
}

// Quality-targeted encode (include/icer_hip.h).  T = floor(target_mse x samples x 16) in the units of the frame's distortion D
// (distortion_core.hpp: Q4 weights), saturated; false: the target is negative or not a number.
static bool target_threshold(const icerx_encoder *e, double target_mse, uint64_t *T)
{
    if (!(target_mse >= 0.0)) return false;
    const double t = target_mse * (double)((uint64_t)e->w * e->h * (uint64_t)e->channels * 16u);     // (the sample count x 16 < 2^40: exact)
    *T = t >= 18446744073709551616.0 ? ~0ull : (uint64_t)t;
    return true;
}

uint64_t icerx_target_threshold(const icerx_encoder *e, double target_mse)
{
    uint64_t T = 0;
    return e && target_threshold(e, target_mse, &T) ? T : 0;
}

// What the first target call of an encoder makes: the families' weights on the device, the energy table, the events of the energy
// pass -- after checking that the frame's distortion cannot leave 64 bits: D <= sum over families of coefficients x (2^15 - 1)^2 x weight (128^2 for the uint8 twins).
static int prepare_target(icerx_encoder *e, const char *entry = "icerx_encode_device_target")
{
    const size_t n_fam = e->plan.n_families, entries = (size_t)(e->sample_bits == 8 ? kPlanes8 : kPlanes) + 1;
    if (e->fam_weight.p) return 0;
    std::vector<uint32_t> weight(n_fam, 0u), chan(n_fam, 0u);
    std::vector<unsigned long long> ll_term(n_fam, 0ull);
    const uint64_t max_mag = e->sample_bits == 8 ? 128u : 32767u;        // (int8 / int16 coefficients in sign-magnitude form)
    unsigned __int128 bound = 0;
    for (const UnitDesc &u : e->plan.units) {
        if (weight[u.family]) continue;
        weight[u.family] = kSubbandGainQ4[e->filt][u.level - 1][u.subband];
        chan[u.family] = u.chan;
        bound += (unsigned __int128)((uint64_t)u.w * u.h) * (max_mag * max_mag) * weight[u.family];
        if (u.subband == kLL && e->sample_bits == 16) {      // (the LL mean's upper byte, lost in the packet header: at most 0x7F00 per coefficient)
            ll_term[u.family] = (unsigned long long)u.w * u.h * weight[u.family];
            bound += (unsigned __int128)ll_term[u.family] * (0x7F00ull * 0x7F00ull);
        }
    }
    if (bound >> 64) {
        set_error("%s: the distortion of a %zu x %zu frame of %d channel(s) can exceed 64 bits", entry, e->w, e->h, e->channels);
        return ICER_INVALID_INPUT;
    }
    for (int k = 0; k < kMaxParts; k++) {
        if (!e->energy_fork[k]) HIP_TRY(hipEventCreateWithFlags(&e->energy_fork[k], hipEventDisableTiming));
        if (!e->energy_join[k]) HIP_TRY(hipEventCreateWithFlags(&e->energy_join[k], hipEventDisableTiming));
    }
    if (e->dist.ensure((size_t)e->max_frames * n_fam * entries)) return ICER_FATAL_ERROR;
    if (e->fam_chan.ensure(n_fam) || e->fam_ll_term.ensure(n_fam)) return ICER_FATAL_ERROR;
    if (hipMemcpy(e->fam_chan.p, chan.data(), n_fam * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->fam_ll_term.p, ll_term.data(), n_fam * sizeof(unsigned long long), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("icerx_encode_device_target: uploading the family tables failed");
        return ICER_FATAL_ERROR;
    }
    DevBuf<uint32_t> w;
    if (w.ensure(n_fam)) return ICER_FATAL_ERROR;
    if (hipMemcpy(w.p, weight.data(), n_fam * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) { w.release(); set_error("icerx_encode_device_target: uploading the weights failed"); return ICER_FATAL_ERROR; }
    e->fam_weight = w;           // (last: its presence says that everything above exists)
    return 0;
}

int icerx_encode_device_target(icerx_encoder *e, const void *d_frames, int n_frames, const double *target_mse, int n_targets, size_t byte_cap,
                               uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, int32_t *d_reached, uint64_t *d_dist,
                               uint64_t *d_equiv_quota, void *stream)
{
    if (int rc = enter_encode("icerx_encode_device_target", e, d_frames && target_mse && d_out && d_sizes && d_rcs && d_reached && d_dist && d_equiv_quota &&
                              n_targets >= 1 && n_targets <= ICERX_MAX_LADDER, n_frames, 0, 0, " (1 <= n_targets <= ICERX_MAX_LADDER, 1 <= n_frames <= max_frames)")) return rc;
    Target tg;
    tg.n = n_targets;
    tg.pitch = n_frames;
    tg.d_reached = d_reached;
    tg.d_dist = reinterpret_cast<unsigned long long *>(d_dist);
    tg.d_equiv = reinterpret_cast<unsigned long long *>(d_equiv_quota);
    for (int t = 0; t < n_targets; t++)
        if (!target_threshold(e, target_mse[t], &tg.thresholds.t[t])) {
            set_error("icerx_encode_device_target: target %d is negative or not a number", t);
            return ICER_INVALID_INPUT;
        }
    if (int rc = prepare_target(e)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (upload_units(e, byte_cap, st)) return ICER_FATAL_ERROR;
    if (!stride_admissible(e, out_stride, byte_cap)) {
        set_error("icerx_encode_device_target: out_stride %zu smaller than the byte cap %zu", out_stride, byte_cap);
        return ICER_INVALID_INPUT;
    }
    if (n_targets > 1 && e->final_off.ensure((size_t)n_targets * e->max_frames * e->plan.units.size())) return ICER_FATAL_ERROR;
    const uint16_t *planes = static_cast<const uint16_t *>(d_frames);
    if (e->sample_bits == 8) {          // (as icerx_encode_device_s8)
        if (convert_samples(e, Convert::S8, static_cast<const uint8_t *>(d_frames), (size_t)n_frames * e->channels * e->w * e->h, st)) return ICER_FATAL_ERROR;
        planes = e->in.p;
    }
    e->dist_frames = n_frames;
    EncodeCall c{planes, n_frames, byte_cap, d_out, out_stride, d_sizes, d_rcs, st, true, nullptr, &tg};
    return encode_sync(e, c, caller_rows);
}

// Budget encode (include/icer_hip.h): checked here in full before anything is enqueued, then a synchronous call at the byte cap whose
// assembly cuts every budget's streams.  What the first such call of an encoder makes beyond prepare_target: the frames' curves.
int icerx_encode_device_budget(icerx_encoder *e, const void *d_frames, int n_frames, const uint64_t *budgets, int n_budgets, size_t byte_cap,
                               uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, int32_t *d_at_cap, uint64_t *d_dist,
                               uint64_t *d_equiv_quota, uint64_t *d_threshold, uint64_t *d_total, void *stream)
{
    if (int rc = enter_encode("icerx_encode_device_budget", e, d_frames && budgets && d_out && d_sizes && d_rcs && d_at_cap && d_dist && d_equiv_quota &&
                              d_threshold && d_total && n_budgets >= 1 && n_budgets <= ICERX_MAX_LADDER, n_frames, 0, 0,
                              " (1 <= n_budgets <= ICERX_MAX_LADDER, 1 <= n_frames <= max_frames)")) return rc;
    Budget bg;
    bg.n = n_budgets;
    bg.n_frames = n_frames;
    bg.d_at_cap = d_at_cap;
    bg.d_dist = reinterpret_cast<unsigned long long *>(d_dist);
    bg.d_equiv = reinterpret_cast<unsigned long long *>(d_equiv_quota);
    bg.d_threshold = reinterpret_cast<unsigned long long *>(d_threshold);
    bg.d_total = reinterpret_cast<unsigned long long *>(d_total);
    for (int b = 0; b < n_budgets; b++) bg.budgets.b[b] = budgets[b];
    if (int rc = prepare_target(e, "icerx_encode_device_budget")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (upload_units(e, byte_cap, st)) return ICER_FATAL_ERROR;
    if (!stride_admissible(e, out_stride, byte_cap)) {
        set_error("icerx_encode_device_budget: out_stride %zu smaller than the byte cap %zu", out_stride, byte_cap);
        return ICER_INVALID_INPUT;
    }
    const size_t n_units = e->plan.units.size();
    if (e->curve.ensure(2 * (size_t)e->max_frames * (n_units + 1)) || e->curve_head.ensure((size_t)e->max_frames * kCurveHeadWords) ||
        ((uint32_t)e->max_frames > kBudgetLdsFrames && e->budget_state.ensure((size_t)kMaxLadder * e->max_frames))) return ICER_FATAL_ERROR;
    if (n_budgets > 1 && e->final_off.ensure((size_t)n_budgets * e->max_frames * n_units)) return ICER_FATAL_ERROR;
    const uint16_t *planes = static_cast<const uint16_t *>(d_frames);
    if (e->sample_bits == 8) {          // (as icerx_encode_device_s8)
        if (convert_samples(e, Convert::S8, static_cast<const uint8_t *>(d_frames), (size_t)n_frames * e->channels * e->w * e->h, st)) return ICER_FATAL_ERROR;
        planes = e->in.p;
    }
    e->dist_frames = n_frames;
    EncodeCall c{planes, n_frames, byte_cap, d_out, out_stride, d_sizes, d_rcs, st, true, nullptr, nullptr, &bg};
    return encode_sync(e, c, caller_rows);
}

int icerx_get_distortion_table(icerx_encoder *e, int frame, uint64_t *dst, size_t n_entries)
{
    if (!e || !dst || !e->dist.p || frame < 0 || frame >= e->dist_frames) return ICER_INVALID_INPUT;
    const size_t per_frame = (size_t)e->plan.n_families * ((size_t)(e->sample_bits == 8 ? kPlanes8 : kPlanes) + 1);
    if (n_entries != per_frame) return ICER_INVALID_INPUT;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(dst, e->dist.p + (size_t)frame * per_frame, per_frame * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

// The distortion sidecar (include/icer_hip_sidecar.h): the table above with the frame's LL means behind it, into device memory.
size_t icerx_distortion_sidecar_entries(const icerx_encoder *e)
{
    return e ? (size_t)e->plan.n_families * ((size_t)(e->sample_bits == 8 ? kPlanes8 : kPlanes) + 1) + 1 : 0;
}

int icerx_get_distortion_sidecar_device(icerx_encoder *e, int n_frames, uint64_t *d_dst, size_t stride_entries, void *stream)
{
    if (!e || !d_dst || !e->dist.p || !e->means.p || n_frames < 1 || n_frames > e->dist_frames) return ICER_INVALID_INPUT;
    const size_t entries = icerx_distortion_sidecar_entries(e);
    if (stride_entries < entries) return ICER_INVALID_INPUT;
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(sidecar_export_kernel, dim3((unsigned)((entries + 255) / 256), (unsigned)n_frames), dim3(256), 0, (hipStream_t)stream, e->dist.p,
                       e->means.p, e->channels, (uint32_t)(entries - 1), reinterpret_cast<unsigned long long *>(d_dst), stride_entries);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The 8-bit front ends: converted into the encoder's own planes on `stream`, then icerx_encode_device on those.
static int encode_converted(const char *entry, int bits, int channels, const char *needs, Convert how, icerx_encoder *e, const uint8_t *d_src, int n_frames,
                            size_t byte_quota, uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream)
{
    if (int rc = enter_encode(entry, e, d_src && d_out && d_sizes && d_rcs, n_frames, bits, channels, needs)) return rc;
    const size_t n = (size_t)n_frames * e->w * e->h * (how == Convert::Rgb8 ? 1 : e->channels);
    if (convert_samples(e, how, d_src, n, (hipStream_t)stream)) return ICER_FATAL_ERROR;
    EncodeCall c{e->in.p, n_frames, byte_quota, d_out, out_stride, d_sizes, d_rcs, (hipStream_t)stream, true};
    return encode_sync(e, c, caller_rows);
}

int icerx_encode_device_u8(icerx_encoder *e, const uint8_t *d_frames, int n_frames, size_t byte_quota, uint8_t *d_out,
                           size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream)
{
    return encode_converted("icerx_encode_device_u8", 16, 1, " (needs a 1-channel encoder)", Convert::U8, e, d_frames, n_frames, byte_quota, d_out, out_stride,
                            d_sizes, d_rcs, stream);
}

int icerx_encode_device_s8(icerx_encoder *e, const uint8_t *d_planes, int n_frames, size_t byte_quota, uint8_t *d_out,
                           size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream)
{
    return encode_converted("icerx_encode_device_s8", 8, 0, " (needs an encoder created with sample_bits = 8)", Convert::S8, e, d_planes, n_frames, byte_quota,
                            d_out, out_stride, d_sizes, d_rcs, stream);
}

int icerx_encode_device_rgb8(icerx_encoder *e, const uint8_t *d_rgb, int n_frames, size_t byte_quota, uint8_t *d_out,
                             size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream)
{
    return encode_converted("icerx_encode_device_rgb8", 16, 3, " (needs a 3-channel encoder)", Convert::Rgb8, e, d_rgb, n_frames, byte_quota, d_out, out_stride,
                            d_sizes, d_rcs, stream);
}

int icerx_encode_host(icerx_encoder *e, const uint16_t *frames, int n_frames, size_t byte_quota, uint8_t *out,
                      size_t out_stride, uint64_t *sizes, int32_t *rcs)
{
    if (int rc = enter_encode("icerx_encode_host", e, frames && out && sizes && rcs, n_frames, 16, 0, " (needs a 16-bit encoder, 1 <= n_frames <= max_frames)")) return rc;
    const size_t plane = e->w * e->h, P = (size_t)n_frames * e->channels;
    if (e->in.ensure((size_t)e->max_frames * e->channels * plane)) return ICER_FATAL_ERROR;
    HIP_TRY(hipMemcpy(e->in.p, frames, P * plane * 2, hipMemcpyHostToDevice));
    EncodeCall c{e->in.p, n_frames, byte_quota, nullptr, 0, (uint64_t *)e->sizes.p, e->rcs.p, nullptr, true};       // (rows: encode_staged)
    if (int rc = encode_staged(e, c)) return rc;
    HIP_TRY(hipMemcpy(sizes, e->sizes.p, (size_t)n_frames * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rcs, e->rcs.p, (size_t)n_frames * 4, hipMemcpyDeviceToHost));
    // out_stride is the room the caller gives every frame: checked against the streams that came out (for one
    // frame as for many), before anything is copied
    for (int f = 0; f < n_frames; f++)
        if (sizes[f] > out_stride) {
            set_error("icerx_encode_host: stream of frame %d (%llu bytes) longer than out_stride %zu", f, (unsigned long long)sizes[f], out_stride);
            return ICER_OUTPUT_BUF_TOO_SMALL;
        }
    for (int f = 0; f < n_frames; f++)
        if (sizes[f]) HIP_TRY(hipMemcpy(out + (size_t)f * out_stride, e->out.p + (size_t)f * c.out_stride, sizes[f], hipMemcpyDeviceToHost));
    return 0;
}

// ---- a batch over the GPUs of the node (SURVEY 8b "our additions", 8e) ---------------------------------------------
int icerx_device_count(void) { return logical_device_count(); }

}  // extern "C"

// Frames are independent and a frame's transform needs the whole frame, so the batch is cut into contiguous blocks
// of frames, one per device (earlier devices take the larger blocks, icer_compression_amd/shard.py has the same rule);
// one host thread and one encoder per device, no communication between them.  Every frame's bytes, length and
// return code equal a per-frame call of icer_compress_image_uint16.
//
// A device's block is coded in sub-batches over kBatchSets (3) buffer sets, each with an encoder and an encoder stream of
// its own, plus one copy-in and one copy-out stream:
//     copy-in stream    H2D of the sub-batches ahead (set k % 3 is free when the kernels of k - 3 are done)
//     encoder streams   all kernels of sub-batch k on stream k % 3: the kernels of two sets share the chip, so that the last
//                       coding units of one launch do not leave it idle
//     copy-out stream   D2H of the streams of the finished sub-batches (exactly size[f] bytes per frame)
// (Streams are a scarce resource: the HIP runtime multiplexes them onto GPU_MAX_HW_QUEUES = 4 hardware queues by default and
// streams that share a queue run one after the other -- measured on C4 / C5: 0.80-0.85 x the device-resident rate with 4
// queues, 0.92-0.95 x with 8 -- see want_priority_streams below for what the library does about it.  Copies on the
// encoder streams instead of streams of their own -- fewer streams -- measured slower: 0.78 x on C4.)
// The encoders and their staging buffers stay alive between calls (per device, re-made when the geometry changes;
// icerx_batch_release frees them): a call allocates nothing on the device.
namespace {

// Hardware queues.  The runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default; a PROCESS-wide choice read
// once when the HIP runtime starts, which the library does not make behind the caller's back) PER PRIORITY LEVEL, and a new stream gets
// the least-used queue of its level's pool.  Round 5: unless the process has 6 or more queues per level, the four streams of a device's
// pipeline whose kernels must overlap (three encoders + their shared side stream) are created at another level than the host program's
// streams -- a pool of four queues of their own, shared with nothing else in the process (which level: pool_compute_level above); the two
// copy streams stay plain.  With queues to spare (GPU_MAX_HW_QUEUES >= 6) everything is a plain stream.  ICER_HIP_STREAM_PRIO=0|1 pins
// the choice.
bool want_priority_streams()
{
    if (const char *pv = getenv("ICER_HIP_STREAM_PRIO")) return atoi(pv) != 0;
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    return !(q && atoi(q) >= 6);
}
void warn_hw_queues_once()
{
    static std::atomic<bool> said{false};
    // (an informational notice, not a warning: only on request -- ICER_HIP_VERBOSE=1; INTEGRATION.md "Hardware queues" has the full story)
    const char *vb = getenv("ICER_HIP_VERBOSE");
    if (!want_priority_streams() || !vb || atoi(vb) == 0 || said.exchange(true)) return;
    fprintf(stderr, "libicer_hip: host-fed batch: GPU_MAX_HW_QUEUES is below 6, so the pipeline's encoder streams are low-priority streams (a hardware-queue pool "
                    "of their own; kernels of the program's own streams go first); GPU_MAX_HW_QUEUES=8 in the environment before the process initialises HIP makes them plain ones\n");
}

constexpr int kBatchSets = 3;

struct BatchDevice {
    std::mutex mu;                       // one batch call at a time per device
    int device = -1;                     // physical HIP device
    int logical = -1;                    // the device number the caller used (key of the pool)
    bool ready = false;                  // everything below exists (a rebuild that failed part-way leaves this false)
    icerx_encoder *enc[kBatchSets] = {};   // sub-batch k runs on encoder k % sets, each on a stream of its own: the kernels of
                                         // k + 1 fill the compute units that the last coding units of k leave idle
    int sub = 0;                         // most frames per sub-batch (= the encoders' max_frames)
    size_t quota = 0, dev_stride = 0;
    hipStream_t s_in = nullptr, s_enc[kBatchSets] = {}, s_out = nullptr;
    int sets = 0;                        // buffer sets / encoders in use (2..kBatchSets)
    DevBuf<uint16_t> in[kBatchSets];
    DevBuf<uint8_t> out[kBatchSets];
    DevBuf<unsigned long long> d_sizes[kBatchSets];
    DevBuf<int32_t> d_rcs[kBatchSets];
    uint64_t *h_sizes = nullptr;         // pinned: [sets][sub]
    int32_t *h_rcs = nullptr;            // pinned: [sets][sub]
    int *h_flag = nullptr;               // pinned: [sets][2]
    hipEvent_t in_ready[kBatchSets] = {}, coded[kBatchSets] = {}, out_done[kBatchSets] = {};
    void release()
    {
        ready = false;
        if (device >= 0) (void)hipSetDevice(device);
        for (int k = kBatchSets - 1; k >= 0; k--) {          // (encoder 0 owns the side stream the others borrow: last)
            if (enc[k]) { icerx_encoder_destroy(enc[k]); enc[k] = nullptr; }
            if (s_enc[k]) (void)hipStreamDestroy(s_enc[k]);
            s_enc[k] = nullptr;
            in[k].release(); out[k].release(); d_sizes[k].release(); d_rcs[k].release();
            if (in_ready[k]) (void)hipEventDestroy(in_ready[k]);
            if (coded[k]) (void)hipEventDestroy(coded[k]);
            if (out_done[k]) (void)hipEventDestroy(out_done[k]);
            in_ready[k] = coded[k] = out_done[k] = nullptr;
        }
        if (s_in) (void)hipStreamDestroy(s_in);
        if (s_out) (void)hipStreamDestroy(s_out);
        s_in = s_out = nullptr;
        if (h_sizes) (void)hipHostFree(h_sizes);
        if (h_rcs) (void)hipHostFree(h_rcs);
        if (h_flag) (void)hipHostFree(h_flag);
        h_sizes = nullptr; h_rcs = nullptr; h_flag = nullptr;
        sub = 0; sets = 0; quota = 0; dev_stride = 0;
    }
    // after an error in the middle of a call: nothing of this device's pipeline may still be reading the caller's frames or
    // writing the caller's rows when the API returns, and the pooled encoders must be idle for the next call
    void quiesce()
    {
        if (device >= 0) (void)hipSetDevice(device);
        if (s_in) (void)hipStreamSynchronize(s_in);
        for (int k = 0; k < kBatchSets; k++) {
            if (s_enc[k]) (void)hipStreamSynchronize(s_enc[k]);
            if (enc[k]) {
                if (enc[k]->side_stream) (void)hipStreamSynchronize(enc[k]->side_stream);
                enc[k]->pend.active = false; enc[k]->wg_once = false; enc[k]->ev_pending = false;
            }
        }
        if (s_out) (void)hipStreamSynchronize(s_out);
        (void)hipGetLastError();
    }
};

std::mutex g_pool_mutex;
std::map<int, std::unique_ptr<BatchDevice>> g_pool;

// (keyed by the LOGICAL device: with ICER_HIP_VIRTUAL_DEVICES every logical device has a pipeline of its own)
BatchDevice *pool_device(int logical)
{
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    auto &slot = g_pool[logical];
    if (!slot) { slot.reset(new BatchDevice()); slot->logical = logical; slot->device = physical_of(logical); }
    return slot.get();
}

// frames per sub-batch: about eight sub-batches per block (measured on C4 / C5 with three sets in flight: 4 of 32 frames and
// 2 of 8 are best, 8 / 1 cost 3-12 %), each small enough that three input + three output sets are a modest share of HBM
// (ICER_HIP_BATCH_SUB pins it)
int sub_batch_frames(int cnt, size_t frame_bytes)
{
    if (const char *sv = getenv("ICER_HIP_BATCH_SUB")) { const int v = atoi(sv); if (v >= 1) return v < cnt ? v : cnt; }
    size_t by_mem = ((size_t)256 << 20) / (frame_bytes ? frame_bytes : 1);
    if (by_mem < 1) by_mem = 1;
    int by_overlap = (cnt + 7) / 8;
    if (by_overlap < 1) by_overlap = 1;
    int sub = (size_t)by_overlap < by_mem ? by_overlap : (int)by_mem;
    // (a launch of one large gray frame is bound by the chain of its biggest coding units: prefer two per launch)
    if (sub < 2 && cnt >= 2 && frame_bytes <= ((size_t)512 << 20)) sub = 2;
    return sub;
}

// The sub-batches of a block of `cnt` frames: `sub` frames each, the last one what is left (a block that started or ended with
// smaller sub-batches was measured: C5 the same, C4 9 % slower, profiles/r04_logs/r04_a_host_batch_ramp.log)
void sub_batch_plan(int cnt, int sub, std::vector<int> *first, std::vector<int> *count)
{
    first->clear(); count->clear();
    for (int at = 0; at < cnt; at += sub) { first->push_back(at); count->push_back(std::min(sub, cnt - at)); }
}

int batch_rebuild(BatchDevice *b, size_t w, size_t h, int channels, int stages, int filt, int segments, int sub, int sets)
{
    b->sub = sub;
    b->sets = sets;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(create_level_stream(&b->s_in, want_priority_streams() ? getenv("ICER_HIP_COPY_LEVEL") : nullptr));
    HIP_TRY(create_level_stream(&b->s_out, want_priority_streams() ? getenv("ICER_HIP_COPY_LEVEL") : nullptr));
    for (int k = 0; k < sets; k++) {
        const int rc = icerx_encoder_create(&b->enc[k], b->logical, w, h, channels, stages, filt, segments, sub);
        if (rc) return rc;
        b->enc[k]->sleepy_wait = true;
        // (streams are scarce -- hardware queues, see above: the pipeline's encoders run their short list kernels on ONE side
        // stream, the first encoder's; fork / join events stay per encoder)
        if (k > 0 && b->enc[k]->side_stream && b->enc[0]->side_stream) {
            (void)hipStreamDestroy(b->enc[k]->side_stream);
            b->enc[k]->side_stream = b->enc[0]->side_stream;
            b->enc[k]->side_stream_borrowed = true;
        }
        // (the encoders' streams and their shared side stream at a level of their own unless the process has hardware queues to
        // spare: want_priority_streams, pool_compute_level)
        HIP_TRY(create_level_stream(&b->s_enc[k], want_priority_streams() ? pool_compute_level() : nullptr));
        if (k == 0 && want_priority_streams() && b->enc[0]->side_stream && !b->enc[0]->side_stream_borrowed) {
            hipStream_t ss = nullptr;                           // (the shared side stream at the encoders' level)
            if (create_level_stream(&ss, pool_compute_level()) == hipSuccess) { (void)hipStreamDestroy(b->enc[0]->side_stream); b->enc[0]->side_stream = ss; }
        }
        if (b->in[k].ensure((size_t)sub * channels * w * h) || b->d_sizes[k].ensure(sub) || b->d_rcs[k].ensure(sub)) return ICER_FATAL_ERROR;
        HIP_TRY(hipEventCreateWithFlags(&b->in_ready[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b->coded[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&b->out_done[k], hipEventDisableTiming));
    }
    HIP_TRY(hipHostMalloc((void **)&b->h_sizes, (size_t)sets * (size_t)sub * sizeof(uint64_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **)&b->h_rcs, (size_t)sets * (size_t)sub * sizeof(int32_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **)&b->h_flag, (size_t)sets * 2 * sizeof(int), hipHostMallocDefault));
    b->quota = (size_t)-1;
    return 0;
}

int batch_prepare(BatchDevice *b, size_t w, size_t h, int channels, int stages, int filt, int segments, size_t quota, int sub, int sets)
{
    const icerx_encoder *e = b->enc[0];
    if (!b->ready || !e || b->sets != sets || e->w != w || e->h != h || e->channels != channels || e->stages != stages || e->filt != filt ||
        e->segments != segments || e->sample_bits != 16 || b->sub != sub) {
        b->release();
        // (a rebuild that fails part-way -- the second encoder, a staging buffer, an event -- must not leave a half-built
        // pipeline that the next call with the same geometry would take for a complete one)
        const int rc = batch_rebuild(b, w, h, channels, stages, filt, segments, sub, sets);
        if (rc) { b->release(); return rc; }
        b->ready = true;
    }
    HIP_TRY(hipSetDevice(b->device));
    // slots for this quota, then output rows that hold the longest possible stream
    size_t ds = 0;
    for (int k = 0; k < sets; k++) {
        if (upload_units(b->enc[k], quota, b->s_enc[k])) return ICER_FATAL_ERROR;
        ds = std::max(ds, row_stride(b->enc[k], quota));
    }
    if (b->quota != quota || b->dev_stride < ds) {
        for (int k = 0; k < sets; k++) if (b->out[k].ensure((size_t)sub * ds)) return ICER_FATAL_ERROR;
        b->dev_stride = ds;
        b->quota = quota;
    }
    return 0;
}

// one device's block of the batch: frames [0, cnt) at `frames`, rows of `out` (the caller holds b->mu)
int batch_run(BatchDevice *b, const uint16_t *frames, int cnt, size_t frame_elems, int sub, int S, size_t quota, uint8_t *out, size_t out_stride,
              uint64_t *sizes, int32_t *rcs)
{
    int rc = 0;
    std::vector<int> first, count;
    sub_batch_plan(cnt, sub, &first, &count);
    const int K = (int)first.size();
    // sub-batch k as a call on its buffer set, and its verdict words
    auto call_of = [&](int k) { const int s = k % S; return EncodeCall{b->in[s].p, count[(size_t)k], quota, b->out[s].p, b->dev_stride, (uint64_t *)b->d_sizes[s].p, b->d_rcs[s].p, b->s_enc[s], false}; };
    auto flag_of = [&](int k) { return b->h_flag + 2 * (k % S); };
    // enqueue sub-batch k: its copy-in, then its kernels
    auto issue = [&](int k) -> int {
        const int s = k % S, n = count[(size_t)k];
        // in[s] is free once the kernels of k - S are done, out[s] once the copy-out of k - S is
        if (k >= S) HIP_TRY(hipStreamWaitEvent(b->s_in, b->coded[s], 0));
        HIP_TRY(hipMemcpyAsync(b->in[s].p, frames + (size_t)first[(size_t)k] * frame_elems, (size_t)n * frame_elems * 2, hipMemcpyHostToDevice, b->s_in));
        HIP_TRY(hipEventRecord(b->in_ready[s], b->s_in));
        HIP_TRY(hipStreamWaitEvent(b->s_enc[s], b->in_ready[s], 0));
        if (k >= S) HIP_TRY(hipStreamWaitEvent(b->s_enc[s], b->out_done[s], 0));
        b->enc[s]->wg_once = false;
        return encode_begin(b->enc[s], call_of(k), flag_of(k), b->coded[s]);
    };
    for (int q = 0; q < S; q++) if (accumulate_timing(b->enc[q])) return ICER_FATAL_ERROR;
    for (int k = 0; k < K && k < S; k++) if ((rc = issue(k))) return rc;
    for (int k = 0; k < K; k++) {
        const int s = k % S, n = count[(size_t)k], f0 = first[(size_t)k];
        icerx_encoder *e = b->enc[s];
        // rare: k is coded again, with larger slots or by the barrier-only coder after a time-out.  Let everything in flight finish first
        // (k + 1 was enqueued with the old slot table; its own verdict is read in its turn).  Larger slots may want longer rows, of every set:
        // the sub-batches after k that were in flight wrote rows of the old stride into buffers that are gone, so they are enqueued again.
        auto resize = [&](EncodeCall &c) -> int {
            HIP_TRY(hipDeviceSynchronize());
            const size_t ds = row_stride(e, quota);
            if (b->dev_stride < ds) {
                for (int q = 0; q < S; q++) if (b->out[q].ensure((size_t)sub * ds)) return ICER_FATAL_ERROR;
                b->dev_stride = ds;
                for (int q = k + 1; q < K && q < k + S; q++) if (int r = issue(q)) return r;
            }
            c = call_of(k);
            return 0;
        };
        EncodeCall c = call_of(k);
        if ((rc = encode_finish(e, c, flag_of(k), b->coded[s], resize))) return rc;
        // lengths and return codes of k, then exactly the bytes of every stream
        HIP_TRY(hipStreamWaitEvent(b->s_out, b->coded[s], 0));
        HIP_TRY(hipMemcpyAsync(b->h_sizes + (size_t)s * sub, b->d_sizes[s].p, (size_t)n * 8, hipMemcpyDeviceToHost, b->s_out));
        HIP_TRY(hipMemcpyAsync(b->h_rcs + (size_t)s * sub, b->d_rcs[s].p, (size_t)n * 4, hipMemcpyDeviceToHost, b->s_out));
        HIP_TRY(hipStreamSynchronize(b->s_out));
        for (int f = 0; f < n; f++) {
            const uint64_t sz = b->h_sizes[(size_t)s * sub + f];
            sizes[(size_t)f0 + f] = sz;
            rcs[(size_t)f0 + f] = b->h_rcs[(size_t)s * sub + f];
            if (sz > out_stride) {
                set_error("icerx_compress_batch_uint16: stream of frame %d (%llu bytes) longer than out_stride %zu", f0 + f, (unsigned long long)sz, out_stride);
                return ICER_OUTPUT_BUF_TOO_SMALL;
            }
            if (sz) HIP_TRY(hipMemcpyAsync(out + ((size_t)f0 + f) * out_stride, b->out[s].p + (size_t)f * b->dev_stride, sz, hipMemcpyDeviceToHost, b->s_out));
        }
        HIP_TRY(hipEventRecord(b->out_done[s], b->s_out));
        if (k + S < K && (rc = issue(k + S))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(b->s_out));
    return 0;
}

int batch_on_device(BatchDevice *b, const uint16_t *frames, int cnt, size_t w, size_t h, int channels, int stages, int filt, int segments,
                    size_t quota, uint8_t *out, size_t out_stride, uint64_t *sizes, int32_t *rcs)
{
    std::lock_guard<std::mutex> lk(b->mu);
    const size_t frame_elems = w * h * (size_t)channels;
    const int sub = sub_batch_frames(cnt, frame_elems * 2);
    int sets = 3;                        // (ICER_HIP_BATCH_SETS: 2 or 3)
    if (const char *sv = getenv("ICER_HIP_BATCH_SETS")) { const int v = atoi(sv); if (v >= 2 && v <= kBatchSets) sets = v; }
    int rc = batch_prepare(b, w, h, channels, stages, filt, segments, quota, sub, sets);
    if (rc) return rc;
    rc = batch_run(b, frames, cnt, frame_elems, sub, sets, quota, out, out_stride, sizes, rcs);
    // every error exit of the pipeline ends here: drain the device's streams before the caller gets its buffers back
    if (rc) b->quiesce();
    return rc;
}

}  // namespace

extern "C" {

void icerx_batch_release(void)
{
    std::lock_guard<std::mutex> lk(g_pool_mutex);
    for (auto &kv : g_pool) if (kv.second) { std::lock_guard<std::mutex> lk2(kv.second->mu); kv.second->release(); }
}

int icerx_compress_batch_uint16_devices(const uint16_t *frames, int n_frames, size_t w, size_t h, int channels, int stages, int filt,
                                        int segments, size_t byte_quota, uint8_t *out, size_t out_stride, uint64_t *sizes, int32_t *rcs,
                                        const int *devices, int n_devices)
{
    if (!frames || !out || !sizes || !rcs || n_frames < 1 || !devices || n_devices < 1) { set_error("icerx_compress_batch_uint16: invalid arguments"); return ICER_INVALID_INPUT; }
    const int have = icerx_device_count();
    if (have <= 0) { set_error("no usable HIP device; this library has no CPU path"); return ICER_FATAL_ERROR; }
    for (int d = 0; d < n_devices; d++)
        if (devices[d] < 0 || devices[d] >= have) { set_error("icerx_compress_batch_uint16: device %d of %d present", devices[d], have); return ICER_INVALID_INPUT; }
    warn_hw_queues_once();
    const int g = n_devices > n_frames ? n_frames : n_devices;
    try {
        std::vector<int> rc((size_t)g, 0);
        std::vector<std::string> err((size_t)g);
        const size_t frame_elems = w * h * (size_t)channels;
        auto work = [&](int d) {
            const int base = n_frames / g, extra = n_frames % g;
            const int lo = d * base + (d < extra ? d : extra), cnt = base + (d < extra ? 1 : 0);
            int r;
            try {
                g_last_error.clear();                            // (thread-local: what this block's failure leaves, if anything)
                r = batch_on_device(pool_device(devices[d]), frames + (size_t)lo * frame_elems, cnt, w, h, channels, stages, filt, segments,
                                    byte_quota, out + (size_t)lo * out_stride, out_stride, sizes + lo, rcs + lo);
                if (r) err[(size_t)d] = g_last_error.empty() ? "error code " + std::to_string(r) + " (lib_icer argument check)" : g_last_error;
            } catch (const std::exception &ex) { r = ICER_FATAL_ERROR; err[(size_t)d] = ex.what(); }
            rc[(size_t)d] = r;
        };
        if (g == 1) work(0);
        else {
            // one host thread per device, on the cores next to that device (its NUMA node): the thread allocates the
            // device's page-locked staging words and polls its events
            std::vector<std::thread> th;
            for (int d = 0; d < g; d++)
                th.emplace_back([&work, devices, d] { (void)pin_thread_near_device(physical_of(devices[d])); work(d); });
            for (auto &t : th) t.join();
        }
        int first = 0;
        std::string all;
        for (int d = 0; d < g; d++)
            if (rc[(size_t)d]) { if (!first) first = rc[(size_t)d]; all += (all.empty() ? "device " : "; device ") + std::to_string(devices[d]) + ": " + err[(size_t)d]; }
        if (first) { set_error("%s", all.c_str()); return first; }
        return 0;
    } catch (const std::exception &ex) {          // (std::thread / std::vector: nothing may cross the C boundary)
        set_error("icerx_compress_batch_uint16: %s", ex.what());
        return ICER_FATAL_ERROR;
    }
}

int icerx_compress_batch_uint16(const uint16_t *frames, int n_frames, size_t w, size_t h, int channels, int stages, int filt,
                                int segments, size_t byte_quota, uint8_t *out, size_t out_stride, uint64_t *sizes, int32_t *rcs,
                                int n_gpus)
{
    if (n_gpus < 0) { set_error("icerx_compress_batch_uint16: invalid arguments"); return ICER_INVALID_INPUT; }
    const int have = icerx_device_count();
    if (have <= 0) { set_error("no usable HIP device; this library has no CPU path"); return ICER_FATAL_ERROR; }
    const int g = n_gpus == 0 || n_gpus > have ? have : n_gpus;
    int devices[64];
    for (int d = 0; d < g && d < 64; d++) devices[d] = d;
    return icerx_compress_batch_uint16_devices(frames, n_frames, w, h, channels, stages, filt, segments, byte_quota, out, out_stride, sizes,
                                               rcs, devices, g < 64 ? g : 64);
}

// Page-lock a caller buffer (frames in, streams out) so that the host-buffer entry points move it at PCIe speed by DMA
// instead of through the runtime's staging copies (hipHostRegister / hipHostUnregister behind a C ABI: a C caller need
// not link the HIP runtime).  The caller unpins before it frees the memory.
int icerx_pin_host(void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return ICER_INVALID_INPUT;
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return 0;
}
int icerx_unpin_host(void *ptr)
{
    if (!ptr) return ICER_INVALID_INPUT;
    HIP_TRY(hipHostUnregister(ptr));
    return 0;
}

int icerx_get_coefficients(icerx_encoder *e, int frame, int channel, uint16_t *dst)
{
    if (!e || frame < 0 || frame >= e->max_frames || channel < 0 || channel >= e->channels) return ICER_INVALID_INPUT;
    HIP_TRY(hipSetDevice(e->device));
    const size_t plane = e->w * e->h;
    HIP_TRY(hipMemcpy(dst, e->coef.p + ((size_t)frame * e->channels + channel) * plane, plane * 2, hipMemcpyDeviceToHost));
    return 0;
}

int icerx_timing_enable(icerx_encoder *e, int on)
{
    if (!e) return ICER_INVALID_INPUT;
    e->timing = on != 0;
    return 0;
}

int icerx_timing_read(icerx_encoder *e, double ms[ICERX_NUM_STAGES], uint64_t *calls, int reset)
{
    if (!e) return ICER_INVALID_INPUT;
    HIP_TRY(hipSetDevice(e->device));
    if (accumulate_timing(e)) return ICER_FATAL_ERROR;
    for (int i = 0; i < ICERX_NUM_STAGES; i++) ms[i] = e->ms[i];
    *calls = e->timed_calls;
    if (reset) { for (auto &m : e->ms) m = 0; e->timed_calls = 0; }
    return 0;
}

// the same counters summed over every encoder of the process (the lib_icer-shaped entry points use an internal one)
int icerx_process_stats(uint64_t out[4])
{
    if (!out) return ICER_INVALID_INPUT;
    out[0] = g_stats[0]; out[1] = g_stats[1]; out[2] = g_stats[2]; out[3] = 0;
    return 0;
}

int icerx_encoder_stats(icerx_encoder *e, uint64_t out[4])
{
    if (!e || !out) return ICER_INVALID_INPUT;
    out[0] = e->n_timeouts; out[1] = e->n_fallbacks; out[2] = e->n_slot_retries; out[3] = (uint64_t)e->tuning.coder;
    return 0;
}

int icerx_encoder_routing(icerx_encoder *e, uint64_t out[2])
{
    if (!e || !out) return ICER_INVALID_INPUT;
    out[0] = e->n_routed_units; out[1] = e->n_routed_launches;
    return 0;
}

int icerx_encoder_launch_info(icerx_encoder *e, uint32_t out[4])
{
    if (!e || !out) return ICER_INVALID_INPUT;
    // (the last call: split if a part split, the sub-range workgroups of all parts, routed if a part routed)
    const LaunchPlan &lp = e->last_plan;
    out[0] = out[1] = out[3] = 0;
    for (int k = 0; k < lp.n_parts; k++) { out[0] |= lp.part[k].split; out[1] += lp.part[k].subs; out[3] |= lp.part[k].hybrid; }
    out[2] = lp.use_wg ? 0u : lp.part[lp.n_parts - 1].pipe == PipeKernel::Large ? (uint32_t)kUnitWavesLarge : (uint32_t)kUnitWavesSmall;
    return 0;
}

int icerx_encoder_parts(icerx_encoder *e) { return e ? e->last_plan.n_parts : ICER_INVALID_INPUT; }

int icerx_info(icerx_encoder *e, uint32_t *units_per_frame, uint32_t *slot_bits_per_pixel, uint64_t *slot_bytes_per_frame)
{
    if (!e) return ICER_INVALID_INPUT;
    *units_per_frame = (uint32_t)e->plan.units.size();
    *slot_bits_per_pixel = e->bits_per_pixel;
    *slot_bytes_per_frame = e->plan.slot_bytes;
    return 0;
}

#ifdef ICER_PHASE_TIMERS
// profiling build only: summed s_memtime cycles per coder phase over all units since the last reset
int icerx_prof_read(icerx_encoder *e, uint64_t out[9 * 32], int reset)
{
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(out, e->prof.p, 9 * 32 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(e->prof.p, 0, kProfWords * sizeof(uint64_t)));
    return 0;
}
// the same for the small window coder beside the pipeline (code_units_list_kernel): 9 rows of 32
int icerx_prof_read_wgs(icerx_encoder *e, uint64_t out[9 * 32], int reset)
{
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpy(out, e->prof.p + kProfWgsOffset, 9 * 32 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(e->prof.p + kProfWgsOffset, 0, 9 * 32 * sizeof(uint64_t)));
    return 0;
}
// per list entry of code_units_list_kernel (frame 0, position < kListTrace): start / end (100 MHz wall clock), workgroup | unit << 32,
// lsb | level << 8 | subband << 16 | segment << 24 | chunks << 32
int icerx_prof_list_trace(icerx_encoder *e, uint64_t *out, int n_entries, int reset)
{
    if (!e || !out || n_entries < 0) return ICER_INVALID_INPUT;
    HIP_TRY(hipSetDevice(e->device));
    if (n_entries > kListTrace) n_entries = kListTrace;
    HIP_TRY(hipMemcpy(out, e->prof.p + kProfWgsOffset + 9 * 32, (size_t)n_entries * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(e->prof.p + kProfWgsOffset + 9 * 32, 0, (size_t)kListTrace * 4 * sizeof(uint64_t)));
    return n_entries;
}
// per workgroup of frame 0 (launch position b < kTraceUnits): start / end (100 MHz wall clock), HW_ID | XCC_ID << 32, unit index
int icerx_prof_trace(icerx_encoder *e, uint64_t *out, int n_blocks)
{
    if (!e || !out || n_blocks < 0) return ICER_INVALID_INPUT;
    HIP_TRY(hipSetDevice(e->device));
    if (n_blocks > kTraceUnits) n_blocks = kTraceUnits;
    HIP_TRY(hipMemcpy(out, e->prof.p + 9 * 32, (size_t)n_blocks * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    uint64_t hw[16];
    HIP_TRY(hipMemcpy(hw, e->prof.p + 9 * 32 + 4 * kTraceUnits, sizeof hw, hipMemcpyDeviceToHost));
    fprintf(stderr, "workgroup 0, wave -> SIMD:");
    for (int w = 0; w < kUnitWavesLarge; w++) fprintf(stderr, " %d->%d", w, (int)((hw[w] >> 4) & 3));
    fprintf(stderr, "\n");
    return n_blocks;
}
#endif

// ---- lib_icer drop-in entry points -------------------------------------------------------------
static icerx_encoder *g_cached = nullptr;

// `planes` are uint16_t* (sample_bits 16) or uint8_t* (sample_bits 8) host pointers
static int compress_planes(void *const planes[], int channels, size_t w, size_t h, int stages, int filt, int segments,
                           icer_output_data_buf_typedef *od, int sample_bits)
{
    std::lock_guard<std::recursive_mutex> lk(g_mutex);
    if (!od) return ICER_INVALID_INPUT;
    icerx_encoder *e = g_cached;
    if (!e || e->w != w || e->h != h || e->channels != channels || e->stages != stages || e->filt != filt ||
        e->segments != segments || e->sample_bits != sample_bits) {
        if (e) { icerx_encoder_destroy(e); g_cached = nullptr; }
        const char *dev = getenv("ICER_HIP_DEVICE");
        const int rc = icerx_encoder_create_ex(&e, dev ? atoi(dev) : 0, w, h, channels, stages, filt, segments, 1, sample_bits);
        if (rc == ICER_PACKET_COUNT_EXCEEDED || rc == ICER_TOO_MANY_SEGMENTS) {
            // The reference finds its packet table too small, or the segment grid impossible, only after the transform
            // and the LL-mean check (icer_color.c:31-131, icer_compress.c:279-400): an integer overflow there is what it
            // reports.  Run those on the planes as gray frames with one segment and look at their return codes.
            icerx_encoder *t = nullptr;
            if (icerx_encoder_create_ex(&t, dev ? atoi(dev) : 0, w, h, 1, stages, filt, 1, channels, sample_bits) == 0) {
                const size_t plane = w * h, n = (size_t)channels * plane;
                std::vector<int32_t> rcs(channels, 0);
                int r = 0;
                if (t->in.ensure(n) || (sample_bits == 8 && t->in8.ensure(n))) r = ICER_FATAL_ERROR;
                for (int c = 0; c < channels && !r; c++) {
                    const hipError_t he = sample_bits == 8 ? hipMemcpy(t->in8.p + (size_t)c * plane, planes[c], plane, hipMemcpyHostToDevice)
                                                           : hipMemcpy(t->in.p + (size_t)c * plane, planes[c], plane * 2, hipMemcpyHostToDevice);
                    if (he != hipSuccess) r = ICER_FATAL_ERROR;
                }
                if (!r && sample_bits == 8) r = convert_samples(t, Convert::S8, t->in8.p, n, nullptr);
                if (!r) {
                    EncodeCall c{t->in.p, channels, 64, nullptr, 0, (uint64_t *)t->sizes.p, t->rcs.p, nullptr, true};
                    r = encode_staged(t, c);
                    if (!r && hipMemcpy(rcs.data(), t->rcs.p, sizeof(int32_t) * channels, hipMemcpyDeviceToHost) != hipSuccess) r = ICER_FATAL_ERROR;
                }
                icerx_encoder_destroy(t);
                if (r) return r;
                for (int c = 0; c < channels; c++) if (rcs[c] == ICER_INTEGER_OVERFLOW) return ICER_INTEGER_OVERFLOW;
            }
        }
        if (rc) return rc;
        g_cached = e;
    }
    // The call as a reference user makes it (example/src/example_encode.c:36-77): pageable caller memory in, stream and
    // coefficient planes out.  Everything runs on a stream of the encoder's own; the coefficient planes -- final once the
    // transform is done, 0.2 ms into the call -- go back to the caller's image on a second stream WHILE the coder runs, so
    // that of the three transfers only the upload and the (short) stream download are not hidden.
    const size_t plane = w * h, quota = od->size_allocated;
    HIP_TRY(hipSetDevice(e->device));
    if (!e->io_stream) HIP_TRY(hipStreamCreateWithFlags(&e->io_stream, hipStreamNonBlocking));
    if (!e->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking));
    if (!e->coef_ready) HIP_TRY(hipEventCreateWithFlags(&e->coef_ready, hipEventDisableTiming));
    hipStream_t st = e->io_stream;
    if (e->in.ensure((size_t)channels * plane)) return ICER_FATAL_ERROR;
    if (sample_bits == 16) {
        for (int c = 0; c < channels; c++)
            HIP_TRY(hipMemcpyAsync(e->in.p + (size_t)c * plane, planes[c], plane * 2, hipMemcpyHostToDevice, st));
    } else {
        if (e->in8.ensure((size_t)channels * plane)) return ICER_FATAL_ERROR;
        for (int c = 0; c < channels; c++)
            HIP_TRY(hipMemcpyAsync(e->in8.p + (size_t)c * plane, planes[c], plane, hipMemcpyHostToDevice, st));
        if (convert_samples(e, Convert::S8, e->in8.p, (size_t)channels * plane, st)) return ICER_FATAL_ERROR;
    }
    uint64_t size = 0;
    int32_t rc = 0;
    bool coef_back = false;              // the coefficient planes are in the caller's image already
    // begin, copy the coefficients back beside the coder, finish
    EncodeCall call{e->in.p, 1, quota, nullptr, 0, (uint64_t *)e->sizes.p, e->rcs.p, st, false};
    if (upload_units(e, quota, st) || stage_rows(e, call)) return ICER_FATAL_ERROR;
    if (accumulate_timing(e)) return ICER_FATAL_ERROR;
    e->wg_once = false;
    if (int r = encode_begin(e, call, e->h_flag, e->done)) return r;
    {   // beside the coder: the frame's status (an aborted frame keeps the caller's planes, see below), then the planes
        int skip = 0;
        HIP_TRY(hipStreamWaitEvent(e->copy_stream, e->coef_ready, 0));
        HIP_TRY(hipMemcpyAsync(&skip, e->skip(0), sizeof(int), hipMemcpyDeviceToHost, e->copy_stream));
        HIP_TRY(hipStreamSynchronize(e->copy_stream));
        if (!skip) {
            if (sample_bits == 16) {
                for (int c = 0; c < channels; c++)
                    HIP_TRY(hipMemcpyAsync(planes[c], e->coef.p + (size_t)c * plane, plane * 2, hipMemcpyDeviceToHost, e->copy_stream));
            } else {
                // what the reference leaves in the caller's image: int8 sign-magnitude bytes; narrowed on the device (in8 is
                // free again: the widening kernel has run, coef_ready lies behind it on the encode stream)
                if (convert_samples(e, Convert::NarrowSm8, nullptr, (size_t)channels * plane, e->copy_stream)) return ICER_FATAL_ERROR;
                for (int c = 0; c < channels; c++)
                    HIP_TRY(hipMemcpyAsync(planes[c], e->in8.p + (size_t)c * plane, plane, hipMemcpyDeviceToHost, e->copy_stream));
            }
            HIP_TRY(hipStreamSynchronize(e->copy_stream));
            coef_back = true;
        }
    }
    if (int r = encode_finish(e, call, e->h_flag, e->done, [e](EncodeCall &again) { return stage_rows(e, again); })) return r;
    HIP_TRY(hipMemcpyAsync(&size, e->sizes.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&rc, e->rcs.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (rc == ICER_INTEGER_OVERFLOW) {
        // The reference aborts before any output; it leaves transformed (not sign-magnitude) data in
        // the planes it had already processed: channels up to the first DWT overflow, or all of them
        // when only the LL-mean check failed (icer_color.c:347-381).  (uint8 twins: that data went through
        // truncating int8 stores after the overflow; we leave the caller's planes untouched instead.)
        if (sample_bits == 8) return rc;
        std::vector<int> fl(2 * (size_t)channels);
        HIP_TRY(hipMemcpy(fl.data(), e->dwt_ovf(0), sizeof(int) * channels, hipMemcpyDeviceToHost));
        int last = channels - 1;
        for (int c = 0; c < channels; c++) if (fl[c]) { last = c; break; }
        // (the detail bands are normally stored as sign-magnitude words: transform once more, plain)
        {
            size_t cw2 = w, ch2 = h;
            launch_dwt(e, reinterpret_cast<const uint16_t *>(e->in.p), 1, st, 0, /* scratch */ e->dwt_ovf(0), &cw2, &ch2);
            HIP_TRY(hipStreamSynchronize(st));
        }
        for (int c = 0; c <= last; c++)
            HIP_TRY(hipMemcpy(planes[c], e->coef.p + (size_t)c * plane, plane * 2, hipMemcpyDeviceToHost));
        return rc;
    }
    if (size) HIP_TRY(hipMemcpyAsync(od->rearrange_start, e->out.p, size, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!coef_back) {                    // (not reached in practice: a frame that was not aborted has its planes back already)
        if (sample_bits == 16) {
            for (int c = 0; c < channels; c++)
                HIP_TRY(hipMemcpy(planes[c], e->coef.p + (size_t)c * plane, plane * 2, hipMemcpyDeviceToHost));
        } else {
            if (convert_samples(e, Convert::NarrowSm8, nullptr, (size_t)channels * plane, st)) return ICER_FATAL_ERROR;
            for (int c = 0; c < channels; c++)
                HIP_TRY(hipMemcpyAsync(planes[c], e->in8.p + (size_t)c * plane, plane, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    }
    od->size_used = size;
    return rc;
}

int icer_compress_image_uint16(uint16_t *image, size_t image_w, size_t image_h, uint8_t stages,
                               enum icer_filter_types filt, uint8_t segments, icer_output_data_buf_typedef *output_data)
{
    void *planes[1] = {image};
    return compress_planes(planes, 1, image_w, image_h, stages, (int)filt, segments, output_data, 16);
}

int icer_compress_image_yuv_uint16(uint16_t *y_channel, uint16_t *u_channel, uint16_t *v_channel, size_t image_w,
                                   size_t image_h, uint8_t stages, enum icer_filter_types filt, uint8_t segments,
                                   icer_output_data_buf_typedef *output_data)
{
    void *planes[3] = {y_channel, u_channel, v_channel};
    return compress_planes(planes, 3, image_w, image_h, stages, (int)filt, segments, output_data, 16);
}

int icer_compress_image_uint8(uint8_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt,
                              uint8_t segments, icer_output_data_buf_typedef *output_data)
{
    void *planes[1] = {image};
    return compress_planes(planes, 1, image_w, image_h, stages, (int)filt, segments, output_data, 8);
}

int icer_compress_image_yuv_uint8(uint8_t *y_channel, uint8_t *u_channel, uint8_t *v_channel, size_t image_w, size_t image_h,
                                  uint8_t stages, enum icer_filter_types filt, uint8_t segments,
                                  icer_output_data_buf_typedef *output_data)
{
    void *planes[3] = {y_channel, u_channel, v_channel};
    return compress_planes(planes, 3, image_w, image_h, stages, (int)filt, segments, output_data, 8);
}

}  // extern "C"
