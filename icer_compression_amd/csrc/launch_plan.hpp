// launch_plan.hpp -- the encoder's launch policy: which kernels an encode call launches, in which instances and shapes, in how many
// parts.  Host-only (plain C++17, like plan.hpp), so that tests/test_launch_plan.py pins every decision on a CPU; api.hip maps the
// kernel instances (the enum classes below) to its template instantiations and keeps only buffer offsets and launches.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace icer {

constexpr int kMaxParts = 4;                 // parts of a batch in flight per call
// Settled by measurement (the records under profiles/):
constexpr int kSplitPlanes = 1;              // launches of at most this many planes are cut into sub-ranges (one gray frame)
constexpr int kListWgsPerCu = 2;             // list kernel workgroups per compute unit in a batch launch (C4 6 525 -> 6 664, C5 6 526 -> 6 671 Mpix/s;
                                             // 3: the same, 4: C5 + 0.5 %, C4 - 1.8 %, 8: C5 - 5 %, profiles/r06_logs/r06t_list_grid.log); a split
                                             // launch: one per compute unit (128: 6.8 ms, 256: 5.9, 512: 7.25, profiles/r06_logs/r06u_lone_list_grid.log)
constexpr uint32_t kSplitRoutePercent = 90;  // a split launch: units with at least this share of blank chunks go to the list kernel
constexpr uint32_t kNoSplitPercent = 20;     // ... and units with at least this share are not cut (their words stay open for long stretches)
constexpr uint32_t kListHeavyMin = 64;       // listed units with at least this many chunks that are not blank are taken first (route_units_kernel)

// The encoder settings that can still be set from the environment, with their defaults (parse_tuning).
struct Tuning {
    int coder = 0;                   // ICER_HIP_CODER: 0 = by call, 1 = always the pipeline (pipe), 2 = always the window coder (wg)
    int pipe_waves = 0;              // ICER_HIP_PIPE_WAVES=8|11: pins the pipeline's workgroup shape (0: by launch)
    int hybrid_percent = 95;         // ICER_HIP_HYBRID: units with at least this share of blank chunks go to the list kernel (0: none)
    int hybrid_frames = 2;           // ICER_HIP_HYBRID_FRAMES: ... in launches of at least this many planes (frames x channels)
    int split_chunks = 1;            // ICER_HIP_SPLIT: chunks per sub-range (0: off; 1: by geometry, plan.hpp auto_split_chunks)
    int list_waves = 0;              // ICER_HIP_LIST_WAVES=1|2|4: pins the list kernel's instance (0: by launch)
    int slot_bpp = 3;                // ICER_HIP_SLOT_BPP: initial slot bound in bits per pixel (doubled on overflow)
    int overlap_parts = 2;           // ICER_HIP_OVERLAP_PARTS: parts a synchronous batch call is enqueued in (1: one stream)
    int fail_frame = -1, fail_unit = -1, fail_calls = 0;   // ICER_HIP_TEST_FAIL_UNIT=<frame>:<unit>[:<calls>] (test hook)
};

// `get(name)` returns the variable's value or nullptr (getenv in the library); a value out of range leaves the default
template <class Get> inline Tuning parse_tuning(Get &&get)
{
    Tuning t;
    auto num = [&](const char *name, int *to, bool (*ok)(int)) { if (const char *v = get(name)) if (ok(atoi(v))) *to = atoi(v); };
    if (const char *v = get("ICER_HIP_CODER")) t.coder = !strcmp(v, "pipe") ? 1 : !strcmp(v, "wg") ? 2 : 0;
    num("ICER_HIP_PIPE_WAVES", &t.pipe_waves, [](int x) { return x == 8 || x == 11; });
    num("ICER_HIP_HYBRID", &t.hybrid_percent, [](int x) { return x >= 0 && x <= 100; });
    num("ICER_HIP_HYBRID_FRAMES", &t.hybrid_frames, [](int x) { return x >= 1; });
    num("ICER_HIP_SPLIT", &t.split_chunks, [](int x) { return x == 0 || x >= 128; });
    num("ICER_HIP_LIST_WAVES", &t.list_waves, [](int x) { return x == 1 || x == 2 || x == 4; });
    num("ICER_HIP_SLOT_BPP", &t.slot_bpp, [](int x) { return x >= 1 && x <= 24; });
    num("ICER_HIP_OVERLAP_PARTS", &t.overlap_parts, [](int x) { return x >= 1 && x <= kMaxParts; });
    if (const char *v = get("ICER_HIP_TEST_FAIL_UNIT")) {
        int f = -1, u = -1, c = 1;
        if (sscanf(v, "%d:%d:%d", &f, &u, &c) >= 2 && f >= 0 && f < (1 << 11) && u >= 0 && u < (1 << 20) && c >= 1) { t.fail_frame = f; t.fail_unit = u; t.fail_calls = c; }
    }
    return t;
}

struct LaunchShape {
    int channels = 1, max_frames = 1;
    size_t w = 0, h = 0;
    int n_cus = 256; uint32_t n_subs = 0;   // compute units of the device; sub-range workgroups planned per frame (Plan::subs; 0: none)
};

// the window coder's LDS block was granted; this call re-runs a batch on it (after a unit time-out); the encoder has the stream of a
// batch's odd parts
struct CoderState { bool wg_available = true, wg_once = false, half_stream = false; };

enum class ListKernel : uint8_t { One, Small, Four };    // code_units_list_kernel<WgOne | WgSmall | WgFour>
enum class PipeKernel : uint8_t { Large, Lone, Batch };  // code_units_kernel<11, 1, 0> | <8, 1, kLonePadBytes> | <8, 8, 0>
enum class WindowKernel : uint8_t { Four, Full };        // code_units_wg_kernel<WgFour | WgFull>

struct PartPlan {
    int f0 = 0, n_frames = 0;        // the frames [f0, f0 + n_frames) of the call
    bool hybrid = false, split = false;   // the list kernel takes the all-but-blank units; dense units are cut into sub-ranges
    uint32_t subs = 0;               // sub-range workgroups per frame (0 unless split)
    uint32_t list_grid = 0, route_percent = 0;   // (hybrid) workgroups of the list kernel; share of blank chunks that routes a unit to it
    ListKernel list = ListKernel::One;
    PipeKernel pipe = PipeKernel::Large;        // (pipeline)
    bool position_major = false;                // (pipeline) workgroups position-major over the frames instead of frame by frame
    WindowKernel window = WindowKernel::Full;   // (window coder alone)
};

struct LaunchPlan {
    bool progressive = false;        // quota far below the lossless size: units in priority order, stopped once it is spent
    bool use_wg = false;             // the window coder codes every unit (no pipeline kernel)
    int n_parts = 1;
    PartPlan part[kMaxParts];
};

// Whether the units are planned with sub-ranges: for encoders of a few planes only (a split launch has at most kSplitPlanes, and the
// sub-ranges' private slot areas and snapshots are per frame), and only when a split launch is possible at all -- a YUV encoder would
// otherwise carry sub-range areas in every frame's slots that no launch ever uses.
inline bool plans_sub_ranges(const LaunchShape &s, const Tuning &t, bool wg_available)
{ return wg_available && t.coder == 0 && s.max_frames * s.channels <= 4 && s.channels <= kSplitPlanes && t.hybrid_percent > 0 && t.split_chunks > 0; }

// Whether an encoder gets the stream of a batch's odd parts (api.hip create_part_events): batches of four frames or more can be parts.
inline bool wants_half_stream(const LaunchShape &s, const Tuning &t) { return s.max_frames >= 4 && t.overlap_parts > 1; }

// `overlap_ok`: the call may be enqueued in parts on two streams (the synchronous entry points).  `code_all`: the call's cut is not a
// prefix of the priority order (a region-of-interest call), so every unit is coded whatever the quota: never progressive mode.
inline LaunchPlan plan_launch(const LaunchShape &s, const Tuning &t, const CoderState &st, int n_frames, size_t quota, bool overlap_ok,
                              bool code_all = false)
{
    LaunchPlan p;
    const int C = s.channels;
    // Progressive mode: with a byte quota far below the lossless size only the first part of the priority order can end up in
    // the stream.  The units are then launched in priority order with the quota: a unit whose finished higher-priority
    // predecessors alone already exceed it stops (at its start, or at its next check) -- see quota_already_spent.  Not used
    // for large quotas, where the launch order is largest-first instead.
    p.progressive = !code_all && quota < s.w * s.h * C / 2;
    p.use_wg = st.wg_available && (st.wg_once || t.coder == 2 || (t.coder == 0 && p.progressive));
    // Both coders in one launch: the bit planes that are mostly runs of blank chunks go to the list kernel (the window coder,
    // which closes such runs in closed form), the dense ones to the pipeline (route_units_kernel).  A launch of very few planes
    // (a single frame) cannot fill the chip with whole coding units: its dense units are cut into sub-ranges, one workgroup
    // each, and its all-but-blank ones go to the list kernel as in a batch.
    const bool shared = st.wg_available && !p.use_wg && !p.progressive && t.coder == 0 && t.hybrid_percent > 0;
    if (overlap_ok && t.overlap_parts > 1 && st.half_stream && !p.progressive && t.coder == 0 && !st.wg_once && n_frames >= 2 * t.overlap_parts &&
        n_frames * C >= t.hybrid_frames)
        p.n_parts = t.overlap_parts;
    for (int k = 0, f0 = 0; k < p.n_parts; k++) {
        const int n = n_frames / p.n_parts + (k < n_frames % p.n_parts ? 1 : 0);       // (two parts: the first one takes the odd frame)
        const int planes = n * C;
        PartPlan &q = p.part[k];
        q.f0 = f0; q.n_frames = n;
        q.split = shared && t.split_chunks > 0 && planes <= kSplitPlanes && s.n_subs > 0;
        q.subs = q.split ? s.n_subs : 0u;
        q.hybrid = q.split || (shared && planes >= t.hybrid_frames);
        if (q.hybrid) {
            q.list_grid = (uint32_t)(q.split ? s.n_cus : s.n_cus * kListWgsPerCu);
            q.route_percent = q.split ? kSplitRoutePercent : (uint32_t)t.hybrid_percent;
            // Which instance: measured (profiles/r04_logs/r04_h_list_waves.log).  A batch runs the ONE-wave instance: C4 + 4.2 %,
            // C5 + 2.0 % -- its list is thousands of all-blank units (a first window, then closed-form runs: nothing for a second
            // wave to do but wait at the barriers), and one resident wave of ~ 180 registers leaves the pipeline's workgroups more
            // of the compute unit than two of 204.  The launch of a single frame wants MORE waves per listed unit (7.8 ms with one,
            // 6.4 with two, 6.07 with FOUR, 8.7 with eight -- LDS; profiles/r04_logs/r04_zh_list_kernel_width.log): its list is led
            // by fifty long mid-sparse chains, where every further wave's chunk of a window is progress.
            const int waves = t.list_waves ? t.list_waves : (q.split ? 4 : 1);
            q.list = waves == 1 ? ListKernel::One : waves == 4 ? ListKernel::Four : ListKernel::Small;
        }
        if (!p.use_wg) {
            // The shape of the pipeline's workgroups: one frame alone cannot fill the chip and is bound by the chain of its largest
            // units, which the large shape (two pixel waves, golomb state wave + two workers) shortens; a batch wants the occupancy
            // of the small one, and so does a split launch, which fills the chip (6.63 against 6.78 ms on the headline frame).  A
            // split launch is bound by the chains of its largest units, not by occupancy: it runs the build without the register
            // budget, padded to the LDS footprint of the queue-depth-8 build (49 KiB; measured on the headline frame: 37 KiB
            // 7.5 ms, 45.6 KiB 6.8 ms, 49.5 KiB 6.7-6.8 ms, profiles/archive/r03_logs/r03_aa.log, r03_ab.log).
            const bool large = t.pipe_waves ? t.pipe_waves == 11 : (n == 1 && !q.split);
            q.pipe = large ? PipeKernel::Large : planes <= kSplitPlanes ? PipeKernel::Lone : PipeKernel::Batch;
            // (a batch that is not in progressive mode -- there the priority order across frames does not matter, the order
            // within a frame does -- is launched position-major over its frames)
            q.position_major = n > 1 && !p.progressive;
        } else {
            q.window = p.progressive || planes >= 4 ? WindowKernel::Four : WindowKernel::Full;   // (kernels.hpp code_units_wg_kernel)
        }
        f0 += n;
    }
    return p;
}

}  // namespace icer
