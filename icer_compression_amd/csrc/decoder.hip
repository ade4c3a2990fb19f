// decoder.hip -- C ABI of libicer_hip_dec.so (include/icer_hip_dec.h) and the host-side pipeline of the decoder, for
// a BATCH of streams (the lib_icer-shaped entry points are batches of one):
//   streams -> device | header candidates (one thread per byte offset, grid.y = stream) | payload CRCs (one thread per
//   candidate) | host: per stream the packet walk, table and chains (decoder_plan.hpp) | decode kernel over the
//   chains of all streams (one wavefront per chain; one thread per chain with ICER_DEC_WAVE=0) | if the decoder asks
//   for it, truncated coefficients part-way into their interval (decoder_recon.hpp) | sign-magnitude removal + LL mean | inverse DWT, one level at a time, one thread per line, all frames of a geometry per launch
//   | clamp, narrow, copy back.
// decode_batch runs that as five stages over one BatchRun: batch_packets, batch_plans, batch_chains, batch_samples, batch_results.
// Which kernel takes a chain, in what order and with how much LDS: decoder_route.hpp (route_batch_chains; shared with the async decode).
// icerx_decode_device_async runs the same chain kernels with everything planned on the device (decoder_async.hpp).
// First version: correctness before speed (HISTORY.md 6b (summary: DESIGN.md 8)); every loop is bounded by the stream / image size and no
// kernel waits on another thread.
#ifdef ICER_HOST_MOCK
#define ICER_LAUNCH_PLANES(kernel, grid, shmem, ...) ICER_LAUNCH_WAVE(kernel, grid, shmem, __VA_ARGS__)
#define ICER_LAUNCH_WAVE_ON(stream, kernel, grid, shmem, ...) ICER_LAUNCH_WAVE(kernel, grid, shmem, __VA_ARGS__)
#define ICER_LAUNCH_ON(stream, kernel, grid, block, shmem, ...) ICER_LAUNCH(kernel, grid, block, shmem, __VA_ARGS__)
#define ICER_LAUNCH_PLANES_ON(stream, kernel, grid, shmem, ...) ICER_LAUNCH_PLANES(kernel, grid, shmem, __VA_ARGS__)
#else
#include <hip/hip_runtime.h>
// kernel launches go through these two macros so that tests/emu/hip_mock.h (CPU, tests only) can stand in for them
#define ICER_LAUNCH(kernel, grid, block, shmem, ...) kernel<<<(grid), (block), (shmem)>>>(__VA_ARGS__)
#define ICER_LAUNCH_WAVE(kernel, grid, shmem, ...) kernel<<<(grid), 64, (shmem)>>>(__VA_ARGS__)
// (a workgroup of one wavefront per bit plane; the CPU mock runs the waves of a workgroup in turns inside one call)
#define ICER_LAUNCH_PLANES(kernel, grid, shmem, ...) kernel<<<(grid), 64 * kPwWaves, (shmem)>>>(__VA_ARGS__)
#define ICER_LAUNCH_WAVE_ON(stream, kernel, grid, shmem, ...) kernel<<<(grid), 64, (shmem), (stream)>>>(__VA_ARGS__)
#define ICER_LAUNCH_ON(stream, kernel, grid, block, shmem, ...) kernel<<<(grid), (block), (shmem), (stream)>>>(__VA_ARGS__)
#define ICER_LAUNCH_PLANES_ON(stream, kernel, grid, shmem, ...) kernel<<<(grid), 64 * kPwWaves, (shmem), (stream)>>>(__VA_ARGS__)
#define ICER_DYNAMIC_LDS(T, name) extern __shared__ T name[]
// the decoder tables of a workgroup: a copy in LDS (every decision looks them up; from global memory each look-up is a
// chain of dependent loads)
#define ICER_LDS_TABLES(name, src)                                                                                   \
    __shared__ DecoderTables name;                                                                                   \
    for (uint32_t k_ = threadIdx.x; k_ < sizeof(DecoderTables) / 4u; k_ += blockDim.x)                               \
        reinterpret_cast<uint32_t *>(&name)[k_] = reinterpret_cast<const uint32_t *>(src)[k_];                       \
    __syncthreads()
#endif

#include <algorithm>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/icer_hip_dec.h"
#if !defined(ICER_HOST_MOCK) || defined(ICER_MOCK_ASYNC)
#define ICER_DECODE_ASYNC 1            // icerx_decode_device_async (decoder_async.hpp; the CPU mock needs tests/emu/hip_mock_async.h)
#endif
#include "decoder_wave.hpp"
#include "decoder_planes.hpp"
#include "decoder_core.hpp"
#include "decoder_plan.hpp"
#include "decoder_route.hpp"

using namespace icer;

namespace {

thread_local std::string g_error;

int fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    fprintf(stderr, "libicer_hip_dec: %s\n", buf);
    return ICER_FATAL_ERROR;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        const hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) { rc = fail("%s: %s", #expr, hipGetErrorString(e_)); goto done; } \
    } while (0)

// ------------------------------------------------------------------------------------------ kernels
// what the kernels need to know about one stream / image of the batch
struct FrameInfo {
    uint32_t stream_off, stream_len;     // its bytes in the batch buffer
    uint32_t w, h, ll_w, ll_h;           // image and deepest-LL size
    uint16_t mean[4];
    uint32_t transform;                  // the run reaches sign-magnitude removal / mean / inverse DWT / clamping
};

__global__ void __launch_bounds__(256)
count_headers_kernel(const uint8_t *__restrict__ data, const FrameInfo *__restrict__ frames,
                     const uint32_t *__restrict__ crc_tab, PacketCandidate *__restrict__ out, uint32_t cap,
                     uint32_t *__restrict__ count)
{
    const FrameInfo f = frames[blockIdx.y];
    const uint32_t off = blockIdx.x * blockDim.x + threadIdx.x;
    if (off >= f.stream_len) return;
    PacketCandidate c;
    if (!header_candidate(crc_tab, data + f.stream_off, f.stream_len, off, &c)) return;
    c.frame = blockIdx.y;
    const uint32_t at = atomicAdd(count, 1u);
    if (at < cap) out[at] = c;
}

// payload CRCs: 64 threads per candidate, each a contiguous piece (payload_piece_crc), XOR-combined in the candidate's
// crc_acc; the host compares it with the header's field.  grid = candidates, block = 64.
__global__ void __launch_bounds__(64)
check_payloads_kernel(const uint8_t *__restrict__ data, const FrameInfo *__restrict__ frames,
                      const uint32_t *__restrict__ crc_tab, PacketCandidate *__restrict__ cands, uint32_t n)
{
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const uint32_t v = payload_piece_crc(crc_tab, data + frames[cands[i].frame].stream_off, cands[i], threadIdx.x, 64u);
    if (v) atomicXor(&cands[i].crc_acc, v);
}

// plane of channel `chan` of frame `frame`: planes + (frame * channels + chan) * frame_stride, rows of the frame's width
__global__ void __launch_bounds__(64)
decode_chains_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels,
                     const ChainDesc *__restrict__ chains, uint32_t n, const uint8_t *__restrict__ data,
                     const FrameInfo *__restrict__ frames, const DecoderTables *__restrict__ tables, int nplanes, int sign_bit)
{
    ICER_DYNAMIC_LDS(uint8_t, state);                     // plane_block_bytes(64): the threads' per-bin arrays
    ICER_LDS_TABLES(lt, tables);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ChainDesc c = chains[i];
    const FrameInfo f = frames[c.frame];
    PlaneDecoder job;
    plane_attach_columns(job, state, 64u, threadIdx.x);
    decode_chain(job, chain_plane(planes, c, channels, frame_stride), f.w, c, (int)c.subband, data + f.stream_off,
                 f.stream_len, lt, nplanes, sign_bit);
}

// the same with one wavefront per chain and one lane per packet (decoder_wave.hpp); dynamic LDS = the row ring
__global__ void __launch_bounds__(64)
decode_chains_wave_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels,
                          const ChainDesc *__restrict__ chains, const uint8_t *__restrict__ data,
                          const FrameInfo *__restrict__ frames, const DecoderTables *__restrict__ tables, int nplanes,
                          int sign_bit)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                       // the lanes' per-bin arrays, then the chain's row ring
    ICER_LDS_TABLES(lt, tables);
    const ChainDesc c = chains[blockIdx.x];
    const FrameInfo f = frames[c.frame];
    uint16_t *ring = reinterpret_cast<uint16_t *>(lds + kStateBytes);
    decode_chain_wave(ring, chain_plane(planes, c, channels, frame_stride), f.w, c, (int)c.subband,
                      data + f.stream_off, f.stream_len, lt, nplanes, sign_bit, nullptr, lds);
}

// A workgroup of a planes kernel takes up chain `c`: control words, zero row and ring start out zero; and every wave's number,
// as a scalar.  (The CPU mock runs a chain's waves in turns inside one call, which clears the block itself.)  Two helpers, not
// one: planes_list_kernel takes the wave number once, in front of its loop over chains, and moving it into the loop changes
// that kernel's code.
ICER_DEV void pw_workgroup_clear(uint8_t *lds, const ChainDesc &c, int nplanes)
{
#ifndef ICER_HOST_MOCK
    uint32_t *w = reinterpret_cast<uint32_t *>(lds);
    const uint32_t words = (uint32_t)((pw_lds_bytes(c.w, nplanes) + 3u) / 4u);
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) w[i] = 0;
    __syncthreads();
#else
    (void)lds; (void)c; (void)nplanes;
#endif
}
ICER_DEV uint32_t pw_workgroup_wave()
{
#ifndef ICER_HOST_MOCK
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#else
    return 0;
#endif
}

// one wavefront per bit plane, wave-uniform decisions (decoder_planes.hpp): grid = chains that take the fast entropy path,
// block = 64 * kPwWaves, dynamic LDS = the widest chain's control words + row ring
__global__ void __launch_bounds__(64 * kPwWaves)
decode_chains_planes_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels,
                            const ChainDesc *__restrict__ chains, const uint8_t *__restrict__ data,
                            const FrameInfo *__restrict__ frames, const DecoderTables *__restrict__ tables, int nplanes,
                            int sign_bit, uint32_t *__restrict__ err)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);
    const ChainDesc &c = chains[blockIdx.x];                  // (read in place: see pw_run_chain)
    const FrameInfo f = frames[c.frame];
    pw_workgroup_clear(lds, c, nplanes);
    const uint32_t wave = pw_workgroup_wave();
    (void)pw_run_chain(lds, wave, c, nplanes, sign_bit, chain_plane(planes, c, channels, frame_stride), f.w,
                       data + f.stream_off, f.stream_len, tables, err);
}

// One level of the inverse transform for filters without a recurrence along the line (beta = 0 and alpha_-1 = 0: filter A --
// every restored high then depends on the stored lows and highs alone, idwt_line's `dn` and filter-C terms drop out): one
// thread per output PAIR instead of one per line.  `rows` = false: lines are columns (x = line, y = pair), true: lines are
// rows.  grid = (ceil(cw / 64), ceil(pairs-or-lines / 4), frames * channels), block = (64, 4).
__global__ void __launch_bounds__(256)
idwt_pairs_kernel(const int16_t *__restrict__ src, int16_t *__restrict__ dst, size_t frame_stride, int channels,
                  const uint32_t *__restrict__ list, uint32_t image_w, uint32_t cw, uint32_t ch_rows, FilterTaps f,
                  int bits, const uint32_t *__restrict__ pos_of, bool rows)
{
    const uint32_t gx = blockIdx.x * 64u + (threadIdx.x & 63u), gy = blockIdx.y * 4u + (threadIdx.x >> 6);
    const size_t base = ((size_t)list[blockIdx.z / (unsigned)channels] * channels + blockIdx.z % (unsigned)channels) * frame_stride;
    // (x runs along a row of the image in both passes, so that a wavefront's accesses are contiguous)
    const uint32_t n = rows ? cw : ch_rows, nl = (n + 1u) / 2u, nh = n / 2u;
    const uint32_t line = rows ? gy : gx, k = rows ? gx : gy;
    if (line >= (rows ? ch_rows : cw) || k >= nl) return;
    const size_t stride = rows ? 1 : image_w;
    const int16_t *s = src + base + (rows ? (size_t)line * image_w : (size_t)line);
    int16_t *d = dst + base + (rows ? (size_t)line * image_w : (size_t)line);
    const bool odd = (n & 1u) != 0;
#define LO(i) ((int32_t)s[(size_t)(i) * stride])
#define HI(i) ((int32_t)s[(size_t)(nl + (i)) * stride])
#define RR(i) ((int32_t)(int16_t)(LO((i) - 1) - LO(i)))
#define TR(v) (bits == 8 ? (int16_t)(int8_t)(v) : (int16_t)(v))
    if (k >= nh) { d[(size_t)pos_of[nl - 1u] * stride] = (int16_t)LO(nl - 1u); return; }       // (odd length: the last low)
    int32_t add;
    if (k == 0) add = dec_floordiv(RR(1), 4);
    else if (!odd && k == nh - 1u) add = dec_floordiv(RR(nh - 1u), 4);
    else add = dec_floordiv(f.a0 * RR(k) + f.a1 * RR(k + 1u) + 8, 16);
    const int32_t hi = TR(HI(k) + add);
    const int32_t a = LO(k) + dec_floordiv(hi + 1, 2);
    d[(size_t)pos_of[k] * stride] = TR(a);
    d[(size_t)pos_of[nl + k] * stride] = TR(a - hi);
#undef LO
#undef HI
#undef RR
#undef TR
}

// sign-magnitude words -> int16, LL mean back in (grid.y = frame * channels + channel)
__global__ void __launch_bounds__(256)
unsign_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels, const FrameInfo *__restrict__ frames,
              int sign_bit, int bits)
{
    const FrameInfo f = frames[blockIdx.y / (unsigned)channels];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!f.transform || i >= (size_t)f.w * f.h) return;
    uint16_t *p = planes + (size_t)blockIdx.y * frame_stride;
    int16_t s = from_sign_magnitude(p[i], sign_bit);
    const uint32_t x = (uint32_t)(i % f.w), y = (uint32_t)(i / f.w);
    if (x < f.ll_w && y < f.ll_h) s = add_ll_mean(s, f.mean[blockIdx.y % (unsigned)channels], bits);
    p[i] = (uint16_t)s;
}

// one thread per column (rows = false) or per row (rows = true) of a level's region; grid.y walks the channels of the
// frames in `list` (all of the same size)
__global__ void __launch_bounds__(64)
idwt_lines_kernel(const int16_t *__restrict__ src, int16_t *__restrict__ dst, size_t frame_stride, int channels,
                  const uint32_t *__restrict__ list, uint32_t image_w, uint32_t cw, uint32_t ch_rows, FilterTaps taps,
                  int bits, const uint32_t *__restrict__ pos_of, bool rows)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t base = ((size_t)list[blockIdx.y / (unsigned)channels] * channels + blockIdx.y % (unsigned)channels) * frame_stride;
    if (rows) {
        if (i < ch_rows) idwt_line(src + base + (size_t)i * image_w, dst + base + (size_t)i * image_w, cw, 1, taps, bits, pos_of);
    } else {
        if (i < cw) idwt_line(src + base + i, dst + base + i, ch_rows, image_w, taps, bits, pos_of);
    }
}

// icer_remove_negative_* (icer_util.c:70-91) for the frames that were transformed; `out8` != null: narrow to bytes
// (every frame: a frame that stopped early keeps its sign-magnitude words, narrowed like the reference's uint8 planes)
__global__ void __launch_bounds__(256)
finish_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels, const FrameInfo *__restrict__ frames,
              uint8_t *__restrict__ out8)
{
    const FrameInfo f = frames[blockIdx.y / (unsigned)channels];
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)f.w * f.h) return;
    const size_t at = (size_t)blockIdx.y * frame_stride + i;
    int16_t s = (int16_t)planes[at];
    if (f.transform && s < 0) s = 0;
    planes[at] = (uint16_t)s;
    if (out8) out8[at] = (uint8_t)s;
}

}  // namespace

#include "decoder_display.hpp"         // display_finish_kernel: the last pass of the *_display calls, in finish_kernel's place
#include "decoder_recon.hpp"           // reconstruct_kernel: truncated coefficients part-way into their interval, before unsign_kernel

// ------------------------------------------------------------------------------------------ decoder object
// The side streams carry the kernels of the ring size classes side by side with the plane kernel on the call's own stream.  The HIP runtime
// shares GPU_MAX_HW_QUEUES (4 by default) hardware queues PER PRIORITY LEVEL out over the live streams of the process, and streams on one
// queue take turns: unless the process has asked for 6 queues or more, the side streams are created at the low priority level -- a pool of
// their own, whatever else the process has alive (the encoder library does the same, api.hip want_priority_streams).  In a quiet process
// the A/B shows no difference (64 streams per call 886-915 Mpix/s with plain or low-level side streams at 8 / 4 / default queues,
// profiles/r05_logs/r05_u.log; one earlier run with plain streams on 4 queues had given 782): it is there for the crowded process.
// ICER_HIP_STREAM_PRIO=0|1 pins the choice.
#ifndef ICER_HOST_MOCK
static hipError_t create_side_stream(hipStream_t *st)
{
    bool level = true;
    if (const char *pv = getenv("ICER_HIP_STREAM_PRIO")) level = atoi(pv) != 0;
    else if (const char *q = getenv("GPU_MAX_HW_QUEUES")) level = atoi(q) < 6;
    int least = 0, greatest = 0;
    if (level && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest < least &&
        hipStreamCreateWithPriority(st, hipStreamNonBlocking, least) == hipSuccess)
        return hipSuccess;
    (void)hipGetLastError();
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}
#endif

struct icerx_decoder {
    int device = 0, channels = 1, stages = 1, filt = 0, bits = 16;
    // a reduced-resolution decoder (icerx_decoder_create_reduced): made for streams of stages + reduce stages, it decodes their
    // derived streams (plan_decode) -- `stages` is what is left to run, and everything below the planners goes by it alone
    int reduce = 0;
    // icerx_decoder_set_reconstruction: eighths of the interval a truncated non-zero coefficient is rebuilt at (0: its low end,
    // the reference's decode); read once when a call is enqueued
    int recon = 0;
    unsigned segments = 1;
    DecoderTables tables;
    uint32_t crc_tab[256];
    // device buffers, grown on demand and kept
    struct Buf { void *p = nullptr; size_t cap = 0; };
    Buf data, frames, crc, dtables, count, cands, chains, work, tmp, out8, pos, list, err, disp;
    Buf win, wout;                     // a window decode (decoder_window.hpp): the frames' geometry, the windows of a host call
    int n_cus = 256;                   // compute units of the device
    bool planes_lds_raised = false;    // decode_chains_planes_kernel has been granted more than 64 KiB of dynamic LDS
    int is_gfx950 = -1;                // (-1: not asked yet)
    size_t planes_lds_fallback = 0;    // ... or, refused the hardware's figure, this much (what the runtime reports)
    bool planes_lds_refused = false;   // ... or the runtime refused: chains that need more than 48 KiB go to the lane-per-plane kernel from then on
    // the lane-per-plane kernel is launched once per size class of row ring, side by side (batch_chains; decoder_route.hpp)
    hipStream_t side[kRingClasses] = {};
    bool side_ok = false;
    // icerx_decode_device_async: the events that fork its side-stream work from the caller's stream and join it back, and
    // whether its planes kernel has been granted the LDS that resolve_planes_lds found
#ifdef ICER_DECODE_ASYNC
    hipEvent_t fork = nullptr, join[kRingClasses] = {};
    bool events_ok = false;
#endif
    int async_lds_state = 0;           // 0: not asked yet, 1: granted, -1: refused (the async planes kernel keeps 48 KiB)
};

namespace {

hipError_t ensure(icerx_decoder::Buf &b, size_t bytes)
{
    if (bytes <= b.cap) return hipSuccess;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) b.cap = bytes;
    return e;
}

// The dynamic LDS the wave-per-plane kernel may take on this decoder's device (asked once per decoder; granted to
// decode_chains_planes_kernel on the way)
size_t resolve_planes_lds(icerx_decoder *d)
{
#ifdef ICER_HOST_MOCK
    (void)d;
    return (size_t)1 << 20;
#else
    // what a workgroup of this device may take (gfx950: 160 KiB), less 10 KiB for the kernel's static block and the runtime
    size_t planes_lds_limit = 0;
    int max_lds = 0, dev_id = d->device;
    if (dev_id < 0 && hipGetDevice(&dev_id) != hipSuccess) { (void)hipGetLastError(); dev_id = 0; }      // (-1: the caller's current device)
    if (hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev_id) != hipSuccess) { (void)hipGetLastError(); max_lds = 64 * 1024; }
    // (this runtime reports 64 KiB for gfx950, whose compute units have 160 KiB and grant a workgroup what hipFuncSetAttribute asks for --
    // the encoder's window coder runs on 115 KiB --: ask for the hardware's figure first, the reported one is the fall-back)
    if (d->is_gfx950 < 0) {
        hipDeviceProp_t prop;
        d->is_gfx950 = (hipGetDeviceProperties(&prop, dev_id) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0) ? 1 : 0;
        (void)hipGetLastError();
    }
    const bool gfx950 = d->is_gfx950 == 1;
    if (gfx950 && max_lds < 160 * 1024 && !d->planes_lds_refused) max_lds = 160 * 1024;
    planes_lds_limit = max_lds > 10 * 1024 ? (size_t)max_lds - 10u * 1024u : 0u;
    // more than 48 KiB of dynamic LDS has to be granted; a runtime / device that refuses loses nothing but the fast kernel
    // for the chains that need it (they go to decode_chains_wave_kernel below)
    if (planes_lds_limit > 48u * 1024u && !d->planes_lds_raised && !d->planes_lds_refused) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(decode_chains_planes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)planes_lds_limit) == hipSuccess)
            d->planes_lds_raised = true;
        else {
            (void)hipGetLastError(); d->planes_lds_refused = true;
            int rep = 0;
            if (hipDeviceGetAttribute(&rep, hipDeviceAttributeMaxSharedMemoryPerBlock, dev_id) != hipSuccess) { (void)hipGetLastError(); rep = 64 * 1024; }
            planes_lds_limit = rep > 10 * 1024 ? (size_t)rep - 10u * 1024u : 0u;
            if (planes_lds_limit > 48u * 1024u && hipFuncSetAttribute(reinterpret_cast<const void *>(decode_chains_planes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)planes_lds_limit) == hipSuccess)
                d->planes_lds_fallback = planes_lds_limit;
            else (void)hipGetLastError();
        }
        // (said once per decoder: on a runtime that reports or grants less than gfx950's 160 KiB the fast planes kernel quietly loses
        // the chains that need more -- correct, slower)
        if (d->planes_lds_refused || planes_lds_limit < 150u * 1024u)
            fprintf(stderr, "libicer_hip_dec: %zu KiB of LDS per workgroup for the planes kernel (%s); chains that need more take the wave kernel\n",
                    (d->planes_lds_refused ? (d->planes_lds_fallback ? d->planes_lds_fallback : (size_t)48u * 1024u) : planes_lds_limit) / 1024u,
                    d->planes_lds_refused ? "the runtime refused the hardware's 150 KiB" : "what the device reports, less 10 KiB");
    }
    if (d->planes_lds_refused) planes_lds_limit = d->planes_lds_fallback ? d->planes_lds_fallback : std::min(planes_lds_limit, (size_t)48u * 1024u);
    return planes_lds_limit;
#endif
}

// Grants `kernel` up to `limit` bytes of dynamic LDS (resolve_planes_lds' figure, for the other kernels that take it) and remembers the
// answer in *state -- 0: not asked yet, 1: granted, -1: refused, it keeps the 48 KiB a launch gets without asking.  -> the limit that holds
size_t grant_dynamic_lds(const void *kernel, size_t limit, int *state)
{
#ifndef ICER_HOST_MOCK
    if (limit > 48u * 1024u && *state == 0) {
        *state = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit) == hipSuccess ? 1 : -1;
        if (*state < 0) (void)hipGetLastError();
    }
    if (*state < 0) limit = std::min(limit, (size_t)48u * 1024u);
#endif
    (void)kernel; (void)state;
    return limit;
}

// the side streams of a decoder, made by the first call that needs them (none is kept half-made: the next call tries again)
int ensure_side_streams(icerx_decoder *d)
{
#ifndef ICER_HOST_MOCK
    if (d->side_ok) return ICER_RESULT_OK;
    bool made = true;
    for (hipStream_t &st : d->side) made = made && create_side_stream(&st) == hipSuccess;
    if (!made) {
        for (hipStream_t &st : d->side) { if (st) (void)hipStreamDestroy(st); st = nullptr; }
        (void)hipGetLastError();
        return fail("the decoder could not create its side streams");
    }
    d->side_ok = true;
#endif
    (void)d;
    return ICER_RESULT_OK;
}

// ------------------------------------------------------------------------------------------ synchronous batch decode
// Where decode_batch leaves its results, `p` by kind.  kHostPlanes: void *const *, frame k's channel c goes to p[k * channels + c]
// (host pointers, >= frame_stride samples each); kDevPlanes: device memory, to p + (k * channels + c) * frame_stride samples
// (uint16 or uint8 samples by sample_bits).  Display calls, frame k's 8-bit image (decoder_display.hpp) -- kHostDisplay:
// uint8_t *const *, to p[k] (host pointers, channels * frame_stride bytes each); kDevDisplay: device memory, to
// p + k * channels * frame_stride bytes.
struct BatchOut {
    enum Kind { kHostPlanes, kDevPlanes, kHostDisplay, kDevDisplay } kind;
    const void *p;
    bool display() const { return kind == kHostDisplay || kind == kDevDisplay; }
    bool to_host() const { return kind == kHostPlanes || kind == kHostDisplay; }
};

// one call of decode_batch: what its stages (batch_packets .. batch_results, in this order) hand to one another
struct BatchRun {
    icerx_decoder *d;
    int n;
    size_t frame_stride;
    size_t total_len, max_len;           // the end of the last stream in the batch buffer; the longest stream
    PlaneBits pb;
    std::vector<FrameInfo> frames;
    std::vector<PacketCandidate> cands;  // from batch_packets on: the header candidates, in stream and offset order
    std::vector<DecodePlan> plans;
    std::vector<ChainDesc> chains;       // from batch_chains on: in launch order (route_batch_chains), as uploaded to d->chains
    const uint8_t *d_data;
    FrameInfo *d_frames;
    uint16_t *d_planes;
    // a window decode (decoder_window.hpp): n x 4 x, y, w, h, and the samples a window may have; frame_stride is then the working planes'
    const uint32_t *windows = nullptr;
    size_t out_stride = 0;
    size_t planes_total() const { return (size_t)n * d->channels * frame_stride; }
    dim3 grid_all() const { return dim3((unsigned)((frame_stride + 255u) / 256u), (unsigned)(n * d->channels)); }
};

// Opens a call of any synchronous driver, behind the checks that are the driver's own: the streams' bytes and the 32-bit limits of
// the batch buffer (`too_long`: the driver's sentence, with a %zu) and of the strides (out_stride: 0 but for a window decode)
int batch_open(BatchRun &run, icerx_decoder *d, int n, const uint8_t *data, const size_t *offsets, const size_t *lens, size_t frame_stride,
               size_t out_stride, const char *too_long)
{
    size_t total_len = 0, max_len = 0;
    std::vector<FrameInfo> frames((size_t)n);                // (all zero)
    for (int k = 0; k < n; k++) {
        if (lens[k] && !data) return ICER_INVALID_INPUT;
        total_len = std::max(total_len, offsets[k] + lens[k]);
        max_len = std::max(max_len, lens[k]);
        frames[k].stream_off = (uint32_t)offsets[k];         // (they fit: the test below)
        frames[k].stream_len = (uint32_t)lens[k];
    }
    if (total_len >= 0xFFFFFFFFull - 64u) return fail(too_long, total_len);
    if (std::max(frame_stride, out_stride) > 0xFFFFFFFFull) return fail("frames of %zu samples: 32-bit indices only", std::max(frame_stride, out_stride));
    BatchRun r = {d, n, frame_stride, total_len, max_len, plane_bits(d->bits), std::move(frames), {}, std::vector<DecodePlan>((size_t)n), {},
                  nullptr, nullptr, nullptr, nullptr, out_stride};
    run = std::move(r);
    return ICER_RESULT_OK;
}

// 1. packets: the streams on the device, their header candidates with checked payloads, in stream and offset order
int batch_packets(BatchRun &r, const uint8_t *data, bool data_on_device)
{
    icerx_decoder *d = r.d;
    std::vector<PacketCandidate> &cands = r.cands;
    int rc = ICER_RESULT_OK;
    HIP_TRY(ensure(d->frames, sizeof(FrameInfo) * r.n));
    r.d_frames = (FrameInfo *)d->frames.p;
    HIP_TRY(hipMemcpy(r.d_frames, r.frames.data(), sizeof(FrameInfo) * r.n, hipMemcpyHostToDevice));
    if (r.total_len) {
        if (data_on_device) r.d_data = data;
        else {
            HIP_TRY(ensure(d->data, r.total_len));
            HIP_TRY(hipMemcpy(d->data.p, data, r.total_len, hipMemcpyHostToDevice));
            r.d_data = (const uint8_t *)d->data.p;
        }
        HIP_TRY(ensure(d->count, sizeof(uint32_t)));
        uint32_t cap = (uint32_t)(r.total_len / 64u) + 1024u, count = 0;
        for (int attempt = 0; attempt < 2 && r.max_len; attempt++) {
            HIP_TRY(ensure(d->cands, sizeof(PacketCandidate) * cap));
            HIP_TRY(hipMemset(d->count.p, 0, sizeof(uint32_t)));
            ICER_LAUNCH(count_headers_kernel, dim3((unsigned)((r.max_len + 255u) / 256u), (unsigned)r.n), 256, 0, r.d_data, r.d_frames,
                        (const uint32_t *)d->crc.p, (PacketCandidate *)d->cands.p, cap, (uint32_t *)d->count.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(&count, d->count.p, sizeof count, hipMemcpyDeviceToHost));
            if (count <= cap) break;
            cap = count;                                    // (more header look-alikes than expected: once more, all of them)
        }
        if (count) {
            ICER_LAUNCH(check_payloads_kernel, count, 64, 0, r.d_data, r.d_frames, (const uint32_t *)d->crc.p, (PacketCandidate *)d->cands.p, count);
            HIP_TRY(hipGetLastError());
            cands.resize(count);
            HIP_TRY(hipMemcpy(cands.data(), d->cands.p, sizeof(PacketCandidate) * count, hipMemcpyDeviceToHost));
            for (PacketCandidate &c : cands) c.payload_ok = (c.fits && c.crc_acc == load_le32(c.hdr + 20)) ? 1u : 0u;   // (icer_compress.c:576-577)
            std::sort(cands.begin(), cands.end(), [](const PacketCandidate &a, const PacketCandidate &b) {
                return a.frame != b.frame ? a.frame < b.frame : a.off < b.off;
            });
        }
    }
done:
    return rc;
}

// what the kernels are told about a frame with this plan (stream_off / stream_len stay); -> it delivers samples (plan_delivers)
bool frame_of_plan(FrameInfo &f, const DecodePlan &pl, int stages)
{
    const bool runs = plan_delivers(pl);
    f.w = runs ? (uint32_t)pl.w : 0u;
    f.h = runs ? (uint32_t)pl.h : 0u;
    f.ll_w = (uint32_t)dim_low(pl.w, stages); f.ll_h = (uint32_t)dim_low(pl.h, stages);
    for (int c = 0; c < 3; c++) f.mean[c] = pl.mean[c];
    f.transform = (runs && pl.transform) ? 1u : 0u;
    return runs;
}

// where the working planes of a call live: the caller's buffer when that is device memory of uint16 samples, else d->work
hipError_t batch_working_planes(BatchRun &r, const BatchOut &out)
{
    const bool callers = out.kind == BatchOut::kDevPlanes && r.d->bits == 16;
    const hipError_t e = callers ? hipSuccess : ensure(r.d->work, sizeof(uint16_t) * r.planes_total());
    r.d_planes = (uint16_t *)(callers ? const_cast<void *>(out.p) : r.d->work.p);
    return e;
}

// the error word of a wave-per-plane launch: cleared in front of it, read once the kernels are complete (`whose`: "the decoder", ...)
hipError_t planes_err_begin(icerx_decoder *d)
{
    const hipError_t e = ensure(d->err, sizeof(uint32_t));
    return e != hipSuccess ? e : hipMemset(d->err.p, 0, sizeof(uint32_t));
}
int planes_err_end(icerx_decoder *d, const char *whose)
{
    int rc = ICER_RESULT_OK;
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, d->err.p, sizeof err, hipMemcpyDeviceToHost));
    if (err) rc = fail("a bit-plane wave of %s waited longer than its spin bound (internal error)", whose);
done:
    return rc;
}

// the way out of a call after an error: nothing of it runs on afterwards (launches of the size classes may be left on the side
// streams), and the error it met is not found again by the next call
void drain_after_error(icerx_decoder *d)
{
#ifndef ICER_HOST_MOCK
    if (d->side_ok) for (hipStream_t st : d->side) (void)hipStreamSynchronize(st);
#endif
    (void)hipDeviceSynchronize(); (void)hipGetLastError();
}

// the copy back of a host call, from rows of channels * frame_stride units of `unit` bytes at `from`: of frame k its samples(k)
// samples -- a display call's to the one image pointer of the frame, else each channel's to its plane pointer
template <class Samples>
int rows_to_host(const BatchOut &out, int n, int channels, const void *from, size_t frame_stride, size_t unit, Samples samples)
{
    void *const *to = (void *const *)out.p;
    int rc = ICER_RESULT_OK;
    for (int k = 0; k < n; k++) {
        const size_t count = samples(k);
        const uint8_t *row = (const uint8_t *)from + (size_t)k * channels * frame_stride * unit;
        if (!count) continue;
        if (out.display()) HIP_TRY(hipMemcpy(to[k], row, channels * count, hipMemcpyDeviceToHost));
        else
            for (int c = 0; c < channels; c++)
                HIP_TRY(hipMemcpy(to[k * channels + c], row + (size_t)c * frame_stride * unit, count * unit, hipMemcpyDeviceToHost));
    }
done:
    return rc;
}

// 2. plans: per stream the packet walk (plan_decode) -- its results, its FrameInfo (uploaded again) and its chains
int batch_plans(BatchRun &r, int *rcs, size_t *ws, size_t *hs)
{
    const icerx_decoder *d = r.d;
    const std::vector<PacketCandidate> &cands = r.cands;
    int rc = ICER_RESULT_OK;
    size_t at = 0;
    std::vector<PacketCandidate> mine;
    for (int k = 0; k < r.n; k++) {
        mine.clear();
        while (at < cands.size() && cands[at].frame == (uint32_t)k) mine.push_back(cands[at++]);
        DecodePlan &pl = r.plans[k];
        FrameInfo &f = r.frames[k];
        if (r.windows) {
            const FilterTaps taps = filter_taps(d->filt);
            plan_decode_window(&pl, mine, d->channels, d->stages, d->segments, d->bits, ws[k], hs[k], r.frame_stride, d->reduce,
                               r.windows + 4 * (size_t)k, r.out_stride, taps.be == 0 && taps.am1 == 0);
        } else
            plan_decode(&pl, mine, d->channels, d->stages, d->segments, d->bits, ws[k], hs[k], r.frame_stride, d->reduce);
        ws[k] = pl.w; hs[k] = pl.h; rcs[k] = pl.rc;
        if (!frame_of_plan(f, pl, d->stages)) continue;
        for (ChainDesc c : pl.chains) { c.frame = (uint32_t)k; r.chains.push_back(c); }
    }
    HIP_TRY(hipMemcpy(r.d_frames, r.frames.data(), sizeof(FrameInfo) * r.n, hipMemcpyHostToDevice));
done:
    return rc;
}

// 3. bit planes: into the caller's device buffer when that holds uint16 samples, else into a work buffer; the chains routed
// (decoder_route.hpp), uploaded and decoded -- the wave-per-plane share on the null stream, the ring classes side by side with it
int batch_chains(BatchRun &r, const BatchOut &out)
{
    icerx_decoder *d = r.d;
    const int channels = d->channels, nplanes = r.pb.nplanes, sign_bit = r.pb.sign_bit;
    int rc = ICER_RESULT_OK;
    HIP_TRY(batch_working_planes(r, out));
    // (only the w * h samples of a frame are defined results; the rest of its slot is scratch)
    HIP_TRY(hipMemset(r.d_planes, 0, sizeof(uint16_t) * r.planes_total()));
    if (!r.chains.empty()) {
        const int mode = dec_wave_mode();
        uint32_t n_eligible = 0;
        for (const ChainDesc &c : r.chains) n_eligible += c.fast ? 1u : 0u;
        const bool want_planes = dwant_planes(mode, d->tables.lut_ok, n_eligible, (uint32_t)d->n_cus);
        const size_t planes_lds_limit = resolve_planes_lds(d);
        const BatchRoute route = route_batch_chains(r.chains, [&](uint32_t f) { return r.frames[f].stream_len; }, want_planes, planes_lds_limit, nplanes);
        const uint32_t nc = (uint32_t)r.chains.size(), n_fast = route.n_fast;
        const DecoderTables *tables = (const DecoderTables *)d->dtables.p;
        HIP_TRY(ensure(d->chains, sizeof(ChainDesc) * nc));
        HIP_TRY(hipMemcpy(d->chains.p, r.chains.data(), sizeof(ChainDesc) * nc, hipMemcpyHostToDevice));
        const ChainDesc *d_chains = (const ChainDesc *)d->chains.p;
        if (n_fast) {
            HIP_TRY(planes_err_begin(d));
            ICER_LAUNCH_PLANES(decode_chains_planes_kernel, n_fast, route.planes_lds, r.d_planes, r.frame_stride, channels, d_chains, r.d_data,
                               r.d_frames, tables, nplanes, sign_bit, (uint32_t *)d->err.p);
            HIP_TRY(hipGetLastError());
        }
        if (n_fast < nc) {
            // the planes of a segment side by side (one wavefront per chain) if the chain's row ring fits LDS
            if (mode != 0 && wave_ring_fits(route.rest_ring_elems)) {
                if ((rc = ensure_side_streams(d)) != ICER_RESULT_OK) goto done;
                // (everything the null stream did so far is complete: the upload of `chains` above was a blocking copy)
                uint32_t from = n_fast;
                for (int k = 0; k < kRingClasses; from = route.class_end[k++]) {
                    if (route.class_end[k] == from) continue;
                    ICER_LAUNCH_WAVE_ON(d->side[k], decode_chains_wave_kernel, route.class_end[k] - from, route.class_elems[k] * sizeof(uint16_t) + kStateBytes,
                                        r.d_planes, r.frame_stride, channels, d_chains + from, r.d_data, r.d_frames, tables, nplanes, sign_bit);
                    HIP_TRY(hipGetLastError());
                }
#ifndef ICER_HOST_MOCK
                for (hipStream_t st : d->side) HIP_TRY(hipStreamSynchronize(st));
#endif
            } else {
                ICER_LAUNCH(decode_chains_kernel, (nc - n_fast + 63u) / 64u, 64, plane_block_bytes(64u), r.d_planes, r.frame_stride, channels,
                            d_chains + n_fast, nc - n_fast, r.d_data, r.d_frames, tables, nplanes, sign_bit);
            }
            HIP_TRY(hipGetLastError());
        }
        if (n_fast) rc = planes_err_end(d, "the decoder");
    }
done:
    return rc;
}

// 4. samples: truncated coefficients rebuilt if the decoder asks for it (decoder_recon.hpp), sign-magnitude words -> int16 with
// the LL mean, then the inverse DWT, the frames of one size together
int batch_samples(BatchRun &r)
{
    icerx_decoder *d = r.d;
    const int n = r.n, channels = d->channels, bits = d->bits;
    const FilterTaps taps = filter_taps(d->filt);
    const bool pairwise = taps.be == 0 && taps.am1 == 0;      // (filter A: no recurrence along a line, idwt_pairs_kernel)
    std::vector<char> done((size_t)n, 0);
    int rc = ICER_RESULT_OK;
    if (d->recon != 0 && !r.chains.empty()) {                // (the chain kernels are complete: the side streams were waited for)
        ICER_LAUNCH(reconstruct_kernel, dim3((unsigned)r.chains.size(), kReconParts), kReconThreads, 0, r.d_planes, r.frame_stride, channels,
                    (const ChainDesc *)d->chains.p, (uint32_t)r.chains.size(), r.d_frames, (uint32_t)n, r.pb.nplanes, r.pb.sign_bit, d->recon);
        HIP_TRY(hipGetLastError());
    }
    ICER_LAUNCH(unsign_kernel, r.grid_all(), 256, 0, r.d_planes, r.frame_stride, channels, r.d_frames, r.pb.sign_bit, bits);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < n; k++) {
        if (done[k] || !r.frames[k].transform || r.plans[k].levels.empty()) continue;
        std::vector<uint32_t> list, pos, tab;
        for (int j = k; j < n; j++)
            if (!done[j] && r.frames[j].transform && r.frames[j].w == r.frames[k].w && r.frames[j].h == r.frames[k].h) { list.push_back((uint32_t)j); done[j] = 1; }
        std::vector<size_t> col_at, row_at;              // where each level's position tables start
        for (const DecodeLevel &lv : r.plans[k].levels) {
            col_at.push_back(tab.size());
            pos.resize(lv.ch); interleave_positions(lv.ch, bits, pos.data()); tab.insert(tab.end(), pos.begin(), pos.end());
            row_at.push_back(tab.size());
            pos.resize(lv.cw); interleave_positions(lv.cw, bits, pos.data()); tab.insert(tab.end(), pos.begin(), pos.end());
        }
        HIP_TRY(ensure(d->tmp, sizeof(uint16_t) * r.planes_total()));
        HIP_TRY(ensure(d->pos, sizeof(uint32_t) * tab.size()));
        HIP_TRY(hipMemcpy(d->pos.p, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice));
        HIP_TRY(ensure(d->list, sizeof(uint32_t) * list.size()));
        HIP_TRY(hipMemcpy(d->list.p, list.data(), sizeof(uint32_t) * list.size(), hipMemcpyHostToDevice));
        const unsigned gy = (unsigned)(list.size() * (size_t)channels);
        // one pass of a level -- columns: planes -> tmp, rows: tmp -> planes (only the level's region is touched) -- by pairs or by lines
        auto pass = [&](const DecodeLevel &lv, size_t tab_at, bool rows) {
            const int16_t *src = rows ? (const int16_t *)d->tmp.p : (const int16_t *)r.d_planes;
            int16_t *dst = rows ? (int16_t *)r.d_planes : (int16_t *)d->tmp.p;
            const uint32_t *pos_of = (const uint32_t *)d->pos.p + tab_at;
            if (pairwise)
                ICER_LAUNCH(idwt_pairs_kernel, rows ? dim3(((lv.cw + 1u) / 2u + 63u) / 64u, (lv.ch + 3u) / 4u, gy) : dim3((lv.cw + 63u) / 64u, ((lv.ch + 1u) / 2u + 3u) / 4u, gy),
                            dim3(256), 0, src, dst, r.frame_stride, channels, (const uint32_t *)d->list.p, r.frames[k].w, lv.cw, lv.ch, taps, bits, pos_of, rows);
            else
                ICER_LAUNCH(idwt_lines_kernel, dim3(((rows ? lv.ch : lv.cw) + 63u) / 64u, gy), 64, 0, src, dst, r.frame_stride, channels,
                            (const uint32_t *)d->list.p, r.frames[k].w, lv.cw, lv.ch, taps, bits, pos_of, rows);
        };
        for (size_t li = 0; li < r.plans[k].levels.size(); li++) {
            pass(r.plans[k].levels[li], col_at[li], false);
            HIP_TRY(hipGetLastError());
            pass(r.plans[k].levels[li], row_at[li], true);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipDeviceSynchronize());                 // (the position tables and the list are reused by the next size)
    }
done:
    return rc;
}

// 5. results: a display call is finished and converted in one pass (display_finish_kernel), planes are clamped and narrowed
// (finish_kernel); then the copy back of a host call
int batch_results(BatchRun &r, const BatchOut &out)
{
    icerx_decoder *d = r.d;
    const int n = r.n, channels = d->channels, bits = d->bits;
    const bool display = out.display(), to_host = out.to_host();
    uint8_t *d_bytes = to_host ? nullptr : (uint8_t *)out.p;  // the device's bytes: the display images, or the uint8 samples of 8-bit planes
    int rc = ICER_RESULT_OK;
    if (to_host && (display || bits == 8)) {                 // (a host call: they go through a buffer of the decoder's)
        icerx_decoder::Buf &buf = display ? d->disp : d->out8;
        HIP_TRY(ensure(buf, r.planes_total()));
        d_bytes = (uint8_t *)buf.p;
    }
    if (display)
        ICER_LAUNCH(display_finish_kernel, dim3((unsigned)(((r.frame_stride + 3u) / 4u + 255u) / 256u), (unsigned)n), 256, 0, r.d_planes,
                    r.frame_stride, channels, r.d_frames, bits, d_bytes);
    else
        ICER_LAUNCH(finish_kernel, r.grid_all(), 256, 0, r.d_planes, r.frame_stride, channels, r.d_frames, bits == 8 ? d_bytes : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (to_host)                                             // (16-bit planes come from the working planes themselves)
        rc = rows_to_host(out, n, channels, display || bits == 8 ? (const void *)d_bytes : (const void *)r.d_planes, r.frame_stride,
                          display ? 1u : (size_t)(bits / 8), [&](int k) { return (size_t)r.frames[k].w * r.frames[k].h; });
done:
    return rc;
}

// n streams: stream k = bytes [offsets[k], offsets[k] + lens[k]) of `data` (host memory, or device memory when
// data_on_device).  Results: rcs[k], ws[k] / hs[k] (in: the values kept when stream k holds no valid packet), and `out`.
int decode_batch(icerx_decoder *d, int n, const uint8_t *data, bool data_on_device, const size_t *offsets, const size_t *lens,
                 BatchOut out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs)
{
    g_error.clear();
    if (!d || n < 0 || (n && (!offsets || !lens || !rcs || !ws || !hs)) || (!out.p && n)) return ICER_INVALID_INPUT;
    if (n == 0) return ICER_RESULT_OK;
    BatchRun r;
    int rc = batch_open(r, d, n, data, offsets, lens, frame_stride, 0, "batch of %zu stream bytes: 32-bit offsets only");
    if (rc != ICER_RESULT_OK) return rc;
    rc = batch_packets(r, data, data_on_device);
    if (rc == ICER_RESULT_OK) rc = batch_plans(r, rcs, ws, hs);
    if (rc == ICER_RESULT_OK && r.planes_total()) {
        rc = batch_chains(r, out);
        if (rc == ICER_RESULT_OK) rc = batch_samples(r);
        if (rc == ICER_RESULT_OK) rc = batch_results(r, out);
    }
    if (rc != ICER_RESULT_OK) drain_after_error(d);
    return rc;
}

// A one-shot call: a decoder of its own (the caller's current device; reduced, rebuilding at `eighths`) for one frame at offset
// 0 -- run(d, &off, &frame_rc) is the driver's call -- and gone again; -> the call's code if it failed, else the frame's
template <class Run>
int one_shot(int channels, int stages, int filt, unsigned segments, int bits, int reduce, int eighths, Run run)
{
    icerx_decoder *d = nullptr;
    int rc = icerx_decoder_create_reduced(&d, -1, channels, stages, filt, segments, bits, reduce);
    if (rc != ICER_RESULT_OK) return rc;
    d->recon = eighths;
    const size_t off = 0;
    int frame_rc = ICER_RESULT_OK;
    rc = run(d, &off, &frame_rc);
    icerx_decoder_destroy(d);
    return rc != ICER_RESULT_OK ? rc : frame_rc;
}

int decompress_planes(void *const planes[], int channels, size_t *image_w, size_t *image_h, size_t bufsize,
                      const uint8_t *data, size_t data_length, int stages, int filt, unsigned segments, int bits, int reduce = 0,
                      int eighths = 0)
{
    if (!image_w || !image_h || (!data && data_length) || eighths < 0 || eighths > kReconMax) return ICER_INVALID_INPUT;
    for (int c = 0; c < channels; c++)
        if (!planes[c]) return ICER_INVALID_INPUT;
    return one_shot(channels, stages, filt, segments, bits, reduce, eighths, [&](icerx_decoder *d, const size_t *off, int *frame_rc) {
        return decode_batch(d, 1, data, false, off, &data_length, {BatchOut::kHostPlanes, planes}, bufsize, frame_rc, image_w, image_h);
    });
}

}  // namespace

#include "decoder_window.hpp"          // the window decode: decode_window_batch, and what decode_async enqueues for a window call
#include "decoder_session.hpp"         // progressive decode sessions: icerx_session_* (include/icer_hip_dec_session.h)
#ifdef ICER_DECODE_ASYNC
#include "decoder_async.hpp"
#include "recut.hpp"                   // icerx_recut_device_async: stored streams re-cut to smaller byte quotas
#include "recut_quality.hpp"           // icerx_recut_device_target_async / _budget_async: stored streams re-cut by their distortion sidecars
#include "combine.hpp"               // icerx_combine_device_async: the union and the difference of two stored streams of a frame
#endif

extern "C" {

const char *icerx_decoder_last_error(void) { return g_error.c_str(); }

int icerx_decoder_create(icerx_decoder **out, int device, int channels, int stages, int filt, unsigned segments, int sample_bits)
{
    return icerx_decoder_create_reduced(out, device, channels, stages, filt, segments, sample_bits, 0);
}

int icerx_decoder_reduce(const icerx_decoder *dec) { return dec ? dec->reduce : 0; }

int icerx_decoder_set_reconstruction(icerx_decoder *dec, int eighths)
{
    if (!dec || eighths < 0 || eighths > kReconMax) return ICER_INVALID_INPUT;
    dec->recon = eighths;
    return ICER_RESULT_OK;
}

int icerx_decoder_reconstruction(const icerx_decoder *dec) { return dec ? dec->recon : 0; }

void icerx_reduced_size(size_t w, size_t h, int reduce, size_t *rw, size_t *rh)
{
    const int r = reduce < 0 ? 0 : reduce > 63 ? 63 : reduce;
    if (rw) *rw = (w >> r) + ((w & (((size_t)1 << r) - 1u)) ? 1u : 0u);          // (ceil(w / 2^r) without the overflow of w + 2^r - 1)
    if (rh) *rh = (h >> r) + ((h & (((size_t)1 << r) - 1u)) ? 1u : 0u);
}

int icerx_decoder_create_reduced(icerx_decoder **out, int device, int channels, int stages, int filt, unsigned segments, int sample_bits,
                                 int reduce)
{
    g_error.clear();
    if (!out) return ICER_INVALID_INPUT;
    *out = nullptr;
    if ((channels != 1 && channels != 3) || filt < 0 || filt > 6 || (sample_bits != 8 && sample_bits != 16)) return ICER_INVALID_INPUT;
    if (stages < 1 || stages > kMaxStages) return ICER_TOO_MANY_STAGES;        // (reference: out-of-bounds table)
    if (reduce < 0 || reduce >= stages) return ICER_INVALID_INPUT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no usable HIP device");
#ifndef ICER_HOST_MOCK
    if (device >= 0) {
        if (device >= ndev) return fail("device %d of %d", device, ndev);
        if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice(%d) failed", device);
    }
#endif
    icerx_decoder *d = new icerx_decoder;
    d->device = device; d->channels = channels; d->stages = stages - reduce; d->reduce = reduce; d->filt = filt; d->bits = sample_bits; d->segments = segments;
#ifndef ICER_HOST_MOCK
    { int cur = 0; hipDeviceProp_t prop; if (hipGetDevice(&cur) == hipSuccess && hipGetDeviceProperties(&prop, cur) == hipSuccess && prop.multiProcessorCount > 0) d->n_cus = prop.multiProcessorCount; }
#endif
    CoderTables ct;
    build_coder_tables(&ct);
    build_decoder_tables(&d->tables, ct);
    build_crc32_table(d->crc_tab);
    int rc = ICER_RESULT_OK;
    HIP_TRY(ensure(d->crc, sizeof d->crc_tab));
    HIP_TRY(hipMemcpy(d->crc.p, d->crc_tab, sizeof d->crc_tab, hipMemcpyHostToDevice));
    HIP_TRY(ensure(d->dtables, sizeof d->tables));
    HIP_TRY(hipMemcpy(d->dtables.p, &d->tables, sizeof d->tables, hipMemcpyHostToDevice));
    *out = d;
    return ICER_RESULT_OK;
done:
    icerx_decoder_destroy(d);
    return rc;
}

void icerx_decoder_destroy(icerx_decoder *d)
{
    if (!d) return;
    for (icerx_decoder::Buf *b : {&d->data, &d->frames, &d->crc, &d->dtables, &d->count, &d->cands, &d->chains, &d->work, &d->tmp,
                                  &d->out8, &d->pos, &d->list, &d->err, &d->disp, &d->win, &d->wout})
        if (b->p) (void)hipFree(b->p);
#ifndef ICER_HOST_MOCK
    if (d->side_ok) for (hipStream_t st : d->side) (void)hipStreamDestroy(st);
#endif
#ifdef ICER_DECODE_ASYNC
    if (d->events_ok) {
        (void)hipEventDestroy(d->fork);
        for (hipEvent_t e : d->join) (void)hipEventDestroy(e);
    }
#endif
    delete d;
}

int icerx_decode_host(icerx_decoder *dec, int n, const uint8_t *data, const size_t *offsets, const size_t *lens,
                      void *const *planes_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs)
{
    if (!planes_out && n) return ICER_INVALID_INPUT;
    return decode_batch(dec, n, data, false, offsets, lens, {BatchOut::kHostPlanes, planes_out}, frame_stride, rcs, ws, hs);
}

int icerx_decode_device(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                        void *d_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs)
{
    if (!d_out && n) return ICER_INVALID_INPUT;
    return decode_batch(dec, n, (const uint8_t *)d_data, true, offsets, lens, {BatchOut::kDevPlanes, d_out}, frame_stride, rcs, ws, hs);
}

int icerx_decode_host_display(icerx_decoder *dec, int n, const uint8_t *data, const size_t *offsets, const size_t *lens,
                              uint8_t *const *images_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs)
{
    if (!images_out && n) return ICER_INVALID_INPUT;
    for (int k = 0; k < n; k++)
        if (!images_out[k]) return ICER_INVALID_INPUT;
    return decode_batch(dec, n, data, false, offsets, lens, {BatchOut::kHostDisplay, images_out}, frame_stride, rcs, ws, hs);
}

int icerx_decode_device_display(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                                uint8_t *d_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs)
{
    if (!d_out && n) return ICER_INVALID_INPUT;
    return decode_batch(dec, n, (const uint8_t *)d_data, true, offsets, lens, {BatchOut::kDevDisplay, d_out}, frame_stride, rcs, ws, hs);
}

int icerx_planes_to_display_device(const void *d_planes, int n_frames, int channels, size_t w, size_t h, size_t plane_stride,
                                   int sample_bits, uint8_t *d_out, size_t frame_stride, void *stream)
{
    g_error.clear();
    if (!d_planes || !d_out || n_frames < 0 || (channels != 1 && channels != 3) || (sample_bits != 16 && sample_bits != 8)) return ICER_INVALID_INPUT;
    if (w && h > (size_t)-1 / w) return ICER_INVALID_INPUT;
    const size_t pixels = w * h;
    if (pixels > plane_stride || pixels > frame_stride) return ICER_INVALID_INPUT;       // (a frame stays inside its planes and its row)
    if (n_frames == 0 || pixels == 0) return ICER_RESULT_OK;
    const int sample_bytes = sample_bits / 8;
    const size_t group = 8u / (size_t)sample_bytes, blocks = ((pixels + group - 1u) / group + 255u) / 256u;
    if (blocks > 0x7FFFFFFFull) return fail("frames of %zu pixels: too many for one launch", pixels);
    for (int first = 0; first < n_frames; first += (int)kDisplayFramesPerLaunch) {
        const unsigned count = (unsigned)std::min<int>(n_frames - first, (int)kDisplayFramesPerLaunch);
        ICER_LAUNCH_ON((hipStream_t)stream, display_planes_kernel, dim3((unsigned)blocks, count), 256, 0,
                       (const void *)((const uint8_t *)d_planes + (size_t)first * channels * plane_stride * sample_bytes), plane_stride,
                       channels, sample_bytes, pixels, d_out + (size_t)first * channels * frame_stride, frame_stride);
        if (hipGetLastError() != hipSuccess) return fail("display_planes_kernel could not be launched");
    }
    return ICER_RESULT_OK;
}

int icerx_decompress_display(uint8_t *image, size_t *image_w, size_t *image_h, size_t image_bufsize_pixels,
                             const uint8_t *datastream, size_t data_length, uint8_t stages, enum icer_filter_types filt,
                             uint8_t segments, int channels)
{
    if (!image || !image_w || !image_h || (!datastream && data_length) || (channels != 1 && channels != 3)) return ICER_INVALID_INPUT;
    uint8_t *const images[1] = {image};
    return one_shot(channels, stages, (int)filt, segments, 16, 0, 0, [&](icerx_decoder *d, const size_t *off, int *frame_rc) {
        return decode_batch(d, 1, datastream, false, off, &data_length, {BatchOut::kHostDisplay, images}, image_bufsize_pixels, frame_rc, image_w, image_h);
    });
}

#ifdef ICER_DECODE_ASYNC
size_t icerx_decode_display_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t frame_stride)
{
    if (!dec || n <= 0) return 0;
    return async_layout(dec, n, data_bytes, frame_stride, true).total;
}

int icerx_decode_device_display_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                      size_t stream_stride, const uint64_t *d_lens, uint8_t *d_out, size_t frame_stride,
                                      int32_t *d_rcs, uint64_t *d_ws, uint64_t *d_hs, void *d_workspace, size_t workspace_bytes,
                                      void *stream)
{
    if (!d_out && n > 0) return ICER_INVALID_INPUT;
    return decode_async(dec, n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, nullptr, frame_stride, d_rcs,
                        d_ws, d_hs, d_workspace, workspace_bytes, (hipStream_t)stream, d_out);
}

size_t icerx_decode_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t frame_stride)
{
    if (!dec || n <= 0) return 0;
    return async_layout(dec, n, data_bytes, frame_stride).total;
}

int icerx_decode_device_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                              size_t stream_stride, const uint64_t *d_lens, void *d_out, size_t frame_stride, int32_t *d_rcs,
                              uint64_t *d_ws, uint64_t *d_hs, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return decode_async(dec, n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, d_out, frame_stride, d_rcs,
                        d_ws, d_hs, d_workspace, workspace_bytes, (hipStream_t)stream);
}
#endif

// ---- window decode (include/icer_hip_dec_window.h)
int icerx_decode_host_window(icerx_decoder *dec, int n, const uint8_t *data, const size_t *offsets, const size_t *lens,
                             const uint32_t *windows, void *const *planes_out, size_t frame_stride, size_t full_stride, int *rcs,
                             size_t *ws, size_t *hs, uint32_t *info)
{
    return decode_window_batch(dec, n, data, false, offsets, lens, windows, {BatchOut::kHostPlanes, planes_out}, frame_stride, full_stride,
                               rcs, ws, hs, info);
}

int icerx_decode_device_window(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                               const uint32_t *windows, void *d_out, size_t frame_stride, size_t full_stride, int *rcs, size_t *ws,
                               size_t *hs, uint32_t *info)
{
    return decode_window_batch(dec, n, (const uint8_t *)d_data, true, offsets, lens, windows, {BatchOut::kDevPlanes, d_out}, frame_stride,
                               full_stride, rcs, ws, hs, info);
}

int icerx_decode_device_window_display(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                                       const uint32_t *windows, uint8_t *d_out, size_t frame_stride, size_t full_stride, int *rcs,
                                       size_t *ws, size_t *hs, uint32_t *info)
{
    return decode_window_batch(dec, n, (const uint8_t *)d_data, true, offsets, lens, windows, {BatchOut::kDevDisplay, d_out}, frame_stride,
                               full_stride, rcs, ws, hs, info);
}

int icerx_decompress_window(void *const planes[], int channels, size_t *image_w, size_t *image_h, size_t bufsize,
                            const uint8_t *datastream, size_t data_length, int stages, int filt, unsigned segments, int sample_bits,
                            int reduce, int eighths, const uint32_t *window, uint32_t *info)
{
    if (!planes || (channels != 1 && channels != 3) || !image_w || !image_h || !window || !info || (!datastream && data_length) ||
        eighths < 0 || eighths > kReconMax)
        return ICER_INVALID_INPUT;
    for (int c = 0; c < channels; c++)
        if (!planes[c]) return ICER_INVALID_INPUT;
    return one_shot(channels, stages, filt, segments, sample_bits, reduce, eighths, [&](icerx_decoder *d, const size_t *off, int *frame_rc) {
        // the working planes: the size of the image the stream's first valid packet announces, at the decoder's resolution
        size_t fw = 0, fh = 0, full = 0;
        if (datastream && icer_get_image_dimensions(datastream, data_length, &fw, &fh) == ICER_RESULT_OK) {
            icerx_reduced_size(fw, fh, reduce, &fw, &fh);
            full = fw * fh;
        }
        return decode_window_batch(d, 1, datastream, false, off, &data_length, window, {BatchOut::kHostPlanes, planes}, bufsize, full, frame_rc,
                                   image_w, image_h, info);
    });
}

#ifdef ICER_DECODE_ASYNC
size_t icerx_decode_window_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t full_stride)
{
    if (!dec || n <= 0) return 0;
    return async_layout(dec, n, data_bytes, full_stride, true).total + window_geom_bytes(n);
}

size_t icerx_decode_window_display_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t full_stride)
{
    return icerx_decode_window_workspace_bytes(dec, n, data_bytes, full_stride);
}

int icerx_decode_device_window_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                     size_t stream_stride, const uint64_t *d_lens, const uint32_t *d_windows, void *d_out,
                                     size_t frame_stride, size_t full_stride, int32_t *d_rcs, uint64_t *d_ws, uint64_t *d_hs,
                                     uint32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (n > 0 && (!d_out || !d_windows || !d_info)) return ICER_INVALID_INPUT;
    const WindowCall win = {d_windows, d_info, full_stride};
    return decode_async(dec, n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, d_out, frame_stride, d_rcs, d_ws,
                        d_hs, d_workspace, workspace_bytes, (hipStream_t)stream, nullptr, &win);
}

int icerx_decode_device_window_display_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                             size_t stream_stride, const uint64_t *d_lens, const uint32_t *d_windows, uint8_t *d_out,
                                             size_t frame_stride, size_t full_stride, int32_t *d_rcs, uint64_t *d_ws, uint64_t *d_hs,
                                             uint32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (n > 0 && (!d_out || !d_windows || !d_info)) return ICER_INVALID_INPUT;
    const WindowCall win = {d_windows, d_info, full_stride};
    return decode_async(dec, n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, nullptr, frame_stride, d_rcs, d_ws,
                        d_hs, d_workspace, workspace_bytes, (hipStream_t)stream, d_out, &win);
}
#endif

int icer_get_image_dimensions(const uint8_t *datastream, size_t data_length, size_t *image_w, size_t *image_h)
{
    if (!datastream || !image_w || !image_h) return ICER_INVALID_INPUT;
    if (data_length > 0xFFFFFFFFull) return ICER_INVALID_INPUT;
    uint32_t crc_tab[256];
    build_crc32_table(crc_tab);
    for (uint32_t off = 0; off < (uint32_t)data_length; off++) {
        PacketCandidate c;
        if (!header_candidate(crc_tab, datastream, (uint32_t)data_length, off, &c)) continue;
        check_payload(crc_tab, datastream, &c);
        if (!c.payload_ok) continue;
        *image_w = load_le32(datastream + off + 8);
        *image_h = load_le32(datastream + off + 12);
        return ICER_RESULT_OK;
    }
    return ICER_DECODER_OUT_OF_DATA;
}

int icerx_decompress_reduced(void *const planes[], int channels, size_t *image_w, size_t *image_h, size_t bufsize,
                             const uint8_t *datastream, size_t data_length, uint8_t stages, enum icer_filter_types filt,
                             uint8_t segments, int sample_bits, int reduce)
{
    if (!planes || (channels != 1 && channels != 3)) return ICER_INVALID_INPUT;
    return decompress_planes(planes, channels, image_w, image_h, bufsize, datastream, data_length, stages, (int)filt, segments,
                             sample_bits, reduce);
}

int icerx_decompress_reconstructed(void *const planes[], int channels, size_t *image_w, size_t *image_h, size_t bufsize,
                                   const uint8_t *datastream, size_t data_length, int stages, int filt, unsigned segments,
                                   int sample_bits, int reduce, int eighths)
{
    if (!planes || (channels != 1 && channels != 3)) return ICER_INVALID_INPUT;
    return decompress_planes(planes, channels, image_w, image_h, bufsize, datastream, data_length, stages, filt, segments,
                             sample_bits, reduce, eighths);
}

int icer_decompress_image_uint16(uint16_t *image, size_t *image_w, size_t *image_h, size_t image_bufsize,
                                 const uint8_t *datastream, size_t data_length, uint8_t stages,
                                 enum icer_filter_types filt, uint8_t segments)
{
    void *planes[1] = {image};
    return decompress_planes(planes, 1, image_w, image_h, image_bufsize, datastream, data_length, stages, (int)filt, segments, 16);
}

int icer_decompress_image_yuv_uint16(uint16_t *y_channel, uint16_t *u_channel, uint16_t *v_channel, size_t *image_w,
                                     size_t *image_h, size_t image_bufsize, const uint8_t *datastream,
                                     size_t data_length, uint8_t stages, enum icer_filter_types filt, uint8_t segments)
{
    void *planes[3] = {y_channel, u_channel, v_channel};
    return decompress_planes(planes, 3, image_w, image_h, image_bufsize, datastream, data_length, stages, (int)filt, segments, 16);
}

int icer_decompress_image_uint8(uint8_t *image, size_t *image_w, size_t *image_h, size_t image_bufsize,
                                const uint8_t *datastream, size_t data_length, uint8_t stages,
                                enum icer_filter_types filt, uint8_t segments)
{
    void *planes[1] = {image};
    return decompress_planes(planes, 1, image_w, image_h, image_bufsize, datastream, data_length, stages, (int)filt, segments, 8);
}

int icer_decompress_image_yuv_uint8(uint8_t *y_channel, uint8_t *u_channel, uint8_t *v_channel, size_t *image_w,
                                    size_t *image_h, size_t image_bufsize, const uint8_t *datastream,
                                    size_t data_length, uint8_t stages, enum icer_filter_types filt, uint8_t segments)
{
    void *planes[3] = {y_channel, u_channel, v_channel};
    return decompress_planes(planes, 3, image_w, image_h, image_bufsize, datastream, data_length, stages, (int)filt, segments, 8);
}

}  // extern "C"
