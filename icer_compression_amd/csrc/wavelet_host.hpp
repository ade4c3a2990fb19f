// wavelet_host.hpp -- host side of the standalone wavelet transform, shared by wavelet_fwd.hip (libicer_hip.so) and
// wavelet_inv.hip (libicer_hip_dec.so): the caller's workspace layout, the small kernels both directions use, and the
// lib_icer-shaped host calls as thin wrappers around the device path (icerx_wavelet_forward_device /
// icerx_wavelet_inverse_device).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <stdio.h>
#include <stdlib.h>

#include "wavelet_core.hpp"

namespace icer {
namespace wl {
namespace {              // (internal linkage: both libraries compile this file)

// ------------------------------------------------------------------------------------------ workspace
// [per-plane overflow flags | uint8 interleave tables | per plane: a w*h scratch region + the forward LL chain]
struct Layout {
    size_t flags_off, pos_off, buf_off;
    size_t plane_samples;               // int16 samples of one plane's scratch block
    size_t total;
};
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline Layout layout(size_t w, size_t h, int n_planes)
{
    size_t ll = 0, tables = 0;
    for (size_t cw = w, ch = h;;) {                     // every level a stages call can reach
        tables += 2 * (cw + ch);
        if (cw <= 1 && ch <= 1) break;
        cw = (cw + 1) / 2; ch = (ch + 1) / 2;
        ll += cw * ch;
    }
    Layout L;
    L.flags_off = 0;
    L.pos_off = align_up(sizeof(int) * (size_t)n_planes, 256);
    L.buf_off = align_up(L.pos_off + sizeof(uint32_t) * tables, 256);
    L.plane_samples = align_up(w * h + ll, 64);
    L.total = L.buf_off + sizeof(int16_t) * L.plane_samples * (size_t)n_planes;
    return L;
}

// ------------------------------------------------------------------------------------------ kernels
// one thread per line: forward or inverse lifting (wavelet_core.hpp); grid = (ceil(lines / 64), planes), block = 64
template <class T, bool Inv>
__global__ void __launch_bounds__(64)
lines_kernel(const T *__restrict__ src, size_t src_plane, T *__restrict__ dst, size_t dst_plane, uint32_t n_lines, uint32_t n,
             size_t line_step, size_t elem_step, FilterTaps f, const uint32_t *__restrict__ pos_of, int *__restrict__ ovf)
{
    const uint32_t line = blockIdx.x * blockDim.x + threadIdx.x;
    if (line >= n_lines) return;
    const T *s = src + blockIdx.y * src_plane + line * line_step;
    T *d = dst + blockIdx.y * dst_plane + line * line_step;
    const bool o = Inv ? wl_inv_line<T>(s, d, n, elem_step, f, pos_of) : wl_fwd_line<T>(s, d, n, elem_step, f);
    if (o) atomicOr(&ovf[blockIdx.y], 1);
}

// per-plane result codes from the overflow flags (on the stream: nothing waits on the host)
__global__ void rcs_kernel(const int *__restrict__ ovf, int32_t *__restrict__ rcs, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rcs[i] = ovf[i] ? -1 : 0;                 // ICER_INTEGER_OVERFLOW / ICER_RESULT_OK
}

template <class T, bool Inv>
inline void launch_lines(const T *src, size_t src_plane, T *dst, size_t dst_plane, int planes, size_t n_lines, size_t n, size_t line_step,
                         size_t elem_step, FilterTaps f, const uint32_t *pos_of, int *ovf, hipStream_t st)
{
    hipLaunchKernelGGL((lines_kernel<T, Inv>), dim3((unsigned)((n_lines + 63) / 64), (unsigned)planes), dim3(64), 0, st, src, src_plane, dst, dst_plane,
                       (uint32_t)n_lines, (uint32_t)n, line_step, elem_step, f, pos_of, ovf);
}

inline int fail(const char *what, hipError_t e)
{
    fprintf(stderr, "icer_hip: wavelet transform: %s: %s\n", what, hipGetErrorString(e));
    return -10;                                          // ICER_FATAL_ERROR
}
#define WL_TRY(expr)                                      \
    do {                                                  \
        const hipError_t wl_e_ = (expr);                  \
        if (wl_e_ != hipSuccess) return wl::fail(#expr, wl_e_); \
    } while (0)

constexpr int kMaxPlanes = 65535;                  // planes go on grid.y / grid.z

// argument checks shared by the two device entry points (before anything is enqueued)
inline int check_device_args(const void *d_planes, int n_planes, size_t w, size_t h, size_t plane_stride, int stages, int filt, int bits,
                             const void *ws, const int32_t *rcs)
{
    if (!d_planes || !ws || !rcs || n_planes < 1 || n_planes > kMaxPlanes || (bits != 8 && bits != 16) || filt < 0 || filt > 6 || plane_stride < w * h ||
        w > 0xFFFFFFFFu || h > 0xFFFFFFFFu)
        return -11;                                      // ICER_INVALID_INPUT
    return wl_check(kWlStages, w, h, stages);
}

// ------------------------------------------------------------------------------------------ lib_icer-shaped host calls
// Device-path signature: (d_planes, n_planes, w, h, plane_stride, mode, stages, filt, bits, d_ws, d_rcs, stream)
using Enqueue = int (*)(void *, int, size_t, size_t, size_t, int, int, int, int, void *, int32_t *, hipStream_t);

// One host call: the caller's samples (contiguous stages plane, a rowstride'd 2-D region, or N samples at stride) go to a
// contiguous device plane, the device path runs on the library's stream, the samples come back.  Serialised by a mutex,
// like the other lib_icer-shaped entry points; the device is ICER_HIP_DEVICE (default 0).
inline int host_call(Enqueue enqueue, int mode, void *data, size_t w, size_t h, size_t stride, int stages, int filt, int bits)
{
    const int chk = wl_check(mode, w, h, stages);
    if (chk) return chk;
    if (!data || filt < 0 || filt > 6 || (mode != kWlStages && stride < (mode == kWl2d ? w : 1)) || w > 0xFFFFFFFFu || h > 0xFFFFFFFFu) return -11;
    static std::mutex mu;
    static void *d_plane = nullptr, *d_ws = nullptr;
    static int32_t *d_rc = nullptr;
    static size_t plane_cap = 0, ws_cap = 0;
    static hipStream_t st = nullptr;
    static int st_dev = -1;
    std::lock_guard<std::mutex> lk(mu);
    const char *env = getenv("ICER_HIP_DEVICE");
    const int dev = env ? atoi(env) : 0;
    WL_TRY(hipSetDevice(dev));
    if (st_dev != dev) {                                 // (buffers of another device: start over)
        if (st) { (void)hipStreamDestroy(st); st = nullptr; }
        if (d_plane) (void)hipFree(d_plane);
        if (d_ws) (void)hipFree(d_ws);
        if (d_rc) (void)hipFree(d_rc);
        d_plane = d_ws = nullptr; d_rc = nullptr; plane_cap = ws_cap = 0;
        WL_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        WL_TRY(hipMalloc((void **)&d_rc, sizeof(int32_t)));
        st_dev = dev;
    }
    const size_t es = (size_t)bits / 8, hh = mode == kWl1d ? 1 : h;
    const size_t bytes = es * w * hh, need_ws = layout(w, hh, 1).total;
    if (bytes > plane_cap) {
        if (d_plane) (void)hipFree(d_plane);
        d_plane = nullptr; plane_cap = 0;
        WL_TRY(hipMalloc(&d_plane, bytes));
        plane_cap = bytes;
    }
    if (need_ws > ws_cap) {
        if (d_ws) (void)hipFree(d_ws);
        d_ws = nullptr; ws_cap = 0;
        WL_TRY(hipMalloc(&d_ws, need_ws));
        ws_cap = need_ws;
    }
    if (mode == kWlStages) WL_TRY(hipMemcpyAsync(d_plane, data, bytes, hipMemcpyHostToDevice, st));
    else if (mode == kWl2d) WL_TRY(hipMemcpy2DAsync(d_plane, w * es, data, stride * es, w * es, h, hipMemcpyHostToDevice, st));
    else WL_TRY(hipMemcpy2DAsync(d_plane, es, data, stride * es, es, w, hipMemcpyHostToDevice, st));
    const int r = enqueue(d_plane, 1, w, hh, w * hh, mode, stages, filt, bits, d_ws, d_rc, st);
    if (r) { (void)hipStreamSynchronize(st); return r; }
    if (mode == kWlStages) WL_TRY(hipMemcpyAsync(data, d_plane, bytes, hipMemcpyDeviceToHost, st));
    else if (mode == kWl2d) WL_TRY(hipMemcpy2DAsync(data, stride * es, d_plane, w * es, w * es, h, hipMemcpyDeviceToHost, st));
    else WL_TRY(hipMemcpy2DAsync(data, stride * es, d_plane, es, es, w, hipMemcpyDeviceToHost, st));
    int32_t rc = 0;
    WL_TRY(hipMemcpyAsync(&rc, d_rc, sizeof rc, hipMemcpyDeviceToHost, st));
    WL_TRY(hipStreamSynchronize(st));
    return rc;
}

}  // namespace
}  // namespace wl
}  // namespace icer
