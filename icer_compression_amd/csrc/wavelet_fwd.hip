// wavelet_fwd.hip -- the forward half of lib_icer's standalone wavelet API in libicer_hip.so (include/icer_hip.h):
// icer_wavelet_transform_stages / _2d / _1d (uint16 and uint8), icer_to_sign_magnitude_int16 / _int8 (host-only), and
// the device-resident icerx_wavelet_forward_device the host calls wrap.
//
// Paths, per call:
//   uint16, both sides >= 5   the encoder's fused tile pass (dwt_tile.hpp) with plain two's-complement stores (sm = 0):
//                             stage 0 reads a copy of the plane in the workspace (the tile pass reads a window around what
//                             it writes, so it cannot run in place), every stage writes HL / LH / HH into the plane and its LL
//                             into the workspace's LL chain, the last stage writes its LL into the plane.
//   otherwise                 one thread per line (wavelet_core.hpp): rows of the level (plane -> workspace), then columns
//                             (workspace -> plane).  The uint8 twins go here because the tile pass keeps int16 intermediates,
//                             where the reference truncates every lifting step to int8; lines shorter than 5 go here
//                             because the tile pass clamps the indices the reference lets run past the lows there.
#include <hip/hip_runtime.h>

#include <string.h>

#include "../../include/icer_hip.h"
#include "dwt_tile.hpp"
#include "wavelet_host.hpp"

using namespace icer;

namespace {

// dwt_tile_kernel's body (kernels.hpp) for the standalone transform: every tile, its phases, one overflow flag per plane
__global__ void __launch_bounds__(kTileThreads)
wavelet_tile_kernel(DwtStageArgs a, size_t src_plane, size_t coef_plane, size_t ll_plane, int *__restrict__ ovf)
{
    __shared__ union { DwtTileShared gen; DwtFastShared fast; } u;
    a.src += blockIdx.z * src_plane;
    a.coef += blockIdx.z * coef_plane;
    a.ll += blockIdx.z * ll_plane;
    const int tx = blockIdx.x, ty = blockIdx.y, t = threadIdx.x;
    bool o;
    if (dwt_tile_is_interior(a, tx, ty)) {
        o = dwt_fast_rows_step1(u.fast, a, tx, ty, t);
        __syncthreads();
        o |= dwt_fast_rows_step2(u.fast, a, t);
        __syncthreads();
        o |= dwt_fast_cols_step1(u.fast, a, t);
        __syncthreads();
        o |= dwt_fast_cols_step2(u.fast, a, tx, ty, t);
    } else {
        DwtTileShared &sh = u.gen;
        dwt_tile_load(sh, a, tx, ty, t);
        __syncthreads();
        o = dwt_tile_rows_step1(sh, a, tx, ty, t);
        __syncthreads();
        o |= dwt_tile_rows_step2(sh, a, tx, ty, t);
        __syncthreads();
        o |= dwt_tile_cols_step1(sh, a, tx, ty, t);
        __syncthreads();
        o |= dwt_tile_cols_step2(sh, a, tx, ty, t);
    }
    if (o) atomicOr(&ovf[blockIdx.z], 1);
}

template <class T>
int forward_lines(T *planes, int n, size_t w, size_t h, size_t plane_stride, int mode, int levels, FilterTaps f, const wl::Layout &L,
                  char *ws, hipStream_t st)
{
    int *ovf = (int *)(ws + L.flags_off);
    T *tmp = (T *)(ws + L.buf_off);
    const size_t tmp_plane = L.plane_samples * sizeof(int16_t) / sizeof(T);
    if (mode == kWl1d) {                                 // one line: a copy, then the lifting back into the plane
        WL_TRY(hipMemcpy2DAsync(tmp, tmp_plane * sizeof(T), planes, plane_stride * sizeof(T), w * sizeof(T), n, hipMemcpyDeviceToDevice, st));
        wl::launch_lines<T, false>(tmp, tmp_plane, planes, plane_stride, n, 1, w, 0, 1, f, nullptr, ovf, st);
        WL_TRY(hipGetLastError());
        return 0;
    }
    for (int s = 0; s < levels; s++) {
        const size_t cw = wl_low_dim(w, s), ch = wl_low_dim(h, s);
        wl::launch_lines<T, false>(planes, plane_stride, tmp, tmp_plane, n, ch, cw, w, 1, f, nullptr, ovf, st);      // rows
        wl::launch_lines<T, false>(tmp, tmp_plane, planes, plane_stride, n, cw, ch, 1, w, f, nullptr, ovf, st);      // columns
        WL_TRY(hipGetLastError());
    }
    return 0;
}

int forward_tiles(int16_t *planes, int n, size_t w, size_t h, size_t plane_stride, int levels, FilterTaps f, const wl::Layout &L, char *ws,
                  hipStream_t st)
{
    int16_t *buf = (int16_t *)(ws + L.buf_off);
    const size_t ws_plane = L.plane_samples;
    WL_TRY(hipMemcpy2DAsync(buf, ws_plane * 2, planes, plane_stride * 2, w * h * 2, n, hipMemcpyDeviceToDevice, st));
    DwtStageArgs da;
    da.f = f;
    da.lim = 32767;
    da.sm = 0;
    da.coef = planes; da.coef_stride = (uint32_t)w;
    da.src = buf; da.src_stride = (uint32_t)w;
    size_t src_plane = ws_plane, cw = w, ch = h, ll_off = w * h;
    for (int s = 0; s < levels; s++) {
        const size_t nlw = (cw + 1) / 2, nlh = (ch + 1) / 2;
        da.cw = (int)cw; da.ch = (int)ch;
        size_t ll_plane;
        if (s == levels - 1) { da.ll = planes; da.ll_stride = (uint32_t)w; ll_plane = plane_stride; }
        else { da.ll = buf + ll_off; da.ll_stride = (uint32_t)nlw; ll_plane = ws_plane; }
        hipLaunchKernelGGL(wavelet_tile_kernel, dim3((unsigned)((nlw + kTileKX - 1) / kTileKX), (unsigned)((nlh + kTileKY - 1) / kTileKY), (unsigned)n),
                           dim3(kTileThreads), 0, st, da, src_plane, plane_stride, ll_plane, (int *)(ws + L.flags_off));
        WL_TRY(hipGetLastError());
        da.src = da.ll; da.src_stride = da.ll_stride; src_plane = ll_plane;
        ll_off += nlw * nlh;
        cw = nlw; ch = nlh;
    }
    return 0;
}

// the device path of every forward call; mode kWl2d / kWl1d only from the host calls (geometry checked there)
int forward_enqueue(void *d_planes, int n, size_t w, size_t h, size_t plane_stride, int mode, int stages, int filt, int bits, void *d_ws,
                    int32_t *d_rcs, hipStream_t st)
{
    const wl::Layout L = wl::layout(w, h, n);
    char *ws = (char *)d_ws;
    const FilterTaps f = filter_taps(filt);
    const int levels = mode == kWlStages ? stages : 1;
    WL_TRY(hipMemsetAsync(ws + L.flags_off, 0, sizeof(int) * (size_t)n, st));
    int r = 0;
    if (bits == 16 && mode != kWl1d && w >= 5 && h >= 5) {
        if (levels > 0) r = forward_tiles((int16_t *)d_planes, n, w, h, plane_stride, levels, f, L, ws, st);
    } else if (bits == 16)
        r = forward_lines<int16_t>((int16_t *)d_planes, n, w, h, plane_stride, mode, levels, f, L, ws, st);
    else
        r = forward_lines<int8_t>((int8_t *)d_planes, n, w, h, plane_stride, mode, levels, f, L, ws, st);
    if (r) return r;
    hipLaunchKernelGGL(wl::rcs_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const int *)(ws + L.flags_off), d_rcs, n);
    WL_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

size_t icerx_wavelet_workspace_bytes(size_t w, size_t h, int n_planes, int sample_bits)
{
    (void)sample_bits;                                   // (one layout for both widths)
    return n_planes < 1 ? 0 : wl::layout(w, h, n_planes).total;
}

int icerx_wavelet_forward_device(void *d_planes, int n_planes, size_t w, size_t h, size_t plane_stride, int stages, int filt,
                                 int sample_bits, void *d_workspace, int32_t *d_rcs, void *stream)
{
    const int chk = wl::check_device_args(d_planes, n_planes, w, h, plane_stride, stages, filt, sample_bits, d_workspace, d_rcs);
    if (chk) return chk;
    return forward_enqueue(d_planes, n_planes, w, h, plane_stride, kWlStages, stages, filt, sample_bits, d_workspace, d_rcs, (hipStream_t)stream);
}

int icer_wavelet_transform_stages_uint16(uint16_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt)
{
    return wl::host_call(forward_enqueue, kWlStages, image, image_w, image_h, image_w, stages, (int)filt, 16);
}
int icer_wavelet_transform_2d_uint16(uint16_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt)
{
    return wl::host_call(forward_enqueue, kWl2d, image, image_w, image_h, rowstride, 1, (int)filt, 16);
}
int icer_wavelet_transform_1d_uint16(uint16_t *data, size_t N, size_t stride, enum icer_filter_types filt)
{
    return wl::host_call(forward_enqueue, kWl1d, data, N, 1, stride, 1, (int)filt, 16);
}
int icer_wavelet_transform_stages_uint8(uint8_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt)
{
    return wl::host_call(forward_enqueue, kWlStages, image, image_w, image_h, image_w, stages, (int)filt, 8);
}
int icer_wavelet_transform_2d_uint8(uint8_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt)
{
    return wl::host_call(forward_enqueue, kWl2d, image, image_w, image_h, rowstride, 1, (int)filt, 8);
}
int icer_wavelet_transform_1d_uint8(uint8_t *data, size_t N, size_t stride, enum icer_filter_types filt)
{
    return wl::host_call(forward_enqueue, kWl1d, data, N, 1, stride, 1, (int)filt, 8);
}

// icer_wavelet.c:871-877 / :851-857, on the host (bit manipulation on caller memory)
void icer_to_sign_magnitude_int16(uint16_t *data, size_t len)
{
    for (size_t i = 0; i < len; i++) {
        const uint16_t v = data[i], mask = (uint16_t)((int16_t)v >> 15);
        data[i] = (uint16_t)((((uint16_t)(v + mask)) ^ mask) | (v & 0x8000u));
    }
}
void icer_to_sign_magnitude_int8(uint8_t *data, size_t len)
{
    for (size_t i = 0; i < len; i++) {
        const uint8_t v = data[i], mask = (uint8_t)((int8_t)v >> 7);
        data[i] = (uint8_t)((((uint8_t)(v + mask)) ^ mask) | (v & 0x80u));
    }
}

}  // extern "C"
