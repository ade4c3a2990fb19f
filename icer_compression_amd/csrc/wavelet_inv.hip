// wavelet_inv.hip -- the inverse half of lib_icer's standalone wavelet API in libicer_hip_dec.so (include/icer_hip_dec.h):
// icer_inverse_wavelet_transform_stages / _2d / _1d (uint16 and uint8), icer_from_sign_magnitude_int16 / _int8
// (host-only), and the device-resident icerx_wavelet_inverse_device the host calls wrap.
//
// Filter A: one LDS-tiled pass per level (wavelet_inv.hpp).  The other filters: the reference's two passes per level
// (icer_wavelet.c:175-191), the columns of the level's region (plane -> workspace), then its rows (workspace -> plane),
// one lane per line (wl_inv_line, wavelet_core.hpp: the stored values of 32 steps loaded ahead of the serial chain).  The uint8 twins run on their int8 samples directly; on odd lengths their outputs go through the
// position tables of the uint8 interleave (built on the device, one thread per table, into the workspace).
#include <hip/hip_runtime.h>

#include "../../include/icer_hip_dec.h"
#include "wavelet_host.hpp"
#include "wavelet_inv.hpp"

using namespace icer;

namespace {

// uint8 interleave position table of one line length (one thread: the reference's in-place shuffle on an index array)
__global__ void pos_table_kernel(uint32_t len, uint32_t *__restrict__ tmp, uint32_t *__restrict__ pos_of)
{
    wl_interleave_positions_u8(len, tmp, pos_of);
}

// filter A: one level in one LDS-tiled pass (wavelet_inv.hpp); grid = (ceil(nlw / 32), ceil(nlh / 8), planes)
template <class T>
__global__ void __launch_bounds__(kIaThreads)
inv_tile_a_kernel(IaArgs a, size_t src_plane, size_t dst_plane, int *__restrict__ ovf)
{
    __shared__ IaShared sh;
    a.src = (const T *)a.src + blockIdx.z * src_plane;
    a.dst = (T *)a.dst + blockIdx.z * dst_plane;
    const int tx = blockIdx.x, ty = blockIdx.y, t = threadIdx.x;
    ia_load<T>(sh, a, tx, ty, t);
    __syncthreads();
    bool o = ia_cols<T>(sh, a, ty, t);
    __syncthreads();
    o |= ia_rows<T>(sh, a, tx, ty, t);
    if (o) atomicOr(&ovf[blockIdx.z], 1);
}

template <class T>
int inverse_lines(T *planes, int n, size_t w, size_t h, size_t plane_stride, int mode, int levels, FilterTaps f, const wl::Layout &L,
                  char *ws, hipStream_t st)
{
    int *ovf = (int *)(ws + L.flags_off);
    T *tmp = (T *)(ws + L.buf_off);
    const size_t tmp_plane = L.plane_samples * sizeof(int16_t) / sizeof(T);
    uint32_t *tables = (uint32_t *)(ws + L.pos_off);
    // a table for an odd uint8 line length: [scratch | positions], built on the stream ahead of its use
    auto table = [&](size_t len) -> const uint32_t * {
        if (sizeof(T) != 1 || !(len & 1)) return nullptr;
        uint32_t *t = tables;
        tables += 2 * len;
        hipLaunchKernelGGL(pos_table_kernel, dim3(1), dim3(1), 0, st, (uint32_t)len, t, t + len);
        return t + len;
    };
    if (mode == kWl1d) {
        const uint32_t *pos = table(w);
        WL_TRY(hipMemcpy2DAsync(tmp, tmp_plane * sizeof(T), planes, plane_stride * sizeof(T), w * sizeof(T), n, hipMemcpyDeviceToDevice, st));
        wl::launch_lines<T, true>(tmp, tmp_plane, planes, plane_stride, n, 1, w, 0, 1, f, pos, ovf, st);
        WL_TRY(hipGetLastError());
        return 0;
    }
    // filter A: one tiled pass per level when every level's lines have >= 5 samples and need no uint8 position table.
    // The levels alternate between the plane and a copy of it in the workspace (their detail bands are the same), so that
    // the last level writes the plane.
    bool tiled = f.am1 == 0 && f.be == 0;
    for (int lv = 0; lv < levels && tiled; lv++) {
        const size_t cw = wl_low_dim(w, lv), ch = wl_low_dim(h, lv);
        tiled = cw >= 5 && ch >= 5 && (sizeof(T) == 2 || ((cw | ch) & 1) == 0);
    }
    if (tiled) {
        if (levels == 0) return 0;
        WL_TRY(hipMemcpy2DAsync(tmp, tmp_plane * sizeof(T), planes, plane_stride * sizeof(T), w * h * sizeof(T), n, hipMemcpyDeviceToDevice, st));
        for (int it = 0; it < levels; it++) {
            const int lv = levels - 1 - it;
            const bool to_plane = (lv & 1) == 0;
            IaArgs a;
            a.src = to_plane ? (const void *)tmp : (const void *)planes;
            a.dst = to_plane ? (void *)planes : (void *)tmp;
            a.w = (uint32_t)w; a.cw = (uint32_t)wl_low_dim(w, lv); a.ch = (uint32_t)wl_low_dim(h, lv); a.f = f;
            const size_t nlw = (a.cw + 1) / 2, nlh = (a.ch + 1) / 2;
            hipLaunchKernelGGL(inv_tile_a_kernel<T>, dim3((unsigned)((nlw + kIaPX - 1) / kIaPX), (unsigned)((nlh + kIaPY - 1) / kIaPY), (unsigned)n),
                               dim3(kIaThreads), 0, st, a, to_plane ? tmp_plane : plane_stride, to_plane ? plane_stride : tmp_plane, ovf);
            WL_TRY(hipGetLastError());
        }
        return 0;
    }
    for (int it = 0; it < levels; it++) {                // deepest level first (icer_wavelet.c:96-101)
        const int lv = levels - 1 - it;
        const size_t cw = wl_low_dim(w, lv), ch = wl_low_dim(h, lv);
        const uint32_t *col_pos = table(ch), *row_pos = table(cw);
        wl::launch_lines<T, true>(planes, plane_stride, tmp, tmp_plane, n, cw, ch, 1, w, f, col_pos, ovf, st);     // columns
        wl::launch_lines<T, true>(tmp, tmp_plane, planes, plane_stride, n, ch, cw, w, 1, f, row_pos, ovf, st);     // rows
        WL_TRY(hipGetLastError());
    }
    return 0;
}

int inverse_enqueue(void *d_planes, int n, size_t w, size_t h, size_t plane_stride, int mode, int stages, int filt, int bits, void *d_ws,
                    int32_t *d_rcs, hipStream_t st)
{
    const wl::Layout L = wl::layout(w, h, n);
    char *ws = (char *)d_ws;
    const FilterTaps f = filter_taps(filt);
    const int levels = mode == kWlStages ? stages : 1;
    WL_TRY(hipMemsetAsync(ws + L.flags_off, 0, sizeof(int) * (size_t)n, st));
    const int r = bits == 16 ? inverse_lines<int16_t>((int16_t *)d_planes, n, w, h, plane_stride, mode, levels, f, L, ws, st)
                             : inverse_lines<int8_t>((int8_t *)d_planes, n, w, h, plane_stride, mode, levels, f, L, ws, st);
    if (r) return r;
    hipLaunchKernelGGL(wl::rcs_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const int *)(ws + L.flags_off), d_rcs, n);
    WL_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int icerx_wavelet_inverse_device(void *d_planes, int n_planes, size_t w, size_t h, size_t plane_stride, int stages, int filt,
                                 int sample_bits, void *d_workspace, int32_t *d_rcs, void *stream)
{
    const int chk = wl::check_device_args(d_planes, n_planes, w, h, plane_stride, stages, filt, sample_bits, d_workspace, d_rcs);
    if (chk) return chk;
    return inverse_enqueue(d_planes, n_planes, w, h, plane_stride, kWlStages, stages, filt, sample_bits, d_workspace, d_rcs, (hipStream_t)stream);
}

int icer_inverse_wavelet_transform_stages_uint16(uint16_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt)
{
    return wl::host_call(inverse_enqueue, kWlStages, image, image_w, image_h, image_w, stages, (int)filt, 16);
}
int icer_inverse_wavelet_transform_2d_uint16(uint16_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt)
{
    return wl::host_call(inverse_enqueue, kWl2d, image, image_w, image_h, rowstride, 1, (int)filt, 16);
}
int icer_inverse_wavelet_transform_1d_uint16(uint16_t *data, size_t N, size_t stride, enum icer_filter_types filt)
{
    return wl::host_call(inverse_enqueue, kWl1d, data, N, 1, stride, 1, (int)filt, 16);
}
int icer_inverse_wavelet_transform_stages_uint8(uint8_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt)
{
    return wl::host_call(inverse_enqueue, kWlStages, image, image_w, image_h, image_w, stages, (int)filt, 8);
}
int icer_inverse_wavelet_transform_2d_uint8(uint8_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt)
{
    return wl::host_call(inverse_enqueue, kWl2d, image, image_w, image_h, rowstride, 1, (int)filt, 8);
}
int icer_inverse_wavelet_transform_1d_uint8(uint8_t *data, size_t N, size_t stride, enum icer_filter_types filt)
{
    return wl::host_call(inverse_enqueue, kWl1d, data, N, 1, stride, 1, (int)filt, 8);
}

// icer_wavelet.c:880-886 / :860-866, on the host (bit manipulation on caller memory)
void icer_from_sign_magnitude_int16(uint16_t *data, size_t len)
{
    for (size_t i = 0; i < len; i++) {
        const uint16_t v = data[i], mask = (uint16_t)((int16_t)v >> 15);
        data[i] = (uint16_t)((~mask & v) | ((uint16_t)((int16_t)(v & 0x8000u) - (int16_t)v) & mask));
    }
}
void icer_from_sign_magnitude_int8(uint8_t *data, size_t len)
{
    for (size_t i = 0; i < len; i++) {
        const uint8_t v = data[i], mask = (uint8_t)((int8_t)v >> 7);
        data[i] = (uint8_t)((~mask & v) | ((uint8_t)((int8_t)(v & 0x80u) - (int8_t)v) & mask));
    }
}

}  // extern "C"
