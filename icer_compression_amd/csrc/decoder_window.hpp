// decoder_window.hpp -- the window decode (include/icer_hip_dec_window.h): every frame of a batch delivers a rectangle of its
// image only, stored compactly, and runs only the chains that rectangle depends on.  Which chains those are is decided in
// the two planners (plan_decode_window, decoder_plan.hpp; dplan_window_keeps, decoder_dplan.hpp) from one per-frame
// WinGeom; the chain kernels are the plain call's.  Here: everything behind the chains, restricted by the same WinGeom.
//
//   unsign     sign-magnitude removal and the LL mean over the needed rectangle of every subband (win_unsign_kernel)
//   inverse    per level, columns then rows as the plain call: filter A by pairs over the needed pair and line ranges
//              (win_idwt_pairs_kernel); the other filters by lines, over the needed lines, the backward walk starting at
//              the end of the line and stopping at the first needed pair (win_idwt_lines_kernel, idwt_line_at's k_stop)
//   finish     clamp, narrow or convert to gray8 / RGB888, and the compact store of the window (win_finish_kernel)
// A frame that does not reach the transform (or whose transform has no levels) keeps all its chains: its passes run over the
// whole frame and the last one crops.  The geometry of every frame is read from device memory, so the synchronous calls
// (decode_window_batch, planned on the host) and the asynchronous ones (decoder_async.hpp, planned on the device by
// window_frames_kernel) enqueue the same kernels; every kernel strides over its frame's work with a grid the host sizes
// without knowing the windows.  Included by decoder.hip after its kernels and the stages of decode_batch.
#pragma once
#include "decoder_dplan.hpp"
#include "wavelet_core.hpp"

namespace {

constexpr int kWinInfo = 6;                       // uint32 per frame: x0, y0, ww, wh, chains run, chains of the plain call

// blocks of `per_block` items for up to `items` items per frame, at most `cap`
unsigned win_blocks(size_t items, size_t per_block, size_t cap)
{
#ifdef ICER_HOST_MOCK
    cap = 2;                                       // (the mock runs the blocks one after the other: a few, each striding)
#endif
    return (unsigned)std::max<size_t>(1, std::min((items + per_block - 1) / per_block, cap));
}

// where value v of a line's [lows | highs] lands: the plain interleave, or for the odd lines of an 8-bit decoder (always
// whole lines) the frame's table of the level (win_positions_kernel: [columns | scratch | rows | scratch])
ICER_HD DPos win_pos(const uint32_t *pos, size_t pos_words, uint32_t frame, const WinLevel &L, bool rows, int bits)
{
    const uint32_t n = rows ? L.x.n : L.y.n;
    DPos p;
    p.nl = (n + 1u) / 2u;
    p.tab = (bits == 8 && (n & 1u)) ? pos + (size_t)frame * pos_words + (rows ? 2u * L.y.n : 0u) : nullptr;
    return p;
}
__global__ void __launch_bounds__(64)
win_positions_kernel(const WinGeom *__restrict__ geom, uint32_t n, int j, uint32_t *__restrict__ pos, size_t pos_words)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < 2u * n; i += gridDim.x * blockDim.x) {
        const WinGeom &g = geom[i / 2u];
        const bool rows = (i & 1u) != 0;
        const uint32_t len = rows ? g.lv[j].x.n : g.lv[j].y.n;
        if (!g.active || (uint32_t)j >= g.nlev || !(len & 1u)) continue;
        uint32_t *t = pos + (size_t)(i / 2u) * pos_words + (rows ? 2u * g.lv[j].y.n : 0u);
        wl_interleave_positions_u8(len, t + len, t);
    }
}

// sign-magnitude words -> int16 with the LL mean, over the needed rectangle of every subband (grid.y = frame * channels + channel)
__global__ void __launch_bounds__(256)
win_unsign_kernel(uint16_t *__restrict__ planes, size_t full_stride, int channels, const FrameInfo *__restrict__ frames,
                  const WinGeom *__restrict__ geom, int sign_bit, int bits)
{
    const uint32_t frame = blockIdx.y / (unsigned)channels;
    const FrameInfo f = frames[frame];
    const WinGeom &g = geom[frame];
    if (!f.transform || g.skip) return;
    uint16_t *p = planes + (size_t)blockIdx.y * full_stride;
    const uint16_t mean = f.mean[blockIdx.y % (unsigned)channels];
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    if (!g.active) {                               // (a transform without levels: the whole frame, as unsign_kernel)
        for (size_t i = tid; i < (size_t)f.w * f.h; i += step) {
            int16_t s = from_sign_magnitude(p[i], sign_bit);
            if ((uint32_t)(i % f.w) < f.ll_w && (uint32_t)(i / f.w) < f.ll_h) s = add_ll_mean(s, mean, bits);
            p[i] = (uint16_t)s;
        }
        return;
    }
    for (uint32_t lv = 1; lv <= g.nlev; lv++)
        for (uint32_t sb = (lv == g.nlev ? 0u : 1u); sb < 4u; sb++) {
            const WinAxis &ax = g.lv[lv - 1u].x, &ay = g.lv[lv - 1u].y;
            const uint32_t x0 = (sb & 1u) ? (ax.n + 1u) / 2u + ax.hi0 : ax.lo0, rw = (sb & 1u) ? ax.hi1 - ax.hi0 : ax.lo1 - ax.lo0;
            const uint32_t y0 = (sb & 2u) ? (ay.n + 1u) / 2u + ay.hi0 : ay.lo0, rh = (sb & 2u) ? ay.hi1 - ay.hi0 : ay.lo1 - ay.lo0;
            for (size_t i = tid; i < (size_t)rw * rh; i += step) {
                const size_t at = (size_t)(y0 + (uint32_t)(i / rw)) * f.w + x0 + (uint32_t)(i % rw);
                int16_t s = from_sign_magnitude(p[at], sign_bit);
                if (sb == 0u) s = add_ll_mean(s, mean, bits);
                p[at] = (uint16_t)s;
            }
        }
}

// the lines of one pass of level j: rows = false, the columns of the needed lows and highs of x, restored along y; rows =
// true, the wanted rows of y, restored along x
struct WinPass {
    uint32_t n, k0, k1, lines, lo0, nlo, hi_at;
    ICER_HD uint32_t line(uint32_t i) const { return i < nlo ? lo0 + i : hi_at + (i - nlo); }
};
ICER_HD WinPass win_pass(const WinLevel &L, bool rows)
{
    const WinAxis &along = rows ? L.x : L.y, &across = rows ? L.y : L.x;
    WinPass p;
    p.n = along.n;
    win_pairs(along, &p.k0, &p.k1);
    if (rows) { p.lo0 = across.a; p.nlo = across.b - across.a; p.hi_at = 0u; p.lines = p.nlo; }
    else {
        p.lo0 = across.lo0; p.nlo = across.lo1 - across.lo0; p.hi_at = (across.n + 1u) / 2u + across.hi0;
        p.lines = p.nlo + (across.hi1 - across.hi0);
    }
    return p;
}

// filter A (idwt_pair_at): one thread per needed output pair of a needed line; consecutive threads along a row of the image
__global__ void __launch_bounds__(256)
win_idwt_pairs_kernel(const int16_t *__restrict__ src, int16_t *__restrict__ dst, size_t full_stride, int channels,
                      const WinGeom *__restrict__ geom, int j, FilterTaps taps, int bits, const uint32_t *__restrict__ pos,
                      size_t pos_words, bool rows)
{
    const uint32_t frame = blockIdx.y / (unsigned)channels;
    const WinGeom &g = geom[frame];
    if (!g.active || (uint32_t)j >= g.nlev) return;
    const WinPass ps = win_pass(g.lv[j], rows);
    const uint32_t npairs = ps.k1 - ps.k0;
    const DPos p = win_pos(pos, pos_words, frame, g.lv[j], rows, bits);
    const size_t base = (size_t)blockIdx.y * full_stride, total = (size_t)ps.lines * npairs, stride = rows ? 1 : g.w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t li = rows ? (uint32_t)(i / npairs) : (uint32_t)(i % ps.lines);
        const uint32_t k = ps.k0 + (rows ? (uint32_t)(i % npairs) : (uint32_t)(i / ps.lines));
        const size_t at = base + (rows ? (size_t)ps.line(li) * g.w : (size_t)ps.line(li));
        idwt_pair_at(src + at, dst + at, ps.n, stride, k, taps, bits, p);
    }
}

// the other filters: one thread per needed line
__global__ void __launch_bounds__(64)
win_idwt_lines_kernel(const int16_t *__restrict__ src, int16_t *__restrict__ dst, size_t full_stride, int channels,
                      const WinGeom *__restrict__ geom, int j, FilterTaps taps, int bits, const uint32_t *__restrict__ pos,
                      size_t pos_words, bool rows)
{
    const uint32_t frame = blockIdx.y / (unsigned)channels;
    const WinGeom &g = geom[frame];
    if (!g.active || (uint32_t)j >= g.nlev) return;
    const WinPass ps = win_pass(g.lv[j], rows);
    if (ps.k0 >= ps.k1) return;
    const DPos p = win_pos(pos, pos_words, frame, g.lv[j], rows, bits);
    const size_t base = (size_t)blockIdx.y * full_stride;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ps.lines; i += gridDim.x * blockDim.x) {
        const size_t at = base + (rows ? (size_t)ps.line(i) * g.w : (size_t)ps.line(i));
        idwt_line_at(src + at, dst + at, ps.n, rows ? (size_t)1 : (size_t)g.w, taps, bits, p, ps.k0);
    }
}

// the last pass: the window's samples finished as finish_kernel / display_finish_kernel finish them, stored compactly.
// Planes: channel c of frame k at out + (k * channels + c) * frame_stride samples (uint16, or uint8 for an 8-bit decoder);
// display: frame k at out + k * channels * frame_stride bytes.  grid.y = frame.
__global__ void __launch_bounds__(256)
win_finish_kernel(const uint16_t *__restrict__ planes, size_t full_stride, int channels, const FrameInfo *__restrict__ frames,
                  const WinGeom *__restrict__ geom, int bits, void *__restrict__ out, size_t frame_stride, bool display)
{
    const uint32_t frame = blockIdx.y;
    const WinGeom &g = geom[frame];
    if (g.skip) return;
    const FrameInfo f = frames[frame];
    const size_t total = (size_t)g.ww * g.wh, first = (size_t)frame * channels;
    const bool transform = f.transform != 0u;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t at = (size_t)(g.y0 + (uint32_t)(i / g.ww)) * f.w + g.x0 + (uint32_t)(i % g.ww);
        uint32_t v[3] = {0u, 0u, 0u};
        for (int c = 0; c < channels; c++) v[c] = display_finished(planes[(first + c) * full_stride + at], transform, bits);
        if (display) {
            uint8_t *o = (uint8_t *)out + first * frame_stride + i * (size_t)channels;
            const uint32_t px = channels == 3 ? display_pixel<3>(v) : display_pixel<1>(v);
            for (int c = 0; c < channels; c++) o[c] = (uint8_t)(px >> (8 * c));
        } else if (bits == 8) {
            for (int c = 0; c < channels; c++) ((uint8_t *)out)[(first + c) * frame_stride + i] = (uint8_t)v[c];
        } else {
            for (int c = 0; c < channels; c++) ((uint16_t *)out)[(first + c) * frame_stride + i] = (uint16_t)v[c];
        }
    }
}

// ------------------------------------------------------------------------------------------ the asynchronous calls' part
// what icerx_decode_device_window_async hands to decode_async (decoder_async.hpp) besides the plain call's arguments
struct WindowCall {
    const uint32_t *d_windows;                     // device, n x 4: x, y, w, h
    uint32_t *d_info;                              // device, n x kWinInfo
    size_t full_stride;                            // samples of a working plane: what frame_stride is to the plain call
};
size_t window_geom_bytes(int n) { return (sizeof(WinGeom) * (size_t)n + 255u) & ~(size_t)255u; }

// One workgroup per frame, behind plan_frames_kernel (decoder_async.hpp): the frame's WinGeom from its FrameInfo and its
// window, its info, and every chain slot the window does not depend on emptied (dplan_window_keeps).  A window of more
// than out_stride samples: ICER_BYTE_QUOTA_EXCEEDED, and the frame no longer runs.
__global__ void __launch_bounds__(64)
window_frames_kernel(const uint32_t *__restrict__ windows, DPlanGeom geom, uint64_t out_stride, bool pairwise, int bits,
                     ChainDesc *__restrict__ chains, FrameInfo *__restrict__ frames, int32_t *__restrict__ rcs,
                     WinGeom *__restrict__ geoms, uint32_t *__restrict__ info)
{
    const uint32_t k = blockIdx.x, tid = threadIdx.x;
    const FrameInfo f = frames[k];
    uint32_t *o = info + (size_t)k * kWinInfo;
    if (tid == 0) {
        WinGeom g;
        win_geom(&g, f.w, f.h, (int)geom.stages, f.w != 0u && f.h != 0u, f.transform && f.ll_w >= 3u && f.ll_h >= 3u, windows + 4u * (size_t)k,
                 out_stride, pairwise, bits);
        geoms[k] = g;
        o[0] = g.x0; o[1] = g.y0; o[2] = g.ww; o[3] = g.wh; o[4] = 0u; o[5] = 0u;
    }
#ifndef ICER_HOST_MOCK
    __syncthreads();
#endif
    const WinGeom &g = geoms[k];
    ChainDesc *mine = chains + (size_t)k * geom.chain_slots();
    uint32_t run = 0, full = 0;
    for (uint32_t j = tid; j < geom.chain_slots(); j += blockDim.x) {
        if (mine[j].frame == kNoChain) continue;
        full++;
        if (dplan_window_keeps(geom, g, f.w, f.h, j)) run++;
        else mine[j].frame = kNoChain;
    }
    if (run) atomicAdd(&o[4], run);
    if (full) atomicAdd(&o[5], full);
    if (tid == 0 && g.skip) {
        rcs[k] = kByteQuotaExceeded;
        frames[k].w = 0u; frames[k].h = 0u; frames[k].transform = 0u;
    }
}

// position-table words a frame needs (8-bit decoders): the lines of a level are at most w + h <= full_stride / 3 + 3 samples
// together when the transform runs (both sides >= 3)
size_t win_pos_words(int bits, size_t full_stride) { return bits == 8 ? 2u * (full_stride / 3u + 4u) : 0u; }

// Everything behind the chains, enqueued on `st`.  planes / tmp: n * channels working planes of full_stride samples; frames,
// geom, pos, chains: device memory; `slots` chain records (empty ones marked kNoChain); `span`: an upper bound of the
// samples of a frame that any pass touches (the grids are sized by it).
int enqueue_window_samples(icerx_decoder *d, int n, uint16_t *planes, int16_t *tmp, size_t full_stride, const FrameInfo *frames,
                           const WinGeom *geom, uint32_t *pos, const ChainDesc *chains, uint32_t slots, int recon, void *out,
                           size_t frame_stride, bool display, size_t span, hipStream_t st)
{
    (void)st;
    int rc = ICER_RESULT_OK;
    const int channels = d->channels, bits = d->bits, stages = d->stages;
    const PlaneBits pb = plane_bits(bits);
    const FilterTaps taps = filter_taps(d->filt);
    const bool pairwise = taps.be == 0 && taps.am1 == 0;
    const size_t pos_words = win_pos_words(bits, full_stride);
    const unsigned gy = (unsigned)(n * channels), cus = (unsigned)d->n_cus;
    const unsigned per_frame = std::max(1u, 8u * cus / gy);
    span = std::max<size_t>(1, std::min(span, full_stride));
    if (recon != 0 && slots) {
        ICER_LAUNCH_ON(st, reconstruct_kernel, dim3(slots, kReconParts), kReconThreads, 0, planes, full_stride, channels, chains, slots,
                       frames, (uint32_t)n, pb.nplanes, pb.sign_bit, recon);
        HIP_TRY(hipGetLastError());
    }
    ICER_LAUNCH_ON(st, win_unsign_kernel, dim3(win_blocks(span, 256, per_frame), gy), 256, 0, planes, full_stride, channels, frames, geom,
                   pb.sign_bit, bits);
    HIP_TRY(hipGetLastError());
    for (int j = stages - 1; j >= 0; j--) {
        if (bits == 8) {
            ICER_LAUNCH_ON(st, win_positions_kernel, win_blocks(2u * (size_t)n, 64, 4u * cus), 64, 0, geom, (uint32_t)n, j, pos, pos_words);
            HIP_TRY(hipGetLastError());
        }
        for (int rows = 0; rows < 2; rows++) {
            const int16_t *src = rows ? (const int16_t *)tmp : (const int16_t *)planes;
            int16_t *dst = rows ? (int16_t *)planes : tmp;
            if (pairwise)
                ICER_LAUNCH_ON(st, win_idwt_pairs_kernel, dim3(win_blocks(span / 2u + 1u, 256, per_frame), gy), 256, 0, src, dst, full_stride,
                               channels, geom, j, taps, bits, pos, pos_words, rows != 0);
            else
                ICER_LAUNCH_ON(st, win_idwt_lines_kernel, dim3(win_blocks(full_stride / 3u + 4u, 64, 4u * per_frame), gy), 64, 0, src, dst,
                               full_stride, channels, geom, j, taps, bits, pos, pos_words, rows != 0);
            HIP_TRY(hipGetLastError());
        }
    }
    ICER_LAUNCH_ON(st, win_finish_kernel, dim3(win_blocks(std::min(span, frame_stride), 256, per_frame * (unsigned)channels), (unsigned)n), 256,
                   0, planes, full_stride, channels, frames, geom, bits, out, frame_stride, display);
    HIP_TRY(hipGetLastError());
done:
    return rc;
}

// ------------------------------------------------------------------------------------------ synchronous window decode
// decode_batch with a window per frame (windows: host, n x 4 uint32).  The working planes are the decoder's, n * channels of
// full_stride samples; `out` as decode_batch's, holding windows of at most frame_stride samples.
int decode_window_batch(icerx_decoder *d, int n, const uint8_t *data, bool data_on_device, const size_t *offsets, const size_t *lens,
                        const uint32_t *windows, BatchOut out, size_t frame_stride, size_t full_stride, int *rcs, size_t *ws, size_t *hs,
                        uint32_t *info)
{
    g_error.clear();
    if (!d || n < 0 || (n && (!offsets || !lens || !rcs || !ws || !hs || !windows || !info || !out.p))) return ICER_INVALID_INPUT;
    if (n == 0) return ICER_RESULT_OK;
    const int channels = d->channels, bits = d->bits;
    const bool display = out.display(), to_host = out.to_host();
    if (to_host)
        for (int k = 0; k < n * (display ? 1 : channels); k++)
            if (!((void *const *)out.p)[k]) return ICER_INVALID_INPUT;
    BatchRun r;
    const size_t unit = display ? 1u : (size_t)(bits / 8), out_total = (size_t)n * channels * frame_stride * unit;
    void *d_win_out = to_host ? nullptr : const_cast<void *>(out.p);
    int rc = batch_open(r, d, n, data, offsets, lens, full_stride, frame_stride, "batch of %zu stream bytes: 32-bit offsets only");
    if (rc != ICER_RESULT_OK) return rc;
    r.windows = windows;
    rc = batch_packets(r, data, data_on_device);
    if (rc == ICER_RESULT_OK) rc = batch_plans(r, rcs, ws, hs);
    for (int k = 0; k < n && rc == ICER_RESULT_OK; k++) {
        const WinGeom &g = r.plans[k].win;
        uint32_t *o = info + (size_t)k * kWinInfo;
        o[0] = g.x0; o[1] = g.y0; o[2] = g.ww; o[3] = g.wh;
        o[4] = r.frames[k].w ? (uint32_t)r.plans[k].chains.size() : 0u; o[5] = r.plans[k].chains_full;
    }
    if (rc == ICER_RESULT_OK && r.planes_total() && out_total) {
        rc = batch_chains(r, {BatchOut::kHostPlanes, nullptr});            // (the working planes: the decoder's own buffer)
        if (rc == ICER_RESULT_OK) {
            std::vector<WinGeom> geoms((size_t)n);
            size_t span = 1;
            for (int k = 0; k < n; k++) {
                const WinGeom &g = geoms[k] = r.plans[k].win;
                const WinLevel &L = g.lv[0];
                const size_t fine = (size_t)(L.x.lo1 - L.x.lo0 + L.x.hi1 - L.x.hi0) * (L.y.lo1 - L.y.lo0 + L.y.hi1 - L.y.hi0);
                span = std::max(span, g.active ? std::max(fine, (size_t)g.ww * g.wh) : (size_t)r.frames[k].w * r.frames[k].h);
            }
            const size_t pos_bytes = sizeof(uint32_t) * (size_t)n * win_pos_words(bits, full_stride);
            HIP_TRY(ensure(d->win, sizeof(WinGeom) * (size_t)n));
            HIP_TRY(hipMemcpy(d->win.p, geoms.data(), sizeof(WinGeom) * (size_t)n, hipMemcpyHostToDevice));
            HIP_TRY(ensure(d->tmp, sizeof(uint16_t) * r.planes_total()));
            HIP_TRY(ensure(d->pos, std::max<size_t>(pos_bytes, 4)));
            if (to_host) { HIP_TRY(ensure(d->wout, out_total)); d_win_out = d->wout.p; }
            rc = enqueue_window_samples(d, n, r.d_planes, (int16_t *)d->tmp.p, full_stride, r.d_frames, (const WinGeom *)d->win.p,
                                        (uint32_t *)d->pos.p, (const ChainDesc *)d->chains.p, (uint32_t)r.chains.size(), d->recon, d_win_out,
                                        frame_stride, display, span, (hipStream_t)0);
            if (rc != ICER_RESULT_OK) goto done;
            HIP_TRY(hipDeviceSynchronize());
            if (to_host)
                rc = rows_to_host(out, n, channels, d_win_out, frame_stride, unit, [&](int k) { return geoms[k].skip ? (size_t)0 : (size_t)geoms[k].ww * geoms[k].wh; });
        }
    }
done:
    if (rc != ICER_RESULT_OK) drain_after_error(d);
    return rc;
}

}  // namespace
