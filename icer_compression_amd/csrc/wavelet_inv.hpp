// wavelet_inv.hpp -- the filter-A inverse of the standalone wavelet transform as per-thread phase functions (the GPU
// kernel in wavelet_inv.hip calls them between barriers; tests/emu/wavelet_emu.cpp runs them in thread loops on the CPU).
// It needs lines of >= 5 samples (shorter lines read past the lows, wl_inv_line handles those).
//
// Filter A (alpha_-1 = 0, beta = 0): every output pair depends on stored values only.  One LDS-tiled pass per level,
// mirroring dwt_tile.hpp: a workgroup owns kIaTileX x kIaTileY output samples, loads the four bands' windows it needs
// (the stored lows one pair beyond each side), restores the columns inside LDS, then the rows, and writes its samples.
// It reads `src` and writes `dst` (two buffers: a tile's window overlaps other tiles' outputs).
//
// Filters B..F and Q keep wl_inv_line (wavelet_core.hpp): one lane per line with the stored values of 32 steps
// loaded ahead of the chain (profiles/wavelet_4096.md has the LDS-staged variant that measured slower).
#pragma once
#include "wavelet_core.hpp"

namespace icer {
namespace {

// ------------------------------------------------------------------------------------------ filter A, tiled
constexpr int kIaPX = 32, kIaPY = 8;                              // output pairs per tile (x, y)
constexpr int kIaTileX = 2 * kIaPX, kIaTileY = 2 * kIaPY;          // output samples per tile
constexpr int kIaCols = 2 * kIaPX + 2;                            // columns the tile restores: KX + 2 low, KX high
constexpr int kIaThreads = 256;

struct IaShared {
    int16_t lo[kIaPY + 2][kIaCols];                               // stored lows of the columns (pair rows qy0-1 .. qy0+KY)
    int16_t hi[kIaPY][kIaCols];                                   // stored highs of the columns
    int16_t mid[kIaTileY][kIaCols];                               // the columns restored: rows of the tile
};

struct IaArgs {
    const void *src;                                              // T samples, row stride w
    void *dst;
    uint32_t w, cw, ch;                                           // row stride, level region
    FilterTaps f;
};

// window column c -> region column (the low columns kx0-1 .. kx0+KX, then the high columns kx0 .. kx0+KX-1; clamped:
// a clamped column is a duplicate nobody reads)
WL_HD uint32_t ia_col(int c, int kx0, uint32_t nl, uint32_t nh)
{
    if (c < kIaPX + 2) { int j = kx0 - 1 + c; j = j < 0 ? 0 : (j > (int)nl - 1 ? (int)nl - 1 : j); return (uint32_t)j; }
    int k = kx0 + c - (kIaPX + 2);
    k = k > (int)nh - 1 ? (int)nh - 1 : k;
    return nl + (uint32_t)k;
}

// restoration of pair k of a filter-A line from stored lows l(k-1), l(k), l(k+1) and high h (icer_wavelet.c:484-545)
template <class T>
WL_HD void ia_pair(int32_t lm, int32_t l0, int32_t lp, int32_t h, uint32_t k, uint32_t nh, bool odd, const FilterTaps &f, int32_t *s0,
                   int32_t *s1, bool *ovf)
{
    int32_t add;
    if (k == 0) add = wl_r<T>(l0, lp) >> 2;
    else if (!odd && k == nh - 1u) add = wl_r<T>(lm, l0) >> 2;
    else add = (f.a0 * wl_r<T>(lm, l0) + f.a1 * wl_r<T>(l0, lp) + 8) >> 4;
    const int32_t d = h + add;
    *ovf |= wl_out<T>(d);
    const int32_t hi = (T)d;
    const int32_t tmp = l0 + ((hi + 1) >> 1);
    *ovf |= wl_out<T>(tmp) || wl_out<T>(tmp - hi);
    *s0 = (T)tmp;
    *s1 = (T)(tmp - hi);
}

// phase 1, thread t: the windows of the four bands into LDS
template <class T>
WL_HD void ia_load(IaShared &sh, const IaArgs &a, int tx, int ty, int t)
{
    const uint32_t nlw = (a.cw + 1) / 2, nhw = a.cw / 2, nlh = (a.ch + 1) / 2, nhh = a.ch / 2;
    const int kx0 = tx * kIaPX, qy0 = ty * kIaPY;
    const T *s = (const T *)a.src;
    for (int i = t; i < (2 * kIaPY + 2) * kIaCols; i += kIaThreads) {
        const int r = i / kIaCols, c = i - r * kIaCols;
        const uint32_t gx = ia_col(c, kx0, nlw, nhw);
        if (r < kIaPY + 2) {
            int q = qy0 - 1 + r;
            q = q < 0 ? 0 : (q > (int)nlh - 1 ? (int)nlh - 1 : q);
            sh.lo[r][c] = s[(size_t)q * a.w + gx];
        } else {
            int q = qy0 + r - (kIaPY + 2);
            q = q > (int)nhh - 1 ? (int)nhh - 1 : q;
            sh.hi[r - (kIaPY + 2)][c] = s[(size_t)(nlh + (uint32_t)q) * a.w + gx];
        }
    }
}

// phase 2, thread t: the columns restored into mid (the tile's rows); returns the overflow flag
template <class T>
WL_HD bool ia_cols(IaShared &sh, const IaArgs &a, int ty, int t)
{
    const uint32_t nlh = (a.ch + 1) / 2, nhh = a.ch / 2;
    const bool odd = (a.ch & 1u) != 0;
    const int qy0 = ty * kIaPY;
    bool ovf = false;
    for (int i = t; i < kIaPY * kIaCols; i += kIaThreads) {
        const int qq = i / kIaCols, c = i - qq * kIaCols;
        const uint32_t q = (uint32_t)(qy0 + qq);
        if (q < nhh) {
            int32_t s0, s1;
            ia_pair<T>(sh.lo[qq][c], sh.lo[qq + 1][c], sh.lo[qq + 2][c], sh.hi[qq][c], q, nhh, odd, a.f, &s0, &s1, &ovf);
            sh.mid[2 * qq][c] = (int16_t)s0;
            sh.mid[2 * qq + 1][c] = (int16_t)s1;
        } else if (q < nlh) sh.mid[2 * qq][c] = sh.lo[qq + 1][c];         // odd height: the last low
    }
    return ovf;
}

// phase 3, thread t: the rows restored and stored (consecutive threads: consecutive pairs of a row)
template <class T>
WL_HD bool ia_rows(IaShared &sh, const IaArgs &a, int tx, int ty, int t)
{
    const uint32_t nlw = (a.cw + 1) / 2, nhw = a.cw / 2;
    const bool odd = (a.cw & 1u) != 0;
    const int kx0 = tx * kIaPX, y0 = ty * kIaTileY;
    T *d = (T *)a.dst;
    bool ovf = false;
    for (int i = t; i < kIaTileY * kIaPX; i += kIaThreads) {
        const int r = i / kIaPX, kk = i - r * kIaPX;
        const uint32_t y = (uint32_t)(y0 + r), k = (uint32_t)(kx0 + kk);
        if (y >= a.ch) continue;
        const int16_t *m = sh.mid[r];
        if (k < nhw) {
            int32_t s0, s1;
            ia_pair<T>(m[kk], m[kk + 1], m[kk + 2], m[kIaPX + 2 + kk], k, nhw, odd, a.f, &s0, &s1, &ovf);
            d[(size_t)y * a.w + 2 * k] = (T)s0;
            d[(size_t)y * a.w + 2 * k + 1] = (T)s1;
        } else if (k < nlw) d[(size_t)y * a.w + 2 * k] = (T)m[kk + 1];   // odd width: the last low
    }
    return ovf;
}

}  // namespace
}  // namespace icer
