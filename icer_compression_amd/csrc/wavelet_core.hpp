// wavelet_core.hpp -- per-line bodies of the standalone wavelet transform (icer_wavelet_transform_* and
// icer_inverse_wavelet_transform_*, lib_icer/src/icer_wavelet.c), shared by the forward path of libicer_hip.so
// (wavelet_fwd.hip), the inverse of libicer_hip_dec.so (wavelet_inv.hip) and the tests-only CPU build
// (tests/emu/wavelet_emu.cpp, tests/test_wavelet_emu.py holds them to the reference).
//
// A line is `n` samples `stride` apart.  T = int16_t for the uint16 functions, int8_t for the uint8 twins: every store
// truncates to T exactly as the reference's in-place stores do, and the overflow flag is raised on the untruncated
// value at the reference's checks (icer_wavelet.c:243/:412, :291/:460, :343/:512, :360/:529).
//
//   wl_fwd_line   forward lifting of one line: src (the samples) -> dst ([lows | highs], the reference's deinterleaved
//                 layout).  Step 1 writes the pair averages and differences, step 2 replaces the differences by the
//                 highs in increasing order, reading dst with the reference's raw indices -- so the short-line cases
//                 where an index runs past the lows (n = 2, and n = 4 with filter C) read what the reference reads.
//   wl_inv_line   inverse lifting of one line: src ([lows | highs]) -> dst (the samples).  The only serial term is
//                 beta * d[k+1] (the restored high above); the lows around k are stored values, so the line is walked
//                 backwards with a window of four lows carried in registers, and the stored highs and lows of 32 steps
//                 are loaded together ahead of the chain (none of them depends on it).  Output positions: the plain interleave, or `pos_of` (the
//                 uint8 routine's odd-length scramble, wl_interleave_positions).
// n >= 2 (n < 2 is rejected by the callers: the reference loops through SIZE_MAX there).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WL_HD __host__ __device__ __forceinline__
#else
#define WL_HD static inline
#endif
#include "icer_tables.hpp"

#if defined(__HIPCC__)
#define WL_UNROLL _Pragma("unroll")
#else
#define WL_UNROLL
#endif

namespace icer {
namespace {              // (internal linkage: both libraries compile these bodies)

constexpr uint32_t kWlChunk = 32;             // steps of the inverse chain whose loads are issued together

template <class T> struct WlLimits;
template <> struct WlLimits<int16_t> { static constexpr int32_t lo = -32768, hi = 32767; static constexpr int bits = 16; };
template <> struct WlLimits<int8_t> { static constexpr int32_t lo = -128, hi = 127; static constexpr int bits = 8; };

template <class T> WL_HD bool wl_out(int32_t v) { return v < WlLimits<T>::lo || v > WlLimits<T>::hi; }

// get_r (icer_wavelet.c:196-208): the int16 routine wraps the difference to int16, the int8 one does not need to
template <class T> WL_HD int32_t wl_r(int32_t a, int32_t b) { return WlLimits<T>::bits == 16 ? (int32_t)(int16_t)(a - b) : a - b; }

// floor division by 2, 4, 8 or 16 (icer_floor_div_int16 / _int32) is an arithmetic shift
template <class T>
WL_HD bool wl_fwd_line(const T *__restrict__ src, T *__restrict__ dst, uint32_t n, size_t stride, FilterTaps f)
{
    const uint32_t nl = (n + 1u) / 2u, nh = n / 2u;
    const bool odd = (n & 1u) != 0;
    bool ovf = false;
    for (uint32_t k = 0; k < nh; k++) {                                       // :402-426
        const int32_t a = src[(size_t)(2u * k) * stride], b = src[(size_t)(2u * k + 1u) * stride];
        const int32_t lo = (a + b) >> 1, d = a - b;
        ovf |= wl_out<T>(lo) || wl_out<T>(d);
        dst[(size_t)k * stride] = (T)lo;
        dst[(size_t)(nl + k) * stride] = (T)d;
    }
    if (odd) dst[(size_t)(nl - 1u) * stride] = src[(size_t)(n - 1u) * stride];
#define W(j) ((int32_t)dst[(size_t)(j) * stride])
#define R(j) wl_r<T>(W((j) - 1u), W(j))
    for (uint32_t k = 0; k < nh; k++) {                                       // :430-462
        int32_t sub;
        if (k == 0) sub = R(1u) >> 2;
        else if (k == 1 && f.am1 != 0) {
            const int32_t x = (odd && nl == 3u) ? 0 : W(nl + 1u);            // get_d(2) with offset low_N
            sub = (2 * R(1u) + 3 * R(2u) - 2 * x + 4) >> 3;
        } else if (!odd && k == nh - 1u) sub = R(nh - 1u) >> 2;
        else {
            const int32_t rm = k >= 2u ? R(k - 1u) : 1;
            const int32_t dn = (odd && k + 1u == nl - 1u) ? 0 : W(nl + k + 1u);
            sub = (f.am1 * rm + f.a0 * R(k) + f.a1 * R(k + 1u) - f.be * dn + 8) >> 4;
        }
        const int32_t h = W(nl + k) - sub;
        ovf |= wl_out<T>(h);
        dst[(size_t)(nl + k) * stride] = (T)h;
    }
#undef W
#undef R
    return ovf;
}

WL_HD uint32_t wl_plain_pos(uint32_t i, uint32_t nl) { return i < nl ? 2u * i : 2u * (i - nl) + 1u; }

template <class T>
WL_HD bool wl_inv_line(const T *__restrict__ src, T *__restrict__ dst, uint32_t n, size_t stride, FilterTaps f,
                       const uint32_t *__restrict__ pos_of)
{
    const uint32_t nl = (n + 1u) / 2u, nh = n / 2u;
    const bool odd = (n & 1u) != 0;
#define LO(j) ((int32_t)src[(size_t)(j) * stride])
#define POS(i) (pos_of ? pos_of[i] : wl_plain_pos((i), nl))
    bool ovf = false;
    // window of stored values at raw indices k-2 .. k+1 (index nh < n always; for n = 2 it is the stored high 0,
    // which is what the reference reads there)
    int32_t e = LO(nh), c = LO(nh - 1u);
    int32_t b = nh >= 2u ? LO(nh - 2u) : 0, a = nh >= 3u ? LO(nh - 3u) : 0;
    int32_t next = 0;                                                         // restored high k + 1
    // one step of the chain (:484-545) from the stored high k and the window; `lnew` = stored low k - 3
    auto step = [&](uint32_t k, int32_t hk, int32_t lnew) {
        int32_t add;
        if (k == 0) add = wl_r<T>(c, e) >> 2;
        else if (k == 1 && f.am1 != 0) {
            const int32_t x = (odd && nl == 3u) ? 0 : hk;                     // high 1 itself, still unrestored
            add = (2 * wl_r<T>(b, c) + 3 * wl_r<T>(c, e) - 2 * x + 4) >> 3;
        } else if (!odd && k == nh - 1u) add = wl_r<T>(b, c) >> 2;
        else {
            const int32_t rm = k >= 2u ? wl_r<T>(a, b) : 1;
            const int32_t dn = (odd && k + 1u == nl - 1u) ? 0 : next;
            add = (f.am1 * rm + f.a0 * wl_r<T>(b, c) + f.a1 * wl_r<T>(c, e) - f.be * dn + 8) >> 4;
        }
        const int32_t d = hk + add;
        ovf |= wl_out<T>(d);
        const int32_t hi = (T)d;
        next = hi;
        const int32_t tmp = c + ((hi + 1) >> 1);
        ovf |= wl_out<T>(tmp) || wl_out<T>(tmp - hi);
        dst[(size_t)POS(k) * stride] = (T)tmp;
        dst[(size_t)POS(nl + k) * stride] = (T)(tmp - hi);
        e = c; c = b; b = a; a = lnew;
    };
    // the line is walked backwards in chunks of kWlChunk steps: the chunk's stored highs and lows are loaded together
    // (none depends on the chain), so the chain waits on one memory round trip per chunk instead of one per step
    uint32_t k = nh;
    for (; k >= kWlChunk; k -= kWlChunk) {
        int32_t hv[kWlChunk], lv[kWlChunk];
        WL_UNROLL
        for (uint32_t i = 0; i < kWlChunk; i++) {
            const uint32_t kk = k - 1u - i;
            hv[i] = LO(nl + kk);
            lv[i] = kk >= 3u ? LO(kk - 3u) : 0;
        }
        WL_UNROLL
        for (uint32_t i = 0; i < kWlChunk; i++) step(k - 1u - i, hv[i], lv[i]);
    }
    for (; k > 0; k--) step(k - 1u, LO(nl + k - 1u), k - 1u >= 3u ? LO(k - 4u) : 0);
    if (odd) dst[(size_t)POS(nl - 1u) * stride] = src[(size_t)(nl - 1u) * stride];
#undef LO
#undef POS
    return ovf;
}

// icer_find_k (icer_wavelet.c:823-847): the reference's binary search for a slice length 3^k + 1
WL_HD uint32_t wl_slice(size_t len)
{
    uint32_t lo_k = 0, hi_k = 11, res = 0;
    while (lo_k < hi_k) {
        const uint32_t mid = (hi_k + lo_k) / 2u;
        size_t s = 1;
        for (uint32_t e = 0; e < mid; e++) s *= 3u;
        s += 1u;
        if (len > s) { lo_k = mid + 1u; res = mid; }
        else if (len < s) hi_k = (mid - 1u) & 0xFFu;
        else break;
    }
    size_t s = 1;
    for (uint32_t e = 0; e < res; e++) s *= 3u;
    return (uint32_t)(s + 1u);
}

// Where value i of the [lows | highs] layout lands after icer_interleave_uint8 (icer_wavelet.c:570-628), followed on an
// index array `tmp` of `len` entries: the uint8 routine rotates with bound len/2 instead of len/2 - 1 on odd lengths and
// scrambles those lines (the uint16 routine, and both on even lengths, give the plain interleave).  One thread per table.
WL_HD void wl_interleave_positions_u8(uint32_t len, uint32_t *tmp, uint32_t *pos_of)
{
    const bool odd = (len & 1u) != 0;
    const uint32_t n = len - (odd ? 1u : 0u);
    for (uint32_t i = 0; i < len; i++) tmp[i] = i;
    if (odd) {
        const uint32_t x = tmp[n / 2u];
        for (uint32_t i = n / 2u; i < n; i++) tmp[i] = tmp[i + 1u];
        tmp[len - 1u] = x;
    }
    for (uint32_t done = 0; done < n;) {
        const uint32_t seg = wl_slice(n - done), half = seg / 2u, left = n - done, halfleft = left / 2u - (odd ? 0u : 1u);
        uint32_t lo, hi;
        lo = done + half; hi = done + halfleft + half;
        while (lo < hi) { const uint32_t x = tmp[lo]; tmp[lo] = tmp[hi]; tmp[hi] = x; lo++; hi--; }
        lo = done + half; hi = done + seg - 1u;
        while (lo < hi) { const uint32_t x = tmp[lo]; tmp[lo] = tmp[hi]; tmp[hi] = x; lo++; hi--; }
        lo = done + seg; hi = done + halfleft + half;
        while (lo < hi) { const uint32_t x = tmp[lo]; tmp[lo] = tmp[hi]; tmp[hi] = x; lo++; hi--; }
        for (uint32_t i = 1; i < seg; i *= 3u) {
            uint32_t j = i, carry = tmp[done + j];
            do {
                j = j < half ? 2u * j : (j - half) * 2u + 1u;
                const uint32_t x = tmp[done + j]; tmp[done + j] = carry; carry = x;
            } while (j != i);
        }
        done += seg;
    }
    for (uint32_t i = 0; i < len; i++) pos_of[tmp[i]] = i;
}

// ------------------------------------------------------------------------------------------ geometry
// icer_get_dim_n_low_stages (icer_wavelet.c:107-109) without the power overflow: ceil(dim / 2^s)
WL_HD size_t wl_low_dim(size_t dim, int s)
{
    for (int i = 0; i < s && dim > 1; i++) dim = (dim + 1) / 2;
    return dim;
}

// the three kinds of call behind one device path
enum WlMode : int { kWlStages = 0, kWl2d = 1, kWl1d = 2 };

// icer_status of a geometry before anything runs: stages calls need the smallest LL >= 3 on both axes (:63-68); every
// line a call transforms needs >= 2 samples (ICER_INVALID_INPUT: the reference loops through SIZE_MAX there)
WL_HD int wl_check(int mode, size_t w, size_t h, int stages)
{
    if (mode == kWl1d) return w >= 2 ? 0 : -11;
    if (mode == kWl2d) return (w >= 2 && h >= 2) ? 0 : -11;
    if (stages < 0) return -11;
    if (wl_low_dim(w, stages) < 3 || wl_low_dim(h, stages) < 3) return -4;
    return 0;
}

}  // namespace
}  // namespace icer
