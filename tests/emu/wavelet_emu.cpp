// CPU build of the standalone wavelet transform's line bodies (icer_compression_amd/csrc/wavelet_core.hpp), driven in
// the same passes the GPU line kernels run: forward = rows (region -> scratch) then columns (scratch -> region), inverse =
// columns then rows.  Compiled by tests/test_wavelet_emu.py itself.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../icer_compression_amd/csrc/wavelet_core.hpp"
#include "../../icer_compression_amd/csrc/wavelet_inv.hpp"
#include "../../icer_compression_amd/csrc/dwt_tile.hpp"

using namespace icer;

namespace {

template <class T>
bool lines(bool inv, const T *src, T *dst, uint32_t n_lines, uint32_t n, size_t line_step, size_t elem_step, FilterTaps f)
{
    std::vector<uint32_t> pos, tmp;
    const uint32_t *p = nullptr;
    if (inv && sizeof(T) == 1 && (n & 1u)) {
        pos.resize(n); tmp.resize(n);
        wl_interleave_positions_u8(n, tmp.data(), pos.data());
        p = pos.data();
    }
    bool ovf = false;
    for (uint32_t l = 0; l < n_lines; l++) {
        const T *s = src + l * line_step;
        T *d = dst + l * line_step;
        ovf |= inv ? wl_inv_line<T>(s, d, n, elem_step, f, p) : wl_fwd_line<T>(s, d, n, elem_step, f);
    }
    return ovf;
}

// one level on the w x h region of a plane of row stride W (scratch: same layout)
template <class T>
bool level(bool inv, T *plane, T *scratch, size_t w, size_t h, size_t W, FilterTaps f)
{
    if (!inv) {
        const bool o = lines<T>(false, plane, scratch, (uint32_t)h, (uint32_t)w, W, 1, f);
        return lines<T>(false, scratch, plane, (uint32_t)w, (uint32_t)h, 1, W, f) || o;
    }
    const bool o = lines<T>(true, plane, scratch, (uint32_t)w, (uint32_t)h, 1, W, f);
    return lines<T>(true, scratch, plane, (uint32_t)h, (uint32_t)w, W, 1, f) || o;
}

template <class T>
int run(int mode, bool inv, void *data, size_t w, size_t h, size_t stride, int stages, int filt)
{
    const int chk = wl_check(mode, w, h, stages);
    if (chk) return chk;
    const FilterTaps f = filter_taps(filt);
    T *p = (T *)data;
    bool ovf = false;
    if (mode == kWl1d) {
        std::vector<T> a(w), b(w);
        for (size_t i = 0; i < w; i++) a[i] = p[i * stride];
        ovf = lines<T>(inv, a.data(), b.data(), 1, (uint32_t)w, 0, 1, f);
        for (size_t i = 0; i < w; i++) p[i * stride] = b[i];
    } else if (mode == kWl2d) {
        std::vector<T> s(h * stride);
        ovf = level<T>(inv, p, s.data(), w, h, stride, f);
    } else {
        std::vector<T> s(h * w);
        for (int it = 0; it < stages; it++) {
            const int lv = inv ? stages - 1 - it : it;
            ovf |= level<T>(inv, p, s.data(), wl_low_dim(w, lv), wl_low_dim(h, lv), w, f);
        }
    }
    return ovf ? -1 : 0;
}


// ---- the filter-A tile pass's phase functions (wavelet_inv.hpp), run the way wavelet_inv.hip launches them
template <class T>
bool ia_level(const T *src, T *dst, size_t W, size_t cw, size_t ch, FilterTaps f)
{
    static IaShared sh;
    IaArgs a;
    a.src = src; a.dst = dst; a.w = (uint32_t)W; a.cw = (uint32_t)cw; a.ch = (uint32_t)ch; a.f = f;
    bool ovf = false;
    for (size_t ty = 0; ty < ((ch + 1) / 2 + kIaPY - 1) / kIaPY; ty++)
        for (size_t tx = 0; tx < ((cw + 1) / 2 + kIaPX - 1) / kIaPX; tx++) {
            for (int t = 0; t < kIaThreads; t++) ia_load<T>(sh, a, (int)tx, (int)ty, t);
            for (int t = 0; t < kIaThreads; t++) ovf |= ia_cols<T>(sh, a, (int)ty, t);
            for (int t = 0; t < kIaThreads; t++) ovf |= ia_rows<T>(sh, a, (int)tx, (int)ty, t);
        }
    return ovf;
}

// inverse_lines of wavelet_inv.hip on one contiguous plane of w x h (mode stages or 2-D)
template <class T>
int run_kernels(int mode, void *data, size_t w, size_t h, int stages, int filt)
{
    const int chk = wl_check(mode, w, h, stages);
    if (chk) return chk;
    const FilterTaps f = filter_taps(filt);
    const int levels = mode == kWlStages ? stages : 1;
    T *p = (T *)data;
    std::vector<T> tmp(w * h);
    bool ovf = false;
    bool tiled = f.am1 == 0 && f.be == 0;
    for (int lv = 0; lv < levels && tiled; lv++) {
        const size_t cw = wl_low_dim(w, lv), ch = wl_low_dim(h, lv);
        tiled = cw >= 5 && ch >= 5 && (sizeof(T) == 2 || ((cw | ch) & 1) == 0);
    }
    if (tiled) {
        memcpy(tmp.data(), p, w * h * sizeof(T));
        for (int it = 0; it < levels; it++) {
            const int lv = levels - 1 - it;
            const bool to_plane = (lv & 1) == 0;
            ovf |= ia_level<T>(to_plane ? tmp.data() : p, to_plane ? p : tmp.data(), w, wl_low_dim(w, lv), wl_low_dim(h, lv), f);
        }
        return ovf ? -1 : 0;
    }
    for (int it = 0; it < levels; it++) {
        const int lv = levels - 1 - it;
        ovf |= level<T>(true, p, tmp.data(), wl_low_dim(w, lv), wl_low_dim(h, lv), w, f);
    }
    return ovf ? -1 : 0;
}
}  // namespace

extern "C" {
// mode: 0 = stages, 1 = 2-D (stride = rowstride), 2 = 1-D (w = N, stride in samples); bits 16 or 8
int wl_emu(int mode, int inverse, int bits, void *data, size_t w, size_t h, size_t stride, int stages, int filt)
{
    return bits == 8 ? run<int8_t>(mode, inverse != 0, data, w, h, stride, stages, filt)
                     : run<int16_t>(mode, inverse != 0, data, w, h, stride, stages, filt);
}

// the inverse through the kernels' phase functions: one contiguous w x h plane, mode 0 (stages) or 1 (2-D, one level)
int wl_emu_inv_kernels(int mode, int bits, void *data, size_t w, size_t h, int stages, int filt)
{
    return bits == 8 ? run_kernels<int8_t>(mode, data, w, h, stages, filt) : run_kernels<int16_t>(mode, data, w, h, stages, filt);
}

// one forward stage of the encoder's tile pass (dwt_tile.hpp, generic phases) with the uint8 twins' limit (lim = 127) and
// plain stores, on int8 samples widened to int16 -- to see whether the uint8 forward could run on it.  Result narrowed to
// int8 in `out`; returns the tile pass's overflow flag.
int wl_emu_tile_u8_stage(const int8_t *img, int8_t *out, int w, int h, int filt)
{
    std::vector<int16_t> src(img, img + (size_t)w * h), coef((size_t)w * h);
    DwtStageArgs a;
    a.src = src.data(); a.src_stride = (uint32_t)w; a.cw = w; a.ch = h;
    a.coef = coef.data(); a.coef_stride = (uint32_t)w; a.ll = coef.data(); a.ll_stride = (uint32_t)w;
    a.f = filter_taps(filt); a.lim = 127; a.sm = 0;
    static DwtTileShared sh;
    bool ovf = false;
    for (int ty = 0; ty < ((h + 1) / 2 + kTileKY - 1) / kTileKY; ty++)
        for (int tx = 0; tx < ((w + 1) / 2 + kTileKX - 1) / kTileKX; tx++) {
            for (int t = 0; t < kTileThreads; t++) dwt_tile_load(sh, a, tx, ty, t);
            for (int t = 0; t < kTileThreads; t++) ovf |= dwt_tile_rows_step1(sh, a, tx, ty, t);
            for (int t = 0; t < kTileThreads; t++) ovf |= dwt_tile_rows_step2(sh, a, tx, ty, t);
            for (int t = 0; t < kTileThreads; t++) ovf |= dwt_tile_cols_step1(sh, a, tx, ty, t);
            for (int t = 0; t < kTileThreads; t++) ovf |= dwt_tile_cols_step2(sh, a, tx, ty, t);
        }
    for (size_t i = 0; i < coef.size(); i++) out[i] = (int8_t)coef[i];
    return ovf ? -1 : 0;
}
}
