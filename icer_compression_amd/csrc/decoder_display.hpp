// decoder_display.hpp -- the decoder's last pass fused with the conversion to 8-bit display images (include/icer_hip_dec.h,
// the *_display entry points): gray8 for 1-channel decoders, packed RGB888 for 3-channel ones.  Included by decoder.hip after
// its kernels (it needs FrameInfo); finish_kernel and the paths that deliver planes do not pass through here.
//
// Per pixel: the working-plane word of each channel is finished as finish_kernel finishes it (a frame that reached the
// transform: negative -> 0; a frame that stopped early: the word as it is; an 8-bit decoder: narrowed to a byte), taken as
// unsigned (uint16, or uint8 for an 8-bit decoder) and converted:
//   gray8    min(v, 255)
//   RGB888   R = clip(Y + ((91881 Cr) >> 16) - 179), G = clip(Y - ((22544 Cb + 46793 Cr) >> 16) + 135),
//            B = clip(Y + ((116129 Cb) >> 16) - 226), clip to 0..255
// -- the formulas of the reference's callers (example/inc/color_util.h CYCbCr2R/G/B, example/src/icer_util.c
// yuv_to_rgb888_packed and :321-326).  The reference evaluates them in 32-bit int, where the products overflow (undefined
// behaviour) from Cb >= 18 493 or Cr >= 23 373; here they are evaluated in 64 bits: the exact integer result for every input
// 0..65535, equal to the reference's wherever the reference's is defined.
//
// Memory bound (6 bytes read, 3 written per pixel).  A thread takes a group of 8 bytes' worth of consecutive pixels of a
// frame (4 of uint16 planes, 8 of uint8 planes): one 8-byte load per plane and whole-dword stores of the packed bytes when the
// frame's planes are 8-byte aligned and its image 4-byte aligned (a group's image bytes are a multiple of 4, so every group of
// an aligned frame is); anything else -- an unaligned base, a stride that is no multiple of the group, the tail of w * h --
// goes pixel by pixel.  Both ways go through display_pixel.
#pragma once

namespace {

// what finish_kernel leaves of a working-plane word, as unsigned (transform = false, bits = 16: the word as it is)
ICER_HD uint32_t display_finished(uint32_t word, bool transform, int bits)
{
    int16_t s = (int16_t)(uint16_t)word;
    if (transform && s < 0) s = 0;
    return bits == 8 ? (uint32_t)(uint8_t)s : (uint32_t)(uint16_t)s;
}

ICER_HD uint32_t display_clip(int64_t v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// the image bytes of one pixel from its finished values, first byte lowest: C = 1 one byte, C = 3 R, G, B
template <int C> ICER_HD uint32_t display_pixel(const uint32_t *v)
{
    if (C == 1) return v[0] > 255u ? 255u : v[0];
    const int64_t y = v[0], cb = v[1], cr = v[2];                 // (0..65535 each: the sums below stay under 2^33)
    const uint32_t r = display_clip(y + ((91881 * cr) >> 16) - 179);
    const uint32_t g = display_clip(y - ((22544 * cb + 46793 * cr) >> 16) + 135);
    const uint32_t b = display_clip(y + ((116129 * cb) >> 16) - 226);
    return r | (g << 8) | (b << 16);
}

// Group `g` of a frame of `pixels` pixels: planes[c * plane_stride + i] = sample i of channel c, out[C * i ..] = pixel i.
// `vec`: the frame's planes are 8-byte aligned and `out` is 4-byte aligned.
template <typename T, int C>
ICER_HD void display_group(const T *planes, size_t plane_stride, uint8_t *out, size_t pixels, size_t g, bool vec, bool transform, int bits)
{
    constexpr int G = 8 / (int)sizeof(T), kWords = G * C / 4;
    const size_t first = g * (size_t)G;
    if (first >= pixels) return;
    if (vec && pixels - first >= (size_t)G) {
        uint64_t in[C];
        for (int c = 0; c < C; c++)
            __builtin_memcpy(&in[c], __builtin_assume_aligned(planes + (size_t)c * plane_stride + first, 8), 8);
        uint32_t words[kWords] = {};
        for (int p = 0; p < G; p++) {
            uint32_t v[C];
            for (int c = 0; c < C; c++)
                v[c] = display_finished((uint32_t)(in[c] >> (8 * (int)sizeof(T) * p)) & (sizeof(T) == 2 ? 0xFFFFu : 0xFFu), transform, bits);
            const uint32_t px = display_pixel<C>(v);
            for (int j = 0; j < C; j++) {
                const int at = p * C + j;
                words[at >> 2] |= ((px >> (8 * j)) & 0xFFu) << (8 * (at & 3));
            }
        }
        __builtin_memcpy(__builtin_assume_aligned(out + first * (size_t)C, 4), words, sizeof words);
        return;
    }
    const size_t end = pixels - first < (size_t)G ? pixels : first + (size_t)G;
    for (size_t i = first; i < end; i++) {
        uint32_t v[C];
        for (int c = 0; c < C; c++) v[c] = display_finished(planes[(size_t)c * plane_stride + i], transform, bits);
        const uint32_t px = display_pixel<C>(v);
        for (int j = 0; j < C; j++) out[i * (size_t)C + j] = (uint8_t)(px >> (8 * j));
    }
}

template <typename T>
ICER_HD void display_frame_group(const T *planes, size_t plane_stride, int channels, uint8_t *out, size_t pixels, size_t g, bool transform, int bits)
{
    // (uniform over the frame, so over the wavefront)
    const bool vec = ((uintptr_t)planes & 7u) == 0 && ((uintptr_t)out & 3u) == 0 && (channels == 1 || (plane_stride * sizeof(T)) % 8u == 0);
    if (channels == 3) display_group<T, 3>(planes, plane_stride, out, pixels, g, vec, transform, bits);
    else display_group<T, 1>(planes, plane_stride, out, pixels, g, vec, transform, bits);
}

// the last pass of a display decode, in finish_kernel's place: frame k = blockIdx.y reads its `channels` working planes
// (planes + (k * channels + c) * frame_stride, uint16 words) and writes its image at out + k * channels * frame_stride bytes;
// a frame that does not run (w * h = 0) writes nothing.  grid = (ceil(ceil(frame_stride / 4) / 256), frames), block = 256.
__global__ void __launch_bounds__(256)
display_finish_kernel(const uint16_t *__restrict__ planes, size_t frame_stride, int channels, const FrameInfo *__restrict__ frames,
                      int bits, uint8_t *__restrict__ out)
{
    const FrameInfo f = frames[blockIdx.y];
    const size_t at = (size_t)blockIdx.y * (size_t)channels * frame_stride;
    display_frame_group<uint16_t>(planes + at, frame_stride, channels, out + at, (size_t)f.w * f.h,
                                  (size_t)blockIdx.x * blockDim.x + threadIdx.x, f.transform != 0u, bits);
}

// the conversion alone (icerx_planes_to_display_device): every frame `pixels` samples per plane, values as they are;
// sample_bytes 2: uint16 planes, 1: uint8 planes.  grid = (ceil(ceil(pixels / group) / 256), frames), block = 256.
__global__ void __launch_bounds__(256)
display_planes_kernel(const void *__restrict__ planes, size_t plane_stride, int channels, int sample_bytes, size_t pixels,
                      uint8_t *__restrict__ out, size_t frame_stride)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x, first_plane = (size_t)blockIdx.y * (size_t)channels * plane_stride;
    uint8_t *o = out + (size_t)blockIdx.y * (size_t)channels * frame_stride;
    if (sample_bytes == 2) display_frame_group<uint16_t>((const uint16_t *)planes + first_plane, plane_stride, channels, o, pixels, g, false, 16);
    else display_frame_group<uint8_t>((const uint8_t *)planes + first_plane, plane_stride, channels, o, pixels, g, false, 16);
}

constexpr unsigned kDisplayFramesPerLaunch = 32768;              // (grid.y is limited to 65535)

}  // namespace
