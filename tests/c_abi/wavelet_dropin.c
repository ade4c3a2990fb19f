/* The standalone wavelet calls of lib_icer, written against the product headers and linked with libicer_hip.so and
 * libicer_hip_dec.so (tests/test_gpu_wavelet.py builds and runs it and compares its output with the reference's).
 *
 *   wavelet_dropin <in> <out>
 * <in>:  a 61 x 37 uint16 image, then a 61 x 37 uint8 image.  <out>: for every filter, the return code (int32) and the
 * buffer after each step of the sequence below. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "icer_hip_dec.h"

#define W 61
#define H 37

static void put(FILE *f, int rc, const void *buf, size_t bytes)
{
    fwrite(&rc, sizeof rc, 1, f);
    fwrite(buf, 1, bytes, f);
}

int main(int argc, char **argv)
{
    static uint16_t img16[W * H], a16[W * H];
    static uint8_t img8[W * H], a8[W * H];
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    if (fread(img16, 2, W * H, in) != W * H || fread(img8, 1, W * H, in) != W * H) return 4;
    for (int filt = 0; filt <= ICER_FILTER_Q; filt++) {
        const enum icer_filter_types f = (enum icer_filter_types)filt;
        memcpy(a16, img16, sizeof a16);
        put(out, icer_wavelet_transform_stages_uint16(a16, W, H, 3, f), a16, sizeof a16);
        put(out, icer_inverse_wavelet_transform_stages_uint16(a16, W, H, 3, f), a16, sizeof a16);
        put(out, icer_wavelet_transform_2d_uint16(a16, W - 4, H, W, f), a16, sizeof a16);
        put(out, icer_inverse_wavelet_transform_1d_uint16(a16 + 1, H - 2, W, f), a16, sizeof a16);
        icer_to_sign_magnitude_int16(a16, W * H);
        put(out, 0, a16, sizeof a16);
        icer_from_sign_magnitude_int16(a16, W * H);
        put(out, 0, a16, sizeof a16);
        memcpy(a8, img8, sizeof a8);
        put(out, icer_wavelet_transform_stages_uint8(a8, W, H, 2, f), a8, sizeof a8);
        put(out, icer_inverse_wavelet_transform_stages_uint8(a8, W, H, 2, f), a8, sizeof a8);
        put(out, icer_wavelet_transform_1d_uint8(a8 + 3, W - 6, 1, f), a8, sizeof a8);
        put(out, icer_inverse_wavelet_transform_2d_uint8(a8, W, H - 1, W, f), a8, sizeof a8);
        icer_to_sign_magnitude_int8(a8, W * H);
        put(out, 0, a8, sizeof a8);
        icer_from_sign_magnitude_int8(a8, W * H);
        put(out, 0, a8, sizeof a8);
    }
    put(out, icer_wavelet_transform_stages_uint16(img16, W, H, 5, ICER_FILTER_A), img16, sizeof img16);   /* too many stages */
    fclose(out);
    fclose(in);
    return 0;
}
