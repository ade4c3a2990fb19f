// display_main.cpp -- TEST ONLY.  A stand-alone program for the decoder's display entry points (include/icer_hip_dec.h)
// on the CPU mock runtime: built by tests/test_display_mock.py as ONE executable with decoder.hip,
//     g++ -x c++ -fsanitize=address,undefined -DICER_HOST_MOCK -DICER_WAVE_EMU -include tests/emu/hip_mock_async.h
//         icer_compression_amd/csrc/decoder.hip tests/emu/display_main.cpp
// so that AddressSanitizer and UBSan see every access of the host pipeline and of the kernels.  Every buffer handed to the
// library is allocated at exactly its contractual size.
//
//     display_main <case file>
// case file (little endian, written by the test): int32 channels, bits, stages, filt, segments, n, stride; n x { uint32 len,
// bytes }; n x { int32 rc, uint32 w, uint32 h, uint32 image bytes, bytes } -- the expected results.
// Runs the batch through icerx_decode_device_display, icerx_decode_device_display_async and icerx_decode_device +
// icerx_planes_to_display_device and compares each with the expectation.  Exit code 0: all equal.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/icer_hip_dec.h"

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Want { int32_t rc; uint32_t w, h; std::vector<uint8_t> image; };

static int compare(const char *what, const std::vector<Want> &want, const int32_t *rcs, const uint64_t *ws, const uint64_t *hs,
                   const uint8_t *out, size_t row_bytes, uint8_t junk)
{
    for (size_t k = 0; k < want.size(); k++) {
        if (rcs && (rcs[k] != want[k].rc || ws[k] != want[k].w || hs[k] != want[k].h)) { fprintf(stderr, "%s: frame %zu rc / size\n", what, k); return 1; }
        const uint8_t *row = out + k * row_bytes;
        if (!want[k].image.empty() && memcmp(row, want[k].image.data(), want[k].image.size()) != 0) { fprintf(stderr, "%s: frame %zu image\n", what, k); return 1; }
        for (size_t i = want[k].image.size(); i < row_bytes; i++)
            if (row[i] != junk) { fprintf(stderr, "%s: frame %zu byte %zu behind the image written\n", what, k, i); return 1; }
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[7];
    if (!rd(f, hdr, sizeof hdr)) return 2;
    const int channels = hdr[0], bits = hdr[1], stages = hdr[2], filt = hdr[3], segments = hdr[4], n = hdr[5];
    const size_t stride = (size_t)hdr[6];
    std::vector<uint8_t> blob;
    std::vector<size_t> offs((size_t)n), lens((size_t)n);
    for (int k = 0; k < n; k++) {
        uint32_t len;
        if (!rd(f, &len, 4)) return 2;
        offs[k] = blob.size(); lens[k] = len;
        blob.resize(blob.size() + len);
        if (!rd(f, blob.data() + offs[k], len)) return 2;
    }
    std::vector<Want> want((size_t)n);
    for (int k = 0; k < n; k++) {
        uint32_t v[4];
        if (!rd(f, v, sizeof v)) return 2;
        want[k].rc = (int32_t)v[0]; want[k].w = v[1]; want[k].h = v[2];
        want[k].image.resize(v[3]);
        if (!rd(f, want[k].image.data(), v[3])) return 2;
    }
    fclose(f);

    icerx_decoder *dec = nullptr;
    if (icerx_decoder_create(&dec, -1, channels, stages, filt, (unsigned)segments, bits) != ICER_RESULT_OK) return 3;
    const size_t row_bytes = (size_t)channels * stride, out_bytes = (size_t)n * row_bytes;
    const uint8_t junk = 0xA5;
    // (exact sizes: the blob without slack, the images without a guard -- the sanitizer is the guard)
    uint8_t *data = (uint8_t *)malloc(blob.size() ? blob.size() : 1);
    memcpy(data, blob.data(), blob.size());
    int bad = 0;

    {   // synchronous
        uint8_t *out = (uint8_t *)malloc(out_bytes);
        memset(out, junk, out_bytes);
        std::vector<int> rcs((size_t)n);
        std::vector<size_t> ws((size_t)n, 0), hs((size_t)n, 0);
        if (icerx_decode_device_display(dec, n, data, offs.data(), lens.data(), out, stride, rcs.data(), ws.data(), hs.data()) != ICER_RESULT_OK) return 4;
        std::vector<int32_t> r32(rcs.begin(), rcs.end());
        std::vector<uint64_t> w64(ws.begin(), ws.end()), h64(hs.begin(), hs.end());
        bad |= compare("sync", want, r32.data(), w64.data(), h64.data(), out, row_bytes, junk);
        free(out);
    }
    {   // asynchronous: the workspace at exactly the size asked for
        uint8_t *out = (uint8_t *)malloc(out_bytes);
        memset(out, junk, out_bytes);
        std::vector<uint64_t> o64(offs.begin(), offs.end()), l64(lens.begin(), lens.end()), ws((size_t)n, 0), hs((size_t)n, 0);
        std::vector<int32_t> rcs((size_t)n, 77);
        const size_t need = icerx_decode_display_workspace_bytes(dec, n, blob.size(), stride);
        void *work = malloc(need);
        memset(work, 0xCD, need);
        if (icerx_decode_device_display_async(dec, n, data, blob.size(), o64.data(), 0, l64.data(), out, stride, rcs.data(), ws.data(),
                                              hs.data(), work, need, nullptr) != ICER_RESULT_OK) return 5;
        bad |= compare("async", want, rcs.data(), ws.data(), hs.data(), out, row_bytes, junk);
        if (icerx_decode_device_display_async(dec, n, data, blob.size(), o64.data(), 0, l64.data(), out, stride, rcs.data(), ws.data(),
                                              hs.data(), work, need - 1, nullptr) != ICER_INVALID_INPUT) { fprintf(stderr, "workspace one byte short accepted\n"); bad = 1; }
        free(work);
        free(out);
    }
    {   // the plain decode, then the conversion alone on each frame's delivered samples
        const size_t sample = bits == 16 ? 2 : 1;
        uint8_t *planes = (uint8_t *)malloc(out_bytes * sample);
        std::vector<int> rcs((size_t)n);
        std::vector<size_t> ws((size_t)n, 0), hs((size_t)n, 0);
        if (icerx_decode_device(dec, n, data, offs.data(), lens.data(), planes, stride, rcs.data(), ws.data(), hs.data()) != ICER_RESULT_OK) return 6;
        uint8_t *out = (uint8_t *)malloc(out_bytes);
        memset(out, junk, out_bytes);
        for (int k = 0; k < n; k++) {
            if (want[k].image.empty()) continue;
            if (icerx_planes_to_display_device(planes + (size_t)k * row_bytes * sample, 1, channels, ws[k], hs[k], stride, bits,
                                               out + (size_t)k * row_bytes, stride, nullptr) != ICER_RESULT_OK) return 7;
        }
        bad |= compare("planes", want, nullptr, nullptr, nullptr, out, row_bytes, junk);
        free(out);
        free(planes);
    }
    free(data);
    icerx_decoder_destroy(dec);
    if (!bad) printf("display_main: %d frames, sync / async / planes equal the expectation\n", n);
    return bad;
}
