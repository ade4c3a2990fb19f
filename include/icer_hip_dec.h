/*
 * icer_hip_dec.h -- C ABI of libicer_hip_dec.so, the MI355X (gfx950) ICER *decoder* (SURVEY.md 8f, row next-1).
 *
 * STATUS: bit-exact against the decoder oracle in its CPU builds (tests/test_emu_decoder.py) and on an MI355X
 * (tests/test_gpu_decoder.py: gray / YUV, 16 / 8 bit, damaged and truncated streams, wrong decode parameters, the golden
 * decoder digests up to 4096 x 4096, the batch object, all three decode kernels; the reference-held fixtures and the
 * reference's own example programs linked against this library, tests/test_gpu_parity.py / test_gpu_examples.py; decoding at
 * 1/2^r resolution, tests/test_reduced_mock.py / test_gpu_reduced.py).
 * Speed (round 4, bench.py `decode` object and tools/decode_bench.py; HISTORY.md 6b (summary: DESIGN.md 8)): a chain (segment of a subband) is a serial
 * adaptive decode, one decision at a time per bit plane.  One 4096 x 4096 headline stream: 55 Mpix/s (303 ms; one wavefront per
 * bit plane with wave-uniform decisions, decoder_planes.hpp) = 14 x the reference decoder on one core of the same box; the
 * kernels around the chains (payload CRCs, inverse DWT, sample post-processing) take 0.6 ms together.  Batches (chains of all
 * streams launched longest first): 4 streams per call 220 Mpix/s, 8: 437 (eight streams in the time of one), 16: 586, 24: 686,
 * 32: 922, 64: 890, 128: 1 036 -- beyond twelve chains per compute unit the lane-per-plane kernel of decoder_wave.hpp takes
 * over, launched once per size class of row ring (chosen per call; ICER_DEC_WAVE=0|1|2 pins a kernel).  A separate library, so
 * that libicer_hip.so (the measured encoder) is unaffected.
 *
 * Same names, argument meaning and return codes as the decoding entry points of lib_icer
 * (TheRealOrange/icer_compression, lib_icer/inc/icer.h); the work runs on the GPU and there is no CPU fallback
 * (without a usable HIP device the image functions return ICER_FATAL_ERROR and print the reason to stderr).
 * Results equal the reference's for streams made of CRC-valid packets; where the reference reads memory it does not
 * own (bits behind the end of the stream, packet fields used as indices unchecked, the mean of a YUV channel without
 * packets) this library reads zeros / ignores the packet / uses 0.
 */
#ifndef ICER_HIP_DEC_H
#define ICER_HIP_DEC_H

#include "icer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* replaces icer_get_image_dimensions, icer.h:374 (lib_icer/src/icer_compress.c:541-566): size fields of the first
 * CRC-valid packet.  Host only.  ICER_INVALID_INPUT for null arguments, ICER_DECODER_OUT_OF_DATA when no packet is found. */
int icer_get_image_dimensions(const uint8_t *datastream, size_t data_length, size_t *image_w, size_t *image_h);

/* replaces icer_decompress_image_uint16, icer.h:461-462 (lib_icer/src/icer_compress.c:430-536).  `image` (host memory,
 * image_bufsize samples) receives the decoded image; *image_w / *image_h are set from the stream.  `stages`, `filt`
 * and `segments` must be the ones the stream was made with.  ICER_BYTE_QUOTA_EXCEEDED when the buffer is too small,
 * ICER_TOO_MANY_SEGMENTS when a subband is too small for the segment grid (the image then holds the sign-magnitude
 * words decoded up to that point, as in the reference). */
int icer_decompress_image_uint16(uint16_t *image, size_t *image_w, size_t *image_h, size_t image_bufsize,
                                 const uint8_t *datastream, size_t data_length, uint8_t stages,
                                 enum icer_filter_types filt, uint8_t segments);

/* replaces icer_decompress_image_yuv_uint16, icer.h:463-465 (lib_icer/src/icer_color.c:534-663) */
int icer_decompress_image_yuv_uint16(uint16_t *y_channel, uint16_t *u_channel, uint16_t *v_channel, size_t *image_w,
                                     size_t *image_h, size_t image_bufsize, const uint8_t *datastream,
                                     size_t data_length, uint8_t stages, enum icer_filter_types filt, uint8_t segments);

/* replace icer_decompress_image_uint8 / icer_decompress_image_yuv_uint8, icer.h:407-411
 * (lib_icer/src/icer_compress.c:168-277, icer_color.c:208-340): int8 storage, 7 bit planes */
int icer_decompress_image_uint8(uint8_t *image, size_t *image_w, size_t *image_h, size_t image_bufsize,
                                const uint8_t *datastream, size_t data_length, uint8_t stages,
                                enum icer_filter_types filt, uint8_t segments);
int icer_decompress_image_yuv_uint8(uint8_t *y_channel, uint8_t *u_channel, uint8_t *v_channel, size_t *image_w,
                                    size_t *image_h, size_t image_bufsize, const uint8_t *datastream,
                                    size_t data_length, uint8_t stages, enum icer_filter_types filt, uint8_t segments);

/* ---- Part 2: batches and device-resident buffers (our extension; what a decode benchmark times) -------------------
 * One decoder per (channels, stages, filter, segments, sample width); its device buffers grow on demand and are kept.
 * Every frame's image, size and return code equal those of a per-frame call of the Part-1 function. */
typedef struct icerx_decoder icerx_decoder;

/* device < 0: the current HIP device.  sample_bits: 16 or 8. */
int icerx_decoder_create(icerx_decoder **out, int device, int channels, int stages, int filt, unsigned segments,
                         int sample_bits);
void icerx_decoder_destroy(icerx_decoder *dec);

/* n streams in one host buffer: stream k = data[offsets[k] .. offsets[k] + lens[k]).  Frame k's channel c is written to
 * planes_out[k * channels + c] (host memory, frame_stride samples each: uint16 or uint8 by sample_bits).  Per frame:
 * rcs[k] = the Part-1 return code, ws[k] / hs[k] = the image size (in: the values kept when the stream holds no valid
 * packet).  Returns ICER_RESULT_OK, or ICER_FATAL_ERROR / ICER_INVALID_INPUT for the call as a whole. */
int icerx_decode_host(icerx_decoder *dec, int n, const uint8_t *data, const size_t *offsets, const size_t *lens,
                      void *const *planes_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs);

/* the same with the streams and the images in device memory: frame k's channel c at
 * d_out + (k * channels + c) * frame_stride samples; only its first ws[k] * hs[k] samples are results.  Synchronous. */
int icerx_decode_device(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                        void *d_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs);

/* Stream-ordered twin of icerx_decode_device: every input and output per frame is in device memory, everything is planned
 * on the GPU (decoder_async.hpp), and the call only enqueues work on `stream` (a hipStream_t; NULL: the null stream) and
 * returns.  It makes no blocking copy, no stream or device synchronisation and no hipMalloc / hipFree.
 *   stream k = d_data[off_k, off_k + d_lens[k]), off_k = d_offsets[k], or k * stream_stride when d_offsets is NULL (the
 *   encoder's d_out / out_stride / d_sizes plug in unchanged).  d_ws / d_hs are read as the in-values of the synchronous call.
 *   Frame k's outputs d_out, d_rcs[k], d_ws[k], d_hs[k] equal those of icerx_decode_device on the same streams.  A frame
 *   whose bytes leave [0, data_bytes) gets ICER_INVALID_INPUT and is not decoded; a wave-per-plane chain past its spin
 *   bound (an internal error; the synchronous call fails as a whole) gives its frame ICER_FATAL_ERROR.
 * The workspace (device memory, owned by the caller) holds at least icerx_decode_workspace_bytes(dec, n, data_bytes,
 * frame_stride) bytes: about 4 bytes per blob byte for the packet candidates (at most ceil(data_bytes / 2) of 8 bytes each)
 * plus 2 bytes per output sample (4 for 8-bit decoders) and a per-frame packet table.  It and every buffer passed in must
 * stay untouched until the work has completed on `stream`.  The call returns ICER_INVALID_INPUT for null arguments or a
 * workspace that is too small, ICER_FATAL_ERROR for data_bytes or frame_stride past the 32-bit limits of the synchronous
 * call (nothing is enqueued then).  Part of the work runs on the decoder's side streams, forked from `stream` and joined
 * back to it with events: once `stream` has completed, so has the call.  Calls on different streams may be in flight
 * together, each with its own workspace; the decoder object itself is not thread-safe. */
size_t icerx_decode_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t frame_stride);
int icerx_decode_device_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                              size_t stream_stride, const uint64_t *d_lens, void *d_out, size_t frame_stride, int32_t *d_rcs,
                              uint64_t *d_ws, uint64_t *d_hs, void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Decoding straight to 8-bit display images ----------------------------------------------------------------------
 * The counterpart of the encoder's front-end fusion (icerx_encode_device_u8 / _rgb8, icer_hip.h): the decoder's last pass
 * writes gray8 (1-channel decoders) or packed RGB888 (3-channel decoders) instead of planes, for sample_bits 16 and 8
 * (csrc/decoder_display.hpp).  With v the sample the plain call delivers, taken as unsigned (uint16, or uint8 for an 8-bit
 * decoder), and clip clamping to 0..255:
 *     gray8    min(v, 255), one byte per pixel
 *     RGB888   R = clip(Y + ((91881 Cr) >> 16) - 179)
 *              G = clip(Y - ((22544 Cb + 46793 Cr) >> 16) + 135)
 *              B = clip(Y + ((116129 Cb) >> 16) - 226),       three bytes per pixel in the order R, G, B
 * -- what the reference's callers compute on the host (example/inc/color_util.h CYCbCr2R/G/B, example/src/icer_util.c
 * yuv_to_rgb888_packed and :321-326).  The reference evaluates the products in 32-bit int, which overflows (undefined
 * behaviour) from Cb >= 18 493 or Cr >= 23 373; this library gives the exact integer result for every input 0..65535, which
 * equals the reference's wherever the reference's is defined.
 * frame_stride is in PIXELS: frame k's image starts at d_out + k * channels * frame_stride bytes (or is images_out[k]), pixel
 * i at byte channels * i.  For every frame of every call rcs / ws / hs equal those of the plain call (icerx_decode_device /
 * _async) on the same input, and the image is the conversion above of the first ws * hs samples the plain call delivers for
 * the frame -- whatever its return code: damaged and truncated streams and frames that stop before the transform included.
 * Nothing is written behind channels * ws * hs bytes of a frame's row, in the row of a frame for which the plain call writes
 * no samples, beyond the n rows, or to the input.  The 32-bit limits of the plain calls apply unchanged. */

/* icerx_decode_host with one host image per frame: images_out[k] holds channels * frame_stride bytes */
int icerx_decode_host_display(icerx_decoder *dec, int n, const uint8_t *data, const size_t *offsets, const size_t *lens,
                              uint8_t *const *images_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs);

/* icerx_decode_device with the images in device memory.  Synchronous. */
int icerx_decode_device_display(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                                uint8_t *d_out, size_t frame_stride, int *rcs, size_t *ws, size_t *hs);

/* icerx_decode_device_async with the images in d_out, stream-ordered under the same rules (no blocking copy, no
 * synchronisation, no hipMalloc / hipFree).  The working planes (2 bytes per sample, for either sample width) live in the
 * caller's workspace: it holds at least icerx_decode_display_workspace_bytes(dec, n, data_bytes, frame_stride) bytes.
 * ICER_INVALID_INPUT for null arguments or a workspace that is too small: nothing is enqueued or written. */
size_t icerx_decode_display_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t frame_stride);
int icerx_decode_device_display_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                      size_t stream_stride, const uint64_t *d_lens, uint8_t *d_out, size_t frame_stride,
                                      int32_t *d_rcs, uint64_t *d_ws, uint64_t *d_hs, void *d_workspace, size_t workspace_bytes,
                                      void *stream);

/* The conversion alone, for planes already in device memory (callers who processed the planes themselves): frame k's channel
 * c = w * h samples at d_planes + (k * channels + c) * plane_stride samples (uint16 or uint8 by sample_bits), taken as they
 * are (no negative-clamping); frame k's image at d_out + k * channels * frame_stride bytes.  Enqueued on `stream`; no
 * synchronisation.  The same device function as the fused pass.  ICER_INVALID_INPUT -- nothing enqueued -- for null pointers,
 * channels other than 1 or 3, sample_bits other than 16 or 8, n_frames < 0, or w * h beyond plane_stride or frame_stride. */
int icerx_planes_to_display_device(const void *d_planes, int n_frames, int channels, size_t w, size_t h, size_t plane_stride,
                                   int sample_bits, uint8_t *d_out, size_t frame_stride, void *stream);

/* lib_icer-shaped single-stream call for 16-bit streams: `image` (host memory, channels * image_bufsize_pixels bytes)
 * receives the gray8 (channels 1) or RGB888 (channels 3) image; return codes as icer_decompress_image_[yuv_]uint16, and
 * ICER_INVALID_INPUT for channels other than 1 or 3. */
int icerx_decompress_display(uint8_t *image, size_t *image_w, size_t *image_h, size_t image_bufsize_pixels,
                             const uint8_t *datastream, size_t data_length, uint8_t stages, enum icer_filter_types filt,
                             uint8_t segments, int channels);

/* ---- Decoding at 1/2^r resolution --------------------------------------------------------------------------------------
 * A stream made with S stages holds the image at 1/2 .. 1/2^(S-1) size as the low-pass corner of its coefficient pyramid.  A
 * reduced decoder (0 <= r < S) never starts the entropy chains of levels 1 .. r -- level 1 alone is 3/4 of all samples -- and
 * runs S - r inverse stages on what is left.  What it delivers is DEFINED through the derived stream X_r of a stream X:
 *     walk X with the decoder's cursor rule (a CRC-valid packet is stepped over whole, anything else byte by byte; every valid
 *     packet takes part in the walk); keep, in order, the valid packets of decomp_level > r; in each kept header set
 *     decomp_level -= r, image_w = ceil(image_w / 2^r), image_h = ceil(image_h / 2^r) and recompute the header CRC; payloads
 *     and payload CRCs stay.
 * The reduced decode of X at r is the plain decode of X_r by a decoder made for (S - r stages, the same filter, segments and
 * sample width): image, size, return code, damaged and truncated streams, a frame whose valid packets are all dropped (it
 * keeps the size in-values, like an empty stream) included.  That is exact, not an approximation: ceil(ceil(w / 2^r) / 2^k) =
 * ceil(w / 2^(r + k)), so the level-k subbands of the reduced image have the sizes -- and therefore the segment grids -- of
 * the level-(r + k) subbands of the full one; the context model goes by subband type alone; the LL mean travels in the
 * header.  The image is the top-left LL_r corner the full decode holds after S - r of its S inverse stages, with negative
 * samples clamped to zero at that size.  (A chain whose packets do not decode within their own payloads -- coefficients
 * above the coded bit planes -- reads on into the bytes that follow in X, as the plain decode does.) */

/* A decoder for streams made with `stages`, delivering every image at 1/2^reduce size.  0 <= reduce < stages, else
 * ICER_INVALID_INPUT; reduce 0 is icerx_decoder_create.  Every entry point that takes the decoder then works on the reduced
 * image: host, device, async, the three display calls, and the two workspace-size functions.  frame_stride / bufsize are
 * measured against ceil(w / 2^r) * ceil(h / 2^r), and ws / hs / d_ws / d_hs report the reduced size. */
int icerx_decoder_create_reduced(icerx_decoder **out, int device, int channels, int stages, int filt, unsigned segments,
                                 int sample_bits, int reduce);
int icerx_decoder_reduce(const icerx_decoder *dec);                                /* the decoder's reduce (0 for NULL) */
void icerx_reduced_size(size_t w, size_t h, int reduce, size_t *rw, size_t *rh);   /* host helper, ceil(w / 2^r) */
/* lib_icer-shaped one-shot: planes[c] host memory of bufsize samples (uint16 / uint8 by sample_bits), channels 1 or 3 */
int icerx_decompress_reduced(void *const planes[], int channels, size_t *image_w, size_t *image_h, size_t bufsize,
                             const uint8_t *datastream, size_t data_length, uint8_t stages, enum icer_filter_types filt,
                             uint8_t segments, int sample_bits, int reduce);

/* ---- Reconstructing truncated coefficients inside their interval ------------------------------------------------------
 * Every lossy stream of this library is a truncated bit-plane stream.  A coefficient whose lowest p planes never arrived is
 * known to lie in [m, m + 2^p - 1]; lib_icer, and this decoder by default, rebuild it at m.  A decoder can be told to rebuild
 * every NON-ZERO coefficient k eighths of the way into that interval instead.  It costs no stream bytes and changes no
 * stream.  The rule is exact and in integers:
 *     P = 9 coded planes (16-bit decoder) or 7 (8-bit).  For a chain (channel, level, subband, segment): t = the packets
 *     present consecutively from plane P - 1 downwards (the planes the chain runs), p = P - t -- the planner's figure: a
 *     packet whose decode stops early inside still counts.  off(p, k) = (k * (2^p - 1)) >> 3.
 *     After the entropy stage and before sign-magnitude removal, every word of the chain's rectangle with a non-zero
 *     magnitude becomes magnitude + off(p, k); the sign stays, a zero magnitude stays (with or without a set sign bit).  LL
 *     chains as well.  Only frames that reach the transform: a frame that stops early keeps its words as they are.
 * Everything behind that step is as before: the LL mean, the inverse transform, the clamp, narrowing, display conversion,
 * return codes.  k = 0 is the plain decoder byte for byte, and a lossless stream (p = 0 everywhere) decodes identically for
 * every k.  For a reduced decoder the rule applies to the chains of the derived stream.
 * k = 3 is the recommended value: it lowered the squared error in every case measured (profiles/decode_recon.md; about
 * 0.6 dB at medium rates), while the midpoint k = 4 is sometimes worse than k = 0. */

/* eighths in 0 .. 4, anything else: ICER_INVALID_INPUT and the decoder stays as it was.  The setting holds for every entry
 * point that takes the decoder (host, device, async, the three display calls; reduced decoders too) and is read when a call
 * is enqueued: asynchronous calls already in flight keep theirs.  The lib_icer drop-in calls icer_decompress_image_* stay
 * at the reference's reconstruction. */
int icerx_decoder_set_reconstruction(icerx_decoder *dec, int eighths);
int icerx_decoder_reconstruction(const icerx_decoder *dec);                        /* the decoder's setting (0 for NULL) */
/* the one-shot call, shaped like icerx_decompress_reduced (reduce 0: full size) */
int icerx_decompress_reconstructed(void *const planes[], int channels, size_t *image_w, size_t *image_h, size_t bufsize,
                                   const uint8_t *datastream, size_t data_length, int stages, int filt, unsigned segments,
                                   int sample_bits, int reduce, int eighths);

/* ---- Re-cutting stored streams to smaller byte quotas ---------------------------------------------------------------
 * A byte quota decides only where a stream is cut, never what a packet holds.  So from a stored master stream M of a frame
 * -- made by this project's encoders or by the reference at quota Qm, return code ICER_RESULT_OK or
 * ICER_BYTE_QUOTA_EXCEEDED -- the stream at any quota Q <= Qm (any Q when M is complete) is cut without the pixels and
 * without re-coding: the output has exactly the bytes, size and return code of icerx_encode_device (or _s8, or the
 * reference) on the original frame at quota Q.  The rule: M's CRC-valid packets are found with the decoder's cursor rule
 * (the last packet of a kind wins), each is mapped to its coding unit in priority order by (channel, level, subband, bit
 * plane, segment), a unit without a packet counts as "does not fit", the encoder's quota walk runs at Q (a unit is kept
 * iff its 28 header bytes fit and floor(bits / 8) < Q - used - 28; the first unit that fails ends the stream), and the
 * kept packets are copied verbatim, header and payload, into the final stream order.
 * Two consequences:
 *   - Q > Qm on a cut master: the walk ends at the first unit M lacks, so the output is M itself with
 *     ICER_BYTE_QUOTA_EXCEEDED (not what an encode at Q gives).
 *   - a damaged master is cut at the first unit, in priority order, whose packet is missing or fails a CRC; valid packets
 *     behind that point are dropped (the encoder's "first failure stops everything").
 * One recutter per geometry the masters were made with; icerx_recutter_create refuses what the encoder's planner refuses,
 * with its code (ICER_INVALID_INPUT, ICER_TOO_MANY_STAGES, ICER_TOO_MANY_SEGMENTS, ICER_PACKET_COUNT_EXCEEDED).  It uploads
 * the unit -> packet-table slot map, the final order and the unit table once; there is no per-sample memory.
 * device < 0: the current HIP device.  sample_bits: 16 or 8. */
typedef struct icerx_recutter icerx_recutter;
int icerx_recutter_create(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, unsigned segments,
                          int sample_bits);
void icerx_recutter_destroy(icerx_recutter *r);

/* Stream-ordered, like icerx_decode_device_async: the call only enqueues work on `stream` and returns -- no blocking copy,
 * no synchronisation, no hipMalloc / hipFree, no host round trip.  The masters are addressed as there: master k =
 * d_data[off_k, off_k + d_lens[k]), off_k = d_offsets[k], or k * stream_stride when d_offsets is NULL, so an encoder's d_out /
 * out_stride / d_sizes plug in unchanged.  `quotas` is a HOST array of 1 .. ICERX_MAX_LADDER byte quotas in any order,
 * repeats allowed, passed by value with the launch.  The outputs are laid out exactly as icerx_encode_device_ladder's:
 * frame f at quota q is row q * n + f of d_out (out_stride bytes per row), its size and return code d_sizes[q * n + f] /
 * d_rcs[q * n + f]; a quota's block of n rows feeds icerx_decode_device_async directly.  Per frame and quota:
 *   every unit kept                                   ICER_RESULT_OK, the stream's length
 *   cut                                               ICER_BYTE_QUOTA_EXCEEDED, the stream's length
 *   the master holds no valid packet                  ICER_DECODER_OUT_OF_DATA, 0
 *   the master leaves [0, data_bytes)                 ICER_INVALID_INPUT, 0
 *   a valid packet's width / height are not w / h     ICER_INVALID_INPUT, 0
 * Nothing is written behind a stream in its row, beyond the n_quotas * n rows, or to the masters.  The whole call returns
 * ICER_INVALID_INPUT -- nothing enqueued, nothing written -- for a null pointer (d_offsets and stream excepted), n outside
 * 1 .. 65535, n_quotas outside 1 .. ICERX_MAX_LADDER, out_stride below the largest quota or a workspace smaller than
 * icerx_recut_workspace_bytes(r, n, data_bytes, n_quotas), and ICER_FATAL_ERROR for data_bytes past the 32-bit limit of the
 * asynchronous decode.  The workspace (device memory, owned by the caller: about 4 bytes per blob byte for the packet
 * candidates, a packet table per frame and 8 bytes per coding unit, frame and quota) and every buffer passed in must stay
 * untouched until the work has completed on `stream`.  Calls on different streams may be in flight together, each with its
 * own workspace. */
size_t icerx_recut_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_quotas);
int icerx_recut_device_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                             size_t stream_stride, const uint64_t *d_lens, const size_t *quotas, int n_quotas,
                             uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs,
                             void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Re-cutting by resolution as well as by byte quota ---------------------------------------------------------------
 * A stored master also holds the stream of the image at 1/2^r size: its derived stream M_r ("Decoding at 1/2^r resolution"
 * above), which an unmodified lib_icer decoder told stages - r decodes.  A CUT is a pair (reduce r, byte quota Q) with
 * 0 <= r <= max_reduce < stages, and the cut of a master M is DEFINED as
 *     the output of the re-cut rule above at quota Q, applied to M_r, by a recutter made for
 *     (ceil(w / 2^r), ceil(h / 2^r), channels, stages - r, segments, sample_bits).
 * The same rule from the master's side: walk M with the decoder's cursor rule (every CRC-valid packet takes part, the last
 * packet of a kind wins); packets of decomp_level <= r are stepped over and otherwise ignored; a packet of level l > r
 * stands for the coding unit (channel, l - r, subband, bit plane, segment) of the geometry at 1/2^r size -- its segment
 * grids are those of level l of the full geometry, as shown above -- while the priority order, the final order and the
 * quota walk are that geometry's own (the planner run on it; the priority order of one geometry is not a part of
 * another's); a unit without a packet ends the walk; the kept packets are copied in final order with decomp_level -= r,
 * image_w = ceil(image_w / 2^r), image_h = ceil(image_h / 2^r) and the header CRC (bytes 24..27) recomputed over bytes
 * 0..23; payload and payload CRC are copied verbatim.  Consequences:
 *   - r = 0 is the re-cut above, byte for byte.
 *   - a complete, undamaged master and Q above the length of M_r: the output is M_r itself with ICER_RESULT_OK.  (At Q equal
 *     to that length the quota walk can drop the last unit -- floor(bits / 8) < Q - used - 28 is strict -- as an encode at
 *     that quota does.)
 *   - damage at a level <= r changes nothing in a cut at r; damage or truncation above level r cuts the stream at the first
 *     unit, in the priority order of the geometry at 1/2^r size, that lost its packet.
 *   - a master whose valid packets all have level <= r gives ICER_DECODER_OUT_OF_DATA and size 0 for that cut, as an empty
 *     master does.
 *   - the two per-frame checks are the MASTER's, the one place where the rule is stated on M and not on M_r: a frame that
 *     leaves the blob, or that holds a valid packet of ANY level whose width or height is not the recutter's w / h, gives
 *     ICER_INVALID_INPUT and size 0 for every cut -- also where M_r would not hold that packet, or would hold it with the
 *     size of the geometry at 1/2^r.
 *   - cuts compose: a stored output of cut (r, Q1), re-cut by a plain recutter of the geometry at 1/2^r size to Q2 <= Q1,
 *     is cut (r, Q2) of the master.
 * icerx_recutter_create_reduced makes a recutter with the tables of reduce 0 .. max_reduce (the unit table, the unit ->
 * packet-table slot map and the final order of every geometry, from the planner on that geometry, uploaded once);
 * 0 <= max_reduce < stages, else ICER_INVALID_INPUT; otherwise it refuses what icerx_recutter_create refuses, and where both
 * the geometry and max_reduce are bad the geometry's code is returned (the planner runs on the full geometry first).  (The units of
 * a geometry at 1/2^r size are a part of the full geometry's, so the planner accepts it whenever it accepts the full one.)
 * icerx_recutter_create is max_reduce 0; every recutter serves icerx_recut_device_async unchanged. */
int icerx_recutter_create_reduced(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages,
                                  unsigned segments, int sample_bits, int max_reduce);
int icerx_recutter_max_reduce(const icerx_recutter *r);            /* 0 for NULL or a plain recutter */

/* icerx_recut_device_async with cuts in place of quotas, and with every stream-ordered promise of it: the call only
 * enqueues.  `reduces` and `quotas` are HOST arrays of n_cuts entries, 1 .. ICERX_MAX_LADDER, in any order, repeats allowed,
 * passed by value with the launch.  Frame f at cut c is row c * n + f of d_out, its size and return code d_sizes[c * n + f]
 * / d_rcs[c * n + f] (the table of icerx_recut_device_async, per frame and cut); the block of n rows of one cut feeds
 * icerx_decode_device_async of a decoder made for stages - reduces[c] directly.  Nothing is written behind a stream in its
 * row, beyond the n_cuts * n rows, or to the masters.  The whole call returns ICER_INVALID_INPUT -- nothing enqueued, nothing
 * written -- for what icerx_recut_device_async refuses, a null `reduces`, a reduce outside 0 .. max_reduce or a workspace
 * smaller than icerx_recut_cuts_workspace_bytes(r, n, data_bytes, n_cuts) (which is never below
 * icerx_recut_workspace_bytes of the same arguments: 4 more bytes per frame and coding unit of every geometry, 8 more per
 * frame, cut and coding unit of the full geometry); ICER_FATAL_ERROR as there.  The packet table is made once per frame;
 * a packet's payload is read once for all cuts that keep it.  A call whose reduces are all 0 runs icerx_recut_device_async's
 * own kernels. */
size_t icerx_recut_cuts_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts);
int icerx_recut_device_cuts_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                  size_t stream_stride, const uint64_t *d_lens, const int *reduces, const size_t *quotas,
                                  int n_cuts, uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs,
                                  void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Re-cutting by region of interest, at any resolution ---------------------------------------------------------------
 * icerx_encode_device_roi (icer_hip.h) spends a byte quota inside a rectangle first, but it needs the frame.  The rule only
 * chooses which packets are kept, so it can be applied to a stored master instead: a CUT is here a triple (reduce r, byte
 * quota Q, ROI shift), each frame has a rectangle (x, y, w, h in pixels of the FULL frame), and
 *   at r = 0 the cut of a master M is the region-of-interest rule of icer_hip.h run on M's packet table instead of the
 *     coder's bit counts: walk M with the decoder's cursor rule exactly as icerx_recut_device_async does (every CRC-valid
 *     packet takes part, the last packet of a kind wins, the master's two per-frame checks apply); a unit without a packet
 *     "does not fit"; a unit is foreground when it belongs to LL or comes within 2 coefficients of the rectangle scaled to
 *     its level; the units are ordered by eff = prio << shift (foreground) or prio (the others), descending, ties by unit
 *     index; a frame whose rectangle, clipped to the frame, is empty has shift 0; the quota walk runs over that order and
 *     keeps the first K units, which are copied verbatim in final order.
 *   at r > 0 take [x0, x1) x [y0, y1), the frame's rectangle clipped to the full frame.  If it is empty the frame has no
 *     region of interest at any r.  Otherwise the rectangle of the cut is [x0 >> r, ceil(x1 / 2^r)) x [y0 >> r,
 *     ceil(y1 / 2^r)): never empty, and inside ceil(w / 2^r) x ceil(h / 2^r).  The cut is DEFINED as the r = 0 rule applied to
 *     the derived stream M_r, with that rectangle and the same shift and quota, by a recutter made for
 *     (ceil(w / 2^r), ceil(h / 2^r), channels, stages - r, segments, sample_bits): priority order, final order and priorities
 *     are that geometry's own, and the headers are relabelled as in icerx_recut_device_cuts_async.
 *     Since floor((x0 >> r) / 2^l) = floor(x0 / 2^(l + r)), and the same for the ceilings, a non-LL unit of level l at
 *     1/2^r size is foreground exactly when the master's unit of level l + r is; only LL and the priorities differ.
 *     (Where the planner keeps a grid -- a subband with fewer samples than segments takes the rectangles of the packet
 *     before it, and which packet that is depends on the priorities -- the rectangles of the plan at 1/2^r size, not the
 *     ones the master's payloads were coded with, decide foreground.)
 * Consequences:
 *   - r = 0 and a complete master: bytes, size, return code, K and the foreground count of icerx_encode_device_roi on the
 *     original frame with the same rectangle, shift and quota.
 *   - shift 0, a rectangle that is empty once clipped (one outside the frame included), a rectangle whose foreground is
 *     every unit, or a one-segment geometry: icerx_recut_device_cuts_async's output for (r, Q), byte for byte.
 *   - cuts compose: a stored ROI stream made with (rectangle, shift) at Q1, re-cut with the same rectangle and shift at
 *     Q2 <= Q1, is the ROI stream at Q2; a stored output of cut (r, Q1, shift), re-cut by a plain recutter of the geometry
 *     at 1/2^r size with the scaled rectangle at Q2 <= Q1, is cut (r, Q2, shift).
 *   - a cut master, or one damaged above level r, ends the walk at the first unit IN ROI ORDER that has no packet, with
 *     ICER_BYTE_QUOTA_EXCEEDED.  (So the byte-quota and cuts calls, which walk in priority order, cut a stored ROI stream
 *     at the first background unit it lacks; this call, given the rectangle and shift it was made with, does not.)
 *   - the frame statuses are icerx_recut_device_cuts_async's (ICER_DECODER_OUT_OF_DATA, ICER_INVALID_INPUT, no valid packet
 *     above level r); size, K and the foreground count of such a frame are 0.
 *   - every output is a subset of M_r's packets with both CRCs valid and no bit plane kept below a dropped one of its
 *     family, so any decoder told stages - r decodes it.
 * Arguments: the masters, d_out / out_stride / d_sizes / d_rcs (row and entry c * n + f) and the nothing-written promises
 * are those of icerx_recut_device_cuts_async.  d_rois is DEVICE memory, n x 4 uint32 (x, y, w, h), read on `stream` -- a
 * kernel that wrote it on the same stream just before needs no synchronisation -- per frame and shared by all cuts; values
 * are read as uint32, so int32 values below 0 read as far outside.  `reduces`, `shifts` and `quotas` are HOST arrays of n_cuts
 * entries passed by value; reduces == NULL means every reduce is 0 (any recutter serves such a call), otherwise each lies in
 * 0 .. max_reduce; 0 <= shifts[c] <= ICERX_MAX_ROI_SHIFT, per cut, so one call delivers a plain cut and a ROI cut side by
 * side.  d_kept / d_foreground: n_cuts * n entries each, K and the number of foreground units of the cut's geometry.
 * The whole call returns ICER_INVALID_INPUT -- nothing enqueued, nothing written -- for what
 * icerx_recut_device_cuts_async refuses (a null `reduces` excepted), a null d_rois, shifts, d_kept or d_foreground, a shift
 * out of range, or a workspace below icerx_recut_roi_workspace_bytes(r, n, data_bytes, n_cuts) (the cuts call's, and 20 more
 * bytes per frame, cut and coding unit of the full geometry).  Stream-ordered with every promise of the calls above: no
 * blocking copy, no synchronisation, no hipMalloc / hipFree, no host round trip.  Every recutter holds, from its creation,
 * the priority of every unit's packet for every geometry 0 .. max_reduce (8 bytes per unit); a geometry whose priorities do
 * not fit the sort keys makes the create call return ICER_FATAL_ERROR (no geometry the planner accepts does). */
size_t icerx_recut_roi_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts);
int icerx_recut_device_roi_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                 size_t stream_stride, const uint64_t *d_lens, const uint32_t *d_rois, const int *reduces,
                                 const int *shifts, const size_t *quotas, int n_cuts, uint8_t *d_out, size_t out_stride,
                                 uint64_t *d_sizes, int32_t *d_rcs, uint32_t *d_kept, uint32_t *d_foreground,
                                 void *d_workspace, size_t workspace_bytes, void *stream);

/* ---- Refinement increments: the difference and the union of two stored streams ------------------------------------------
 * A decoder files every CRC-valid packet by (channel, level, subband, bit plane, segment) and does not mind the order of the
 * packets, so a stream followed by the packets it lacks decodes exactly as the larger stream does.  This call computes those
 * packets -- what to send to a client that holds cut A and wants cut B -- and the canonical stream of both.
 * Operands: both live in one blob d_data[0, data_bytes).  Frame k of operand X is [off, off + d_lens_x[k]) with
 * off = d_offsets_x[k], or base_x + k * stream_stride when d_offsets_x is NULL; the output block of a two-cut re-cut call plugs
 * in as it is (base_a = 0, base_b = n * out_stride, lens d_sizes and d_sizes + n).  A zero-length operand is an empty set.  An
 * operand may be any concatenation of streams and increments of one frame: it is walked with the decoder's cursor rule, as
 * icerx_recut_device_async walks a master, so within an operand the last valid packet of a kind wins.  `r` is a recutter made
 * for the streams' own geometry (for cuts at 1/2^r size: a plain recutter of the geometry at that size); only its tables of
 * reduce 0 are used, and a packet that is not a coding unit of that plan is dropped.  Per unit u of the plan:
 *   ICERX_COMBINE_UNION        kept when A or B has a valid packet of u; B's packet if B has one, else A's
 *   ICERX_COMBINE_DIFFERENCE   kept when B has a valid packet of u and A has none; B's packet
 * The kept packets are copied verbatim, header and payload, in the plan's final order.  "A has it" is decided by the unit
 * alone, never by comparing payloads; a packet of A that fails a CRC is absent, so the difference against a damaged copy
 * re-sends exactly the damaged packets.  When A's units are a part of B's: union(A, difference(A, B)) is B byte for byte, and
 * the difference is len(B) - len(A) bytes.
 * Per frame k: d_sizes[k], d_rcs[k], d_counts[2 k] = packets written, d_counts[2 k + 1] = how many of them came from A.
 *   an operand leaves [0, data_bytes), or either operand holds a
 *   valid packet whose width / height are not the recutter's      ICER_INVALID_INPUT, size 0, counts 0
 *   UNION: neither operand holds a valid packet;
 *   DIFFERENCE: B holds none                                       ICER_DECODER_OUT_OF_DATA, size 0, counts 0
 *   the result is longer than out_stride                           ICER_OUTPUT_BUF_TOO_SMALL, d_sizes = the bytes needed, counts
 *                                                                  valid, the row untouched (len_a + len_b for UNION, len_b
 *                                                                  for DIFFERENCE always suffice)
 *   otherwise                                                      ICER_RESULT_OK, the length (an empty difference: 0)
 * Stream-ordered with every promise of icerx_recut_device_async: the call only enqueues -- no blocking copy, no
 * synchronisation, no hipMalloc / hipFree; nothing is written behind a stream in its row, beyond the n rows, n entries or 2 n
 * counts, to the blob or outside the workspace.  The whole call returns ICER_INVALID_INPUT -- nothing enqueued, nothing
 * written -- for a null pointer (the two offset arrays and `stream` excepted), n outside 1 .. 65535, an `op` other than the
 * two, or a workspace below icerx_combine_workspace_bytes(r, n, data_bytes) (about 4 bytes per blob byte, two packet tables
 * per frame and 16 bytes per frame and coding unit); ICER_FATAL_ERROR for data_bytes past the 32-bit limit, as in the re-cut. */
#define ICERX_COMBINE_UNION      0
#define ICERX_COMBINE_DIFFERENCE 1
size_t icerx_combine_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes);
int icerx_combine_device_async(icerx_recutter *r, int n, int op, const void *d_data, size_t data_bytes,
                               const uint64_t *d_offsets_a, size_t base_a, const uint64_t *d_lens_a,
                               const uint64_t *d_offsets_b, size_t base_b, const uint64_t *d_lens_b, size_t stream_stride,
                               uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, uint32_t *d_counts,
                               void *d_workspace, size_t workspace_bytes, void *stream);

/* last error message of this thread's most recent failing call ("" if none) */
const char *icerx_decoder_last_error(void);

/* ---- Standalone wavelet transform, inverse (lib_icer/inc/icer.h:414-417, :468-471, :487-488) ----------------------
 * The twins of the forward calls in icer_hip.h, with the same contract: buffer and return code equal the reference's
 * (ICER_INTEGER_OVERFLOW included: wrapped values are stored and the transform goes on; the uint8 twins keep the
 * reference's scrambled interleave of odd-length lines), ICER_TOO_MANY_STAGES leaves the buffer untouched, a line
 * shorter than 2 samples returns ICER_INVALID_INPUT untouched, _2d leaves samples beyond image_w of each row alone, _1d
 * touches only its N samples (gathered with a 2-D copy: for completeness, not speed).  Runs on the GPU; serialised.
 * icer_from_sign_magnitude_int16 / _int8 are host-only.  Not provided: see icer_hip.h. */
int icer_inverse_wavelet_transform_stages_uint16(uint16_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt);
int icer_inverse_wavelet_transform_2d_uint16(uint16_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt);
int icer_inverse_wavelet_transform_1d_uint16(uint16_t *data, size_t N, size_t stride, enum icer_filter_types filt);
int icer_inverse_wavelet_transform_stages_uint8(uint8_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt);
int icer_inverse_wavelet_transform_2d_uint8(uint8_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt);
int icer_inverse_wavelet_transform_1d_uint8(uint8_t *data, size_t N, size_t stride, enum icer_filter_types filt);
void icer_from_sign_magnitude_int16(uint16_t *data, size_t len);
void icer_from_sign_magnitude_int8(uint8_t *data, size_t len);

/* The inverse of icerx_wavelet_forward_device (icer_hip.h), same arguments and contract; the workspace size is
 * icerx_wavelet_workspace_bytes of libicer_hip.so. */
int icerx_wavelet_inverse_device(void *d_planes, int n_planes, size_t w, size_t h, size_t plane_stride, int stages, int filt,
                                 int sample_bits, void *d_workspace, int32_t *d_rcs, void *stream);

/* The window decode -- a rectangle of each image, skipping the chains it does not depend on: icerx_decode_*_window*,
 * icerx_decompress_window.  Declared and described in icer_hip_dec_window.h. */
#define ICER_HIP_DEC_H_WINDOW_PART 1
#include "icer_hip_dec_window.h"
#undef ICER_HIP_DEC_H_WINDOW_PART

/* Progressive decode sessions -- the coefficient state of held frames kept on the device, a feed decodes only the bit planes its
 * packets add and delivers the refined image.  Declared and described in icer_hip_dec_session.h. */
#define ICER_HIP_DEC_H_SESSION_PART 1
#include "icer_hip_dec_session.h"
#undef ICER_HIP_DEC_H_SESSION_PART

/* Re-cutting stored masters to a distortion target or a shared byte budget, from the masters and their distortion sidecars:
 * icerx_recutter_create_quality, icerx_recut_device_target_async, icerx_recut_device_budget_async.  Declared and described in
 * icer_hip_dec_quality.h. */
#define ICER_HIP_DEC_H_QUALITY_PART 1
#include "icer_hip_dec_quality.h"
#undef ICER_HIP_DEC_H_QUALITY_PART

#ifdef __cplusplus
}
#endif
#endif
