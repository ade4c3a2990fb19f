/*
 * icer_hip.h -- C ABI of libicer_hip.so, the MI355X (gfx950) ICER encoder.
 *
 * Part 1 restates, with identical names, argument meaning, struct layout and return codes, the
 * entry points of lib_icer that an application needs for ENCODING: the uint16 path and its uint8 twins
 * (TheRealOrange/icer_compression, lib_icer/inc/icer.h).  A program written against lib_icer links
 * against libicer_hip.so instead of libicer.a and produces byte-identical streams; the work runs
 * on the GPU (there is no CPU fallback: without a usable HIP device every compress call returns
 * ICER_FATAL_ERROR and prints the reason to stderr).
 *
 * Part 2 (prefix icerx_) is our extension for batches of frames and device-resident buffers,
 * which is what bench.py measures.  Each frame's stream, length and return code equal those of a
 * per-frame call of the Part-1 function on the same data.
 *
 * Plain C, LP64; no HIP or torch types appear in any signature (streams and device pointers are
 * passed as void*).
 */
#ifndef ICER_HIP_H
#define ICER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Part 1: lib_icer drop-in surface ------------------------------------------------------ */

/* enum icer_status, lib_icer/inc/icer.h:92-105 (same numeric values) */
enum icer_status {
    ICER_RESULT_OK = 0,
    ICER_INTEGER_OVERFLOW = -1,
    ICER_OUTPUT_BUF_TOO_SMALL = -2,
    ICER_TOO_MANY_SEGMENTS = -3,
    ICER_TOO_MANY_STAGES = -4,
    ICER_BYTE_QUOTA_EXCEEDED = -5,
    ICER_BITPLANE_OUT_OF_RANGE = -6,
    ICER_DECODER_OUT_OF_DATA = -7,
    ICER_DECODED_INVALID_DATA = -8,
    ICER_PACKET_COUNT_EXCEEDED = -9,
    ICER_FATAL_ERROR = -10,
    ICER_INVALID_INPUT = -11
};

/* enum icer_filter_types, lib_icer/inc/icer.h:107-115 */
enum icer_filter_types {
    ICER_FILTER_A = 0, ICER_FILTER_B, ICER_FILTER_C, ICER_FILTER_D, ICER_FILTER_E, ICER_FILTER_F, ICER_FILTER_Q
};

/* icer_output_data_buf_typedef, lib_icer/inc/icer.h:307-312 (32 bytes, same layout) */
typedef struct {
    size_t size_used;            /* out: length of the final stream at rearrange_start */
    size_t size_allocated;       /* byte quota */
    uint8_t *data_start;         /* staging half [0, quota): scratch, contents unspecified */
    uint8_t *rearrange_start;    /* final stream */
} icer_output_data_buf_typedef;

/* replaces icer_init, lib_icer/inc/icer.h:370 (lib_icer/src/icer_init.c:24-35): builds the coder
 * tables.  Idempotent.  Does not touch the GPU. */
int icer_init(void);

/* replaces icer_init_output_struct, icer.h:524 (lib_icer/src/icer_util.c:38-45).
 * Returns ICER_OUTPUT_BUF_TOO_SMALL when 2*byte_quota > buf_len. */
int icer_init_output_struct(icer_output_data_buf_typedef *out, uint8_t *data, size_t buf_len, size_t byte_quota);

/* replaces icer_compress_image_uint16, icer.h:440-441 (lib_icer/src/icer_compress.c:279-426).
 * `image` (host memory, w*h uint16, row-major) is overwritten with the sign-magnitude wavelet
 * coefficients exactly as the reference leaves it (written back while the coder is still running: of the
 * call's three transfers only the upload and the stream download are not hidden; bench.py `dropin`).  Returns ICER_RESULT_OK or
 * ICER_BYTE_QUOTA_EXCEEDED with a valid stream in output_data->rearrange_start[0..size_used),
 * or an error code with size_used == 0. */
int icer_compress_image_uint16(uint16_t *image, size_t image_w, size_t image_h, uint8_t stages,
                               enum icer_filter_types filt, uint8_t segments,
                               icer_output_data_buf_typedef *output_data);

/* replaces icer_compress_image_yuv_uint16, icer.h:442-444 (lib_icer/src/icer_color.c:343-530). */
int icer_compress_image_yuv_uint16(uint16_t *y_channel, uint16_t *u_channel, uint16_t *v_channel,
                                   size_t image_w, size_t image_h, uint8_t stages,
                                   enum icer_filter_types filt, uint8_t segments,
                                   icer_output_data_buf_typedef *output_data);

/* replaces icer_compress_image_uint8, icer.h:386-387 (lib_icer/src/icer_compress.c:17-166).  The uint8 twins treat
 * the samples as int8 STORAGE (a pixel value above 127 is a negative number, lib_icer/src/icer_wavelet.c:231) and code
 * 7 bit planes: only data of at most 7 bits survives the round trip, anything that leaves the int8 range during the
 * transform makes the call return ICER_INTEGER_OVERFLOW exactly as the reference does.  `image` (host memory, w*h
 * bytes) is overwritten with the int8 sign-magnitude wavelet coefficients; on ICER_INTEGER_OVERFLOW its contents are
 * left untouched (the reference leaves partially transformed data there).  ICER_PACKET_COUNT_EXCEEDED is returned for
 * (3*stages+1)*7*channels >= 300 packets as in the reference, without touching the image. */
int icer_compress_image_uint8(uint8_t *image, size_t image_w, size_t image_h, uint8_t stages,
                              enum icer_filter_types filt, uint8_t segments,
                              icer_output_data_buf_typedef *output_data);

/* replaces icer_compress_image_yuv_uint8, icer.h:388-390 (lib_icer/src/icer_color.c:18-206); note that its final
 * re-ordering walks subbands, levels and bit planes upwards, unlike the other three entry points. */
int icer_compress_image_yuv_uint8(uint8_t *y_channel, uint8_t *u_channel, uint8_t *v_channel,
                                  size_t image_w, size_t image_h, uint8_t stages,
                                  enum icer_filter_types filt, uint8_t segments,
                                  icer_output_data_buf_typedef *output_data);

/* ---- Part 2: batched / device-resident extension -------------------------------------------- */

typedef struct icerx_encoder icerx_encoder;

/* Create an encoder for frames of w x h with `channels` (1 = gray, 3 = Y,U,V planes) on HIP device
 * `device`.  All device memory for up to `max_frames` frames per call is allocated here.
 * Returns 0, a (negative) icer_status the reference would return for this geometry
 * (ICER_TOO_MANY_STAGES, ...), or ICER_FATAL_ERROR when no usable device exists.
 * Memory: about 14 bytes per sample and frame (coefficients, the stage-to-stage LL buffer, one event byte per sample and bit plane) plus
 * the coding units' slots.  Streams: an encoder owns a SIDE stream (a small kernel runs beside the main coder kernel of every launch)
 * -- a HIGH-priority stream unless GPU_MAX_HW_QUEUES >= 6 (it must not share the caller's hardware queue: INTEGRATION.md "Hardware
 * queues"; its kernels therefore go ahead of the program's normal-priority ones; ICER_HIP_STREAM_PRIO=0 makes it a plain stream) -- and,
 * with max_frames >= 4, a second plain stream for the second half of a synchronous batch call (icerx_encoder_parts). */
int icerx_encoder_create(icerx_encoder **enc, int device, size_t w, size_t h, int channels, int stages,
                         int filt, int segments, int max_frames);
/* The same with the sample width: sample_bits = 16 (as icerx_encoder_create) or 8 for the uint8 twins. */
int icerx_encoder_create_ex(icerx_encoder **enc, int device, size_t w, size_t h, int channels, int stages,
                            int filt, int segments, int max_frames, int sample_bits);
void icerx_encoder_destroy(icerx_encoder *enc);

/* Encode n_frames frames that already live in device memory.
 *   d_frames   device pointer, n_frames * channels planes of w*h uint16 (frame-major, then channel);
 *              not modified
 *   byte_quota per-frame byte quota (the reference's icer_output_data_buf_typedef.size_allocated)
 *   d_out      device pointer, n_frames * out_stride bytes; frame f's stream starts at f*out_stride
 *              (out_stride >= byte_quota)
 *   d_sizes    device pointer, n_frames uint64: stream lengths
 *   d_rcs      device pointer, n_frames int32: per-frame reference return codes
 *   stream     hipStream_t (as void*), NULL = default stream.  All work is enqueued on it; the call returns
 *              after it has completed there (it has to read back one word: whether a coding unit outgrew
 *              its provisioned slot, in which case the batch is redone with larger slots).
 * Returns 0 or ICER_FATAL_ERROR (HIP failure) / ICER_INVALID_INPUT. */
int icerx_encode_device(icerx_encoder *enc, const uint16_t *d_frames, int n_frames, size_t byte_quota,
                        uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream);

/* Rate ladder: the same frames at n_quotas byte quotas in one call, for about the cost of one call at the largest quota.
 * The quota only decides where a stream is cut (DESIGN.md 3 "Rate ladder"), so the batch is transformed and coded once,
 * planned as a call at the largest quota, and every quota's stream is cut from it.
 *   d_frames   as icerx_encode_device takes them (uint16 planes), or as icerx_encode_device_s8 (int8 storage) for an
 *              encoder created with sample_bits = 8; not modified
 *   quotas     HOST array of n_quotas byte quotas, 1 <= n_quotas <= ICERX_MAX_LADDER, in any order, repeats allowed
 *   d_out      device pointer, n_quotas * n_frames rows of out_stride bytes, quota-major: the stream of frame f at quota
 *              quotas[q] starts at d_out + ((size_t)q * n_frames + f) * out_stride; out_stride as icerx_encode_device
 *              requires it for the largest quota
 *   d_sizes    device pointer, n_quotas * n_frames uint64, entry q * n_frames + f
 *   d_rcs      device pointer, n_quotas * n_frames int32, entry q * n_frames + f
 * Quota q's block looks exactly like one icerx_encode_device output: icerx_decode_device_async takes it with d_offsets =
 * NULL, stream_stride = out_stride and d_lens = d_sizes + q * n_frames.  Every (f, q) has the bytes, size and return code
 * of icerx_encode_device (or _s8) on the same frames at quotas[q].  Synchronous, with the same re-runs as
 * icerx_encode_device.  Returns 0, ICER_INVALID_INPUT (nothing written: n_quotas or n_frames out of range, a null pointer,
 * an asynchronous encode pending, out_stride too small) or ICER_FATAL_ERROR (HIP failure). */
#define ICERX_MAX_LADDER 16
int icerx_encode_device_ladder(icerx_encoder *enc, const void *d_frames, int n_frames, const size_t *quotas, int n_quotas,
                               uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream);

/* Quality-targeted encode: every frame is cut where a distortion target is met, or at byte_cap if that comes first -- ICER's
 * two stopping rules.  The batch is transformed and coded once, planned as a call at byte_cap; one extra pass over the
 * coefficient planes gives every family -- a (channel, level, subband, segment) rectangle -- the squared error E[family][b]
 * that is left when its bit planes >= b are kept (b = 0 .. P, P = 9 coded planes, 7 for sample_bits = 8; the decoder rebuilds
 * magnitudes by truncation, so these are exact integers), and the frame's distortion after a prefix of its packets is
 *     D = sum over families of weight(filter, level, subband) * E[family][lowest plane kept, or P]  +  M
 * with the Q4 subband weights of csrc/subband_gain.hpp (the three channels of a YUV frame count equally).  M is what no packet
 * takes out: the packet header has ONE byte for a channel's LL mean (lib_icer's format), so a decoder gets every LL coefficient
 * of a 16-bit frame back short by (mean & 0xFF00); M = sum over LL families of weight * coefficients * (mean & 0xFF00)^2, and
 * 0 for frames whose LL means are below 256 and for sample_bits = 8.  D / 16 estimates the squared error of the decoded image.
 * Accuracy, measured against the reference decoder wherever the actual error is at least 1 per sample
 * (profiles/quality_target.md): within 6.0 dB in the worst case -- a lone large coefficient near the frame's edge, whose
 * weight differs from the subband's --, within about 1 dB where the error is made of many coefficients.  The inverse
 * transform's integer rounding is not modelled.
 * A stream keeps the shortest prefix of the packets in priority order with D <= T, T = icerx_target_threshold(target).
 *   d_frames      as icerx_encode_device_ladder takes them; not modified
 *   target_mse    HOST array of n_targets mean squared errors per sample, 1 <= n_targets <= ICERX_MAX_LADDER, in any order,
 *                 repeats allowed; T = floor(target_mse * w * h * channels * 16), saturated to 64 bits
 *   byte_cap      the byte quota no stream exceeds (plays the role of the ladder's largest quota; out_stride likewise)
 *   d_out, d_sizes, d_rcs   target-major exactly as the ladder's are quota-major: frame f at target t is row / entry
 *                 t * n_frames + f.  rc: ICER_BYTE_QUOTA_EXCEEDED when packets were left out, ICER_RESULT_OK otherwise
 *   d_reached     device pointer, n_targets * n_frames int32: 1 the target was met, 0 the byte cap ended the stream first
 *   d_dist        device pointer, n_targets * n_frames uint64: D of the stream
 *   d_equiv_quota device pointer, n_targets * n_frames uint64: a byte quota at which icerx_encode_device (or _s8, the
 *                 reference encoder, icerx_recut_device_async on a longer stream) produces this very stream
 * A frame without a stream (ICER_INTEGER_OVERFLOW) has d_reached 0, d_dist 0 and d_equiv_quota = byte_cap.  Synchronous, with
 * the same re-runs as the ladder.  Returns 0, ICER_INVALID_INPUT (nothing enqueued or written: n_targets or n_frames out of
 * range, a null pointer, a negative or NaN target, an asynchronous encode pending, out_stride too small, or a geometry
 * whose D could exceed 64 bits -- DESIGN.md 3 "Distortion target") or ICER_FATAL_ERROR (HIP failure).
 * The table E lives in encoder-owned device memory made by the first such call; an encoder that never makes one pays nothing.
 *
 * icerx_target_threshold: the integer T a target becomes for this encoder (0 for a negative or NaN target).
 * icerx_get_distortion_table: host copy of frame `frame`'s E of the last target call, n_entries = families * (P + 1) uint64,
 * entry family * (P + 1) + b, families in the order their first packet has in the priority order (M is not part of the table). */
int icerx_encode_device_target(icerx_encoder *enc, const void *d_frames, int n_frames, const double *target_mse, int n_targets,
                               size_t byte_cap, uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs,
                               int32_t *d_reached, uint64_t *d_dist, uint64_t *d_equiv_quota, void *stream);
uint64_t icerx_target_threshold(const icerx_encoder *enc, double target_mse);
int icerx_get_distortion_table(icerx_encoder *enc, int frame, uint64_t *dst, size_t n_entries);

/* Budget encode: n frames, B bytes in total, equally good.  The batch is transformed and coded once, exactly as
 * icerx_encode_device_target does at byte_cap, and the frames' streams are cut where ONE distortion threshold puts them:
 *   T* = the least T in [0, 2^64 - 1] at which the streams of all frames, each cut at the first packet prefix with D <= T or
 *        at byte_cap if that comes first, take at most B bytes together;
 *   then the bytes T* leaves over go to the frames in the order (D of the stream descending, frame ascending): each in turn is
 *   extended by as many whole packets as the rest of the budget and byte_cap allow.
 * So the sum of the sizes never exceeds B, no stream exceeds byte_cap, every frame that byte_cap did not stop has D <= T*, and
 * whenever byte_cap >= B / n_frames the largest D of the batch is no larger than the one icerx_encode_device leaves at the
 * quota B / n_frames for every frame (csrc/budget_core.hpp; tests/budget_model.py is the definition in plain integers).
 *   d_frames      as icerx_encode_device_ladder takes them; not modified
 *   budgets       HOST array of n_budgets byte budgets for the whole batch, 1 <= n_budgets <= ICERX_MAX_LADDER, in any order,
 *                 repeats allowed
 *   byte_cap      the byte quota no stream exceeds (out_stride as for the target call)
 *   d_out, d_sizes, d_rcs   budget-major exactly as the target call's are target-major: frame f at budget b is row / entry
 *                 b * n_frames + f.  rc: ICER_BYTE_QUOTA_EXCEEDED when packets were left out, ICER_RESULT_OK otherwise
 *   d_at_cap      device pointer, n_budgets * n_frames int32: 1 where the stream ends where byte_cap ends it
 *   d_dist        device pointer, n_budgets * n_frames uint64: D of the stream
 *   d_equiv_quota device pointer, n_budgets * n_frames uint64: a byte quota at which icerx_encode_device (or _s8, the
 *                 reference encoder, icerx_recut_device_async on a longer stream) produces this very stream
 *   d_threshold   device pointer, n_budgets uint64: T*
 *   d_total       device pointer, n_budgets uint64: the sum of the sizes
 * A frame without a stream (ICER_INTEGER_OVERFLOW) takes no bytes: size 0, d_at_cap 0, d_dist 0, d_equiv_quota = byte_cap.
 * Synchronous, with the same re-runs as the target call.  Returns 0, ICER_INVALID_INPUT (nothing enqueued or written:
 * n_budgets or n_frames out of range, a null pointer, an asynchronous encode pending, out_stride too small, or a geometry the
 * target call refuses) or ICER_FATAL_ERROR (HIP failure).  The frames' curves live in encoder-owned device memory made by the
 * first such call -- 16 bytes per packet and frame --; icerx_get_distortion_table serves the last target or budget call. */
int icerx_encode_device_budget(icerx_encoder *enc, const void *d_frames, int n_frames, const uint64_t *budgets, int n_budgets,
                               size_t byte_cap, uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs,
                               int32_t *d_at_cap, uint64_t *d_dist, uint64_t *d_equiv_quota, uint64_t *d_threshold,
                               uint64_t *d_total, void *stream);

/* Region-of-interest encode: a rate ladder whose byte quotas are spent inside a rectangle first.  Every other cut of this
 * library is a prefix of ICER's priority order, which spreads the bytes evenly over the picture.  The format allows more: a
 * packet names its own (channel, level, subband, bit plane, segment), a decoder files the packets it finds by those fields and
 * decodes each segment from its top plane down until one is missing, so a stream that keeps more bit planes of some segments
 * than of others is an ordinary ICER stream.  This call chooses WHICH packets are kept, never what a packet holds: every
 * output is a subset of the packets of the frame's lossless stream, byte for byte, in the usual final order.
 * The rule (tests/roi_model.py states it in plain integers; DESIGN.md 3 "Region of interest"):
 *   - a frame's rectangle (x, y, w, h) is read as uint32 and clipped to the frame: [x0, x1) x [y0, y1);
 *   - a coding unit of level l whose rectangle in its subband's own coordinates is [sx, sx + sw) x [sy, sy + sh) is FOREGROUND
 *     when it belongs to the LL subband (in every frame, so that the background stays a picture), or when the clipped
 *     rectangle is not empty and  sx < ceil(x1 / 2^l) + 2,  sx + sw + 2 > floor(x0 / 2^l)  and the same two hold in y
 *     (a guard of 2 coefficients).  All bit planes of a (channel, level, subband, segment) share a rectangle;
 *   - eff = priority << shift for foreground units, the packet's priority for the others; the ROI order sorts the units by eff
 *     descending, ties in priority order.  Within a family the planes stay in descending order: no hole above a kept plane.
 *     A frame whose clipped rectangle is empty has no region of interest: its shift is 0 and its order the priority order
 *     (with LL alone shifted, "no rectangle" would not be the plain stream);
 *   - the quota walk of icerx_encode_device (a unit is kept iff its 28 header bytes fit and floor(bits / 8) < quota - used -
 *     28; the first unit that fails ends the walk) runs over the units in ROI order and keeps the first K of it.
 * So shift = 0, an empty rectangle, one outside the frame, one whose foreground is every unit, and any encoder of one segment
 * give exactly icerx_encode_device_ladder's streams, and a quota that keeps every unit gives the lossless stream.
 *   d_frames     as icerx_encode_device_ladder takes them; not modified
 *   d_rois       DEVICE pointer, n_frames x 4 uint32: x, y, w, h of each frame's rectangle, read on `stream` (a tensor of
 *                boxes that a detector wrote on the same stream goes straight in; int32 values below 0 read as far outside)
 *   shift        0 <= shift <= ICERX_MAX_ROI_SHIFT: how many bit planes the foreground is put ahead
 *   quotas, d_out, out_stride, d_sizes, d_rcs   as the ladder's, quota-major; rc ICER_BYTE_QUOTA_EXCEEDED when K is less than
 *                the frame's units, else ICER_RESULT_OK
 *   d_kept       device pointer, n_quotas * n_frames uint32, entry q * n_frames + f: K
 *   d_foreground device pointer, n_frames uint32: the frame's foreground units
 * A frame without a stream (ICER_INTEGER_OVERFLOW) has size 0 and K 0.  Synchronous, with the same re-runs as the ladder.
 * Cost: a ROI cut is not a priority prefix, so the call codes EVERY unit whatever the quotas (the ladder stops coding once a
 * small largest quota is spent): at a small quota it costs about what a lossless call costs (profiles/roi.md).  Slots are
 * sized from the largest quota as for the ladder -- a unit that outgrows a quota-sized slot fits the stream in no order.
 * icerx_recut_device_async treats a ROI stream like a damaged one: a unit without a packet ends its walk, so a re-cut keeps
 * the priority prefix that is whole and drops what the ROI order had kept beyond it.
 * Returns 0, ICER_INVALID_INPUT (nothing enqueued or written: what the ladder refuses, a null d_rois, d_kept or d_foreground,
 * a shift outside 0 .. ICERX_MAX_ROI_SHIFT) or ICER_FATAL_ERROR (HIP failure).  The rank arrays live in encoder-owned device
 * memory made by the first such call -- 16 bytes per unit and frame, and 4 more per quota --; an encoder that never makes one pays
 * nothing. */
#define ICERX_MAX_ROI_SHIFT 16
int icerx_encode_device_roi(icerx_encoder *enc, const void *d_frames, int n_frames, const uint32_t *d_rois, int shift,
                            const size_t *quotas, int n_quotas, uint8_t *d_out, size_t out_stride, uint64_t *d_sizes,
                            int32_t *d_rcs, uint32_t *d_kept, uint32_t *d_foreground, void *stream);

/* The same call in two halves.  icerx_encode_device_async returns as soon as all work is enqueued on `stream`;
 * icerx_encoder_wait returns once it has completed there (re-running the batch in the rare cases the synchronous call
 * does: a coding unit that outgrew its slot, a unit time-out).  Between the two the caller may enqueue its own copies
 * on other streams or drive other encoders; the buffers passed in must stay valid and untouched until the wait returns.
 * At most one pending call per encoder (a second async call, or a synchronous one, returns ICER_INVALID_INPUT);
 * icerx_encoder_wait without a pending call returns 0. */
int icerx_encode_device_async(icerx_encoder *enc, const uint16_t *d_frames, int n_frames, size_t byte_quota,
                              uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream);
int icerx_encoder_wait(icerx_encoder *enc);

/* Front-end fusion: inputs as the reference's callers hold them BEFORE their app-side conversion,
 * converted on the device, so only 1 byte per sample crosses PCIe.
 *   icerx_encode_device_u8    8-bit gray frames (n_frames * w*h bytes), widened to the uint16 planes the uint16 API
 *                             takes -- what example/src/icer_util.c:163-168 does on the host.  channels must be 1.
 *   icerx_encode_device_rgb8  packed RGB888 frames (n_frames * w*h*3 bytes), converted to Y, Cb, Cr planes with the
 *                             integer formulas of the reference's callers (rgb888_packed_to_yuv,
 *                             example/src/icer_util.c:69-94 with CRGB2Y/Cb/Cr of example/inc/color_util.h:27-29).
 *                             channels must be 3.
 * Same outputs and return values as icerx_encode_device on the converted planes. */
int icerx_encode_device_u8(icerx_encoder *enc, const uint8_t *d_frames, int n_frames, size_t byte_quota, uint8_t *d_out,
                           size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream);
int icerx_encode_device_rgb8(icerx_encoder *enc, const uint8_t *d_rgb, int n_frames, size_t byte_quota, uint8_t *d_out,
                             size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream);

/* uint8 twins on device-resident planes (encoder created with sample_bits = 8): n_frames * channels planes of w*h
 * bytes (int8 storage), otherwise as icerx_encode_device. */
int icerx_encode_device_s8(icerx_encoder *enc, const uint8_t *d_planes, int n_frames, size_t byte_quota, uint8_t *d_out,
                           size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, void *stream);

/* Host-buffer convenience wrapper: H2D, icerx_encode_device, D2H, synchronous.  `out_stride` is the room of every
 * frame's row in `out`: a stream longer than that is not copied and the call returns ICER_OUTPUT_BUF_TOO_SMALL (sizes /
 * rcs are valid then); byte_quota or more always suffices. */
int icerx_encode_host(icerx_encoder *enc, const uint16_t *frames, int n_frames, size_t byte_quota,
                      uint8_t *out, size_t out_stride, uint64_t *sizes, int32_t *rcs);

/* A batch of frames of one geometry from host memory over the GPUs of the node (BASELINE configs 4 and 5): contiguous
 * blocks of frames per device, one host thread and one encoder per device, no communication between devices.  Every
 * device codes its block in sub-batches through three streams -- upload of sub-batch k+1, kernels of k, download of the
 * streams of k-1 at the same time -- so page-lock `frames` and `out` (icerx_pin_host) to let the copies run as DMA beside
 * the kernels.  The per-device encoders and staging buffers are kept between calls (re-made when the geometry changes);
 * icerx_batch_release frees them.
 * frames: n_frames x channels planes of w*h uint16; out: n_frames rows of out_stride bytes (a stream longer than
 * out_stride makes the call fail with ICER_OUTPUT_BUF_TOO_SMALL; byte_quota always suffices);
 * n_gpus: devices to use (0 = all present; clamped to the number present and to n_frames) -- devices 0 .. n_gpus-1; the
 * _devices variant names them (one process per GPU: pass that process's device).  sizes / rcs per frame equal a
 * per-frame call of icer_compress_image_[yuv_]uint16 (reference: icer.h:440-444).  Returns 0, or the first failing
 * device's error code (icerx_last_error lists every failing device).
 * Env: ICER_HIP_BATCH_SUB=<frames per sub-batch>, ICER_HIP_NUMA=0 (do not pin the per-device host threads to their GPU's NUMA node).
 * The pipeline keeps six streams per device busy.  With GPU_MAX_HW_QUEUES=8 exported before the process initialises HIP they
 * are plain streams (0.94 x the device-resident rate); with fewer hardware queues the encoders' streams are created at the low
 * priority level -- a queue pool of their own: the same 0.94 x whatever else the process has alive, and the program's own kernels
 * go first (ICER_HIP_STREAM_PRIO=0|1 pins the choice; the library does not touch the environment) -- INTEGRATION.md "Hardware queues".
 *
 * icerx_device_count(): devices the batch calls and icerx_encoder_create accept (0 .. count-1).  ICER_HIP_VIRTUAL_DEVICES=<N>
 * makes that N LOGICAL devices mapped round-robin onto the physical ones: a dry run of every multi-device code path (N host
 * threads, N pooled pipelines, error aggregation) on a node with fewer GPUs; streams are unaffected. */
int icerx_device_count(void);
int icerx_compress_batch_uint16(const uint16_t *frames, int n_frames, size_t w, size_t h, int channels, int stages, int filt,
                                int segments, size_t byte_quota, uint8_t *out, size_t out_stride, uint64_t *sizes, int32_t *rcs,
                                int n_gpus);
int icerx_compress_batch_uint16_devices(const uint16_t *frames, int n_frames, size_t w, size_t h, int channels, int stages, int filt,
                                        int segments, size_t byte_quota, uint8_t *out, size_t out_stride, uint64_t *sizes, int32_t *rcs,
                                        const int *devices, int n_devices);
void icerx_batch_release(void);

/* Optional: page-lock a caller buffer that icerx_encode_host / the lib_icer-shaped entry points read frames from or
 * write streams to, so that it crosses PCIe by DMA at link speed (otherwise the runtime stages pageable memory through
 * its own pinned buffers, about 4x slower).  Unpin before freeing the memory.  Returns 0 or ICER_FATAL_ERROR. */
int icerx_pin_host(void *ptr, size_t bytes);
int icerx_unpin_host(void *ptr);

/* Copy the sign-magnitude coefficient plane of (frame, channel) of the last encode to host
 * memory (what the reference leaves in the caller's image buffer). */
int icerx_get_coefficients(icerx_encoder *enc, int frame, int channel, uint16_t *dst);

/* Kernel timing with HIP events on the encode stream.  When enabled, every icerx_encode_device
 * call records events around each pipeline stage; icerx_timing_read synchronises and accumulates.
 * stage ids: 0 = DWT (all stages), 1 = LL mean + sign-magnitude, 2 = coding units (dominant),
 * 3 = quota scan + stream gather.  ms[i] = accumulated milliseconds, calls = number of encodes. */
#define ICERX_NUM_STAGES 4
int icerx_timing_enable(icerx_encoder *enc, int on);
int icerx_timing_read(icerx_encoder *enc, double ms[ICERX_NUM_STAGES], uint64_t *calls, int reset);

/* Number of coding units per frame and the bits-per-pixel slot bound currently in use. */
int icerx_info(icerx_encoder *enc, uint32_t *units_per_frame, uint32_t *slot_bits_per_pixel, uint64_t *slot_bytes_per_frame);

/* Event counters of an encoder since its creation: out[0] = coding units that gave up waiting for a hand-off of the
 * eight-wave pipeline (bounded spins; expected 0), out[1] = batches coded again by the barrier-only workgroup coder
 * because of that (the caller still gets its result), out[2] = batches re-run with larger per-unit slots,
 * out[3] = coder selection in force (0 automatic, 1 pipeline only, 2 workgroup coder only; env ICER_HIP_CODER=pipe|wg).
 * Automatic: the wave pipeline; the workgroup coder for byte quotas below half a byte per sample (progressive mode);
 * in launches of two or more planes (frames x channels), and of one gray frame whose dense units are cut into sub-ranges
 * (icerx_encoder_launch_info), the coding units with >= 95 % (90 %) blank chunks go to a small instance of the workgroup coder
 * (one wave per workgroup in a batch, four for a lone frame; ICER_HIP_LIST_WAVES=1|2|4), which runs beside the pipeline kernel (env ICER_HIP_HYBRID=<percent, 0 = off>, ICER_HIP_HYBRID_FRAMES=<n>).
 * None of this changes a byte of the streams. */
int icerx_encoder_stats(icerx_encoder *enc, uint64_t out[4]);
/* out[0] = coding units (summed over frames and calls) that went to the workgroup coder's small instance beside the
 * pipeline kernel, out[1] = encode calls in which that routing was active (see above: launches of >= 2 planes). */
int icerx_encoder_routing(icerx_encoder *enc, uint64_t out[2]);
/* The shape of the encoder's last launch: out[0] = 1 if its dense coding units were cut into sub-ranges coded by a workgroup
 * each (launches of a single gray frame: the chip has more compute units than such a frame has large units;
 * env ICER_HIP_SPLIT=<chunks per sub-range, 0 = off>), out[1] = those extra workgroups, out[2] = wavefronts per workgroup of
 * the pipeline kernel (8 or 11; 0: the workgroup coder alone), out[3] = 1 if all-but-blank units went to the window coder
 * beside it.  None of this changes a byte of the streams. */
int icerx_encoder_launch_info(icerx_encoder *enc, uint32_t out[4]);
/* Parts the encoder's last call was enqueued in.  A SYNCHRONOUS batch call of four frames or more (icerx_encode_device and the _u8 / _rgb8 /
 * _s8 twins; not progressive mode) enqueues its frames in two parts, the second on a stream of the encoder's own that starts behind
 * whatever `stream` holds and is joined back before the call's own work on `stream` ends: a part's transform and event pass run beside
 * the other part's coder kernels.  The asynchronous calls enqueue one part (their caller overlaps whole batches).  env
 * ICER_HIP_OVERLAP_PARTS=<1..4> (1: off).  None of this changes a byte of the streams. */
int icerx_encoder_parts(icerx_encoder *enc);
/* out[0..2] summed over all encoders of the process, including the one behind the lib_icer-shaped entry points */
int icerx_process_stats(uint64_t out[4]);

/* ---- Standalone wavelet transform, forward (lib_icer/inc/icer.h:392-395, :446-449, :434-435) ----------------------
 * Same names, signatures, return codes and in-place effects as lib_icer (icer_wavelet.c): the caller's buffer and the
 * return code after a call equal the reference's, ICER_INTEGER_OVERFLOW included (the transform keeps going and stores
 * wrapped int16 / int8 values, as the reference does), and the uint8 twins work on int8 storage with int8 limits.
 *   _stages   image_w x image_h, contiguous; ICER_TOO_MANY_STAGES (buffer untouched) when the smallest LL would have a
 *             side below 3; no ICER_MAX_DECOMP_STAGES cap.
 *   _2d       one level on image_w x image_h samples of a plane with `rowstride`; samples beyond image_w stay untouched.
 *   _1d       N samples `stride` apart; only those are read or written.  Gathered and scattered with a 2-D copy: this
 *             call exists for completeness, not speed.
 * A line shorter than 2 samples (image_w, image_h or N < 2) returns ICER_INVALID_INPUT with the data untouched (the
 * reference loops through SIZE_MAX there).  The transform runs on the GPU (device ICER_HIP_DEVICE, default 0); the calls
 * are serialised like the other lib_icer-shaped entry points.
 * icer_to_sign_magnitude_int16 / _int8 are host-only bit manipulation on caller memory.
 * Not provided (in-place shuffles only lib_icer itself calls, or functions on lib_icer's internal context structs):
 * interleave / deinterleave / reverse / remove_negative, the partition, bitplane, entropy-coder and packet functions,
 * and the dimension helpers. */
int icer_wavelet_transform_stages_uint16(uint16_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt);
int icer_wavelet_transform_2d_uint16(uint16_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt);
int icer_wavelet_transform_1d_uint16(uint16_t *data, size_t N, size_t stride, enum icer_filter_types filt);
int icer_wavelet_transform_stages_uint8(uint8_t *image, size_t image_w, size_t image_h, uint8_t stages, enum icer_filter_types filt);
int icer_wavelet_transform_2d_uint8(uint8_t *image, size_t image_w, size_t image_h, size_t rowstride, enum icer_filter_types filt);
int icer_wavelet_transform_1d_uint8(uint8_t *data, size_t N, size_t stride, enum icer_filter_types filt);
void icer_to_sign_magnitude_int16(uint16_t *data, size_t len);
void icer_to_sign_magnitude_int8(uint8_t *data, size_t len);

/* Device-resident batch transform (the path the calls above wrap).  d_planes: n_planes planes of w*h samples (row stride
 * w; uint16 for sample_bits 16, int8 bytes for 8), plane k at d_planes + k*plane_stride samples, transformed in place
 * with `stages` levels of filter `filt`.  Everything is enqueued on `stream` (a hipStream_t; 0 = the null stream) with no
 * host synchronisation; d_rcs[k] (device memory) receives ICER_RESULT_OK or ICER_INTEGER_OVERFLOW for plane k on the
 * stream.  The call itself returns ICER_TOO_MANY_STAGES / ICER_INVALID_INPUT (also for n_planes above 65535) before enqueuing anything, or
 * ICER_FATAL_ERROR on a HIP failure.  d_workspace: icerx_wavelet_workspace_bytes(w, h, n_planes, sample_bits) bytes of
 * device memory owned by the caller, not used by another call until this one has completed on the stream.  The inverse,
 * icerx_wavelet_inverse_device, is in libicer_hip_dec.so. */
size_t icerx_wavelet_workspace_bytes(size_t w, size_t h, int n_planes, int sample_bits);
int icerx_wavelet_forward_device(void *d_planes, int n_planes, size_t w, size_t h, size_t plane_stride, int stages, int filt,
                                 int sample_bits, void *d_workspace, int32_t *d_rcs, void *stream);

const char *icerx_last_error(void);

/* The distortion sidecar -- a frame's energy table and LL means in device memory, stored beside its master so that
 * libicer_hip_dec.so can re-cut the master to a distortion target or a shared byte budget: icerx_distortion_sidecar_entries,
 * icerx_get_distortion_sidecar_device.  Declared and described in icer_hip_sidecar.h. */
#define ICER_HIP_H_SIDECAR_PART 1
#include "icer_hip_sidecar.h"
#undef ICER_HIP_H_SIDECAR_PART

#ifdef __cplusplus
}
#endif
#endif /* ICER_HIP_H */
