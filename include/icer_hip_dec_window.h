/* icer_hip_dec_window.h -- the window decode of libicer_hip_dec.so.  A PART of icer_hip_dec.h, which includes it inside its
 * extern "C" block and behind its types: it has no includes of its own and refuses to be included alone.  Include icer_hip_dec.h.
 *
 * ---- Window decode: a rectangle of each image, without the chains it does not depend on ----------------------------------
 * Every frame of a batch has a rectangle (x, y, w, h) in pixels of the image the decoder delivers (for a reduced decoder:
 * of the reduced image).  The call delivers that rectangle only, stored compactly, and runs only the entropy chains (one
 * segment of one subband) the rectangle depends on.
 *
 * The result, exactly:
 *   - the rectangle clipped to the image is [x0, x0 + ww) x [y0, y0 + wh);
 *   - the window image is the crop of what the plain call of the same decoder (same reduce, reconstruction eighths, sample
 *     width; planes or display) delivers for the same stream, with working planes of full_stride samples where the plain call
 *     has frame_stride: bit for bit, whatever the return code -- damaged and truncated streams, and frames that stop before
 *     the transform (the crop of the sign-magnitude words the plain call leaves);
 *   - rcs / ws / hs are the plain call's, with one addition: a clipped window of more than frame_stride samples gives that
 *     frame ICER_BYTE_QUOTA_EXCEEDED, and nothing is written for it;
 *   - an empty clipped window writes nothing.  A frame the plain call delivers nothing for has an empty window.
 *
 * Layout.  Planes: channel c of frame k at d_out + (k * channels + c) * frame_stride samples (planes_out[k * channels + c]
 * for the host call), sample (x, y) of the window at y * ww + x.  Display: frame k at d_out + k * channels * frame_stride
 * bytes, pixel (x, y) at channels * (y * ww + x).  Nothing else of `out` is written.
 *
 * info: 6 uint32 per frame -- x0, y0, ww, wh of the clipped window, the chains run, the chains the plain call runs.
 *
 * Which chains run.  For a line of n stored samples (nl = ceil(n / 2) lows, nh = floor(n / 2) highs) whose restored samples
 * [a, b) are wanted, with ka = a >> 1 and kb = (b - 1) >> 1:
 *   whole line   n < 8, or an odd line of an 8-bit decoder (whose positions are not the plain interleave): everything
 *   filter A     highs [ka, min(kb, nh - 1)], lows [max(ka - 1, 0), min(kb + 1, nl - 1)]
 *   other        highs [ka, nh - 1], lows [max(ka - 2, 0), nl - 1]  (a restored high needs the next one: the dependence
 *                runs to the end of the line, so a bottom-right window saves and a top-left one does not)
 * Per level, for the wanted rectangle X x Y: LL needs lows(X) x lows(Y), HL highs(X) x lows(Y), LH lows(X) x highs(Y), HH
 * highs(X) x highs(Y); the rectangle needed of LL is the wanted rectangle of the next deeper level.  A chain runs when its
 * segment's rectangle meets the needed rectangle of its subband.  A frame that does not reach the transform (a segment-grid
 * error), or whose deepest LL is thinner than 3, keeps all its chains.
 *
 * The synchronous calls take `windows` as a HOST array of n x 4 uint32 and fill host rcs / ws / hs / info; their full-size
 * working planes are the decoder's own.  The asynchronous calls read d_windows (DEVICE memory, n x 4 uint32) on `stream` and
 * keep every stream-ordered promise of icerx_decode_device_async: no blocking copy, no synchronisation, no allocation; the
 * working planes live in the workspace.  A null argument gives ICER_INVALID_INPUT with nothing enqueued or written. */
#ifndef ICER_HIP_DEC_WINDOW_H
#define ICER_HIP_DEC_WINDOW_H
#ifndef ICER_HIP_DEC_H_WINDOW_PART
#error "icer_hip_dec_window.h is a part of icer_hip_dec.h: include icer_hip_dec.h"
#endif

int icerx_decode_host_window(icerx_decoder *dec, int n, const uint8_t *data, const size_t *offsets, const size_t *lens,
                             const uint32_t *windows, void *const *planes_out, size_t frame_stride, size_t full_stride, int *rcs,
                             size_t *ws, size_t *hs, uint32_t *info);
int icerx_decode_device_window(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                               const uint32_t *windows, void *d_out, size_t frame_stride, size_t full_stride, int *rcs, size_t *ws,
                               size_t *hs, uint32_t *info);
int icerx_decode_device_window_display(icerx_decoder *dec, int n, const void *d_data, const size_t *offsets, const size_t *lens,
                                       const uint32_t *windows, uint8_t *d_out, size_t frame_stride, size_t full_stride, int *rcs,
                                       size_t *ws, size_t *hs, uint32_t *info);

size_t icerx_decode_window_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t full_stride);
int icerx_decode_device_window_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                     size_t stream_stride, const uint64_t *d_lens, const uint32_t *d_windows, void *d_out,
                                     size_t frame_stride, size_t full_stride, int32_t *d_rcs, uint64_t *d_ws, uint64_t *d_hs,
                                     uint32_t *d_info, void *d_workspace, size_t workspace_bytes, void *stream);
size_t icerx_decode_window_display_workspace_bytes(const icerx_decoder *dec, int n, size_t data_bytes, size_t full_stride);
int icerx_decode_device_window_display_async(icerx_decoder *dec, int n, const void *d_data, size_t data_bytes,
                                             const uint64_t *d_offsets, size_t stream_stride, const uint64_t *d_lens,
                                             const uint32_t *d_windows, uint8_t *d_out, size_t frame_stride, size_t full_stride,
                                             int32_t *d_rcs, uint64_t *d_ws, uint64_t *d_hs, uint32_t *d_info, void *d_workspace,
                                             size_t workspace_bytes, void *stream);

/* the one-shot call, shaped like icerx_decompress_reconstructed: planes[c] host memory of bufsize samples for the window;
 * window = x, y, w, h; info = 6 uint32 as above.  The working planes are sized by the image the stream's first valid packet
 * announces (icer_get_image_dimensions), at the decoder's resolution. */
int icerx_decompress_window(void *const planes[], int channels, size_t *image_w, size_t *image_h, size_t bufsize,
                            const uint8_t *datastream, size_t data_length, int stages, int filt, unsigned segments, int sample_bits,
                            int reduce, int eighths, const uint32_t *window, uint32_t *info);

#endif
