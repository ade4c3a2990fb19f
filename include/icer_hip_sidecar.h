/* icer_hip_sidecar.h -- the distortion sidecar of libicer_hip.so.  A PART of icer_hip.h, which includes it inside its
 * extern "C" block and behind its types: it has no includes of its own and refuses to be included alone.  Include icer_hip.h.
 *
 * ---- The distortion sidecar ---------------------------------------------------------------------------------------------
 * Where a quality-targeted or a budget cut falls is a function of two things: the payload bits of the frame's packets, which
 * a stored stream carries, and the frame's residual-energy table E[family][b] with its LL means ("Quality-targeted encode"
 * above), which it does not.  The sidecar is that second part, in device memory, one row per frame:
 *     entries 0 .. n_families * (P + 1) - 1    E, exactly as icerx_get_distortion_table lays it out
 *     the last entry                           the frame's full 16-bit LL means: channel c in bits 16 c .. 16 c + 15, unused
 *                                              channels zero
 * Stored beside a master (a stream made at a generous byte cap, e.g. by a target call at target 0), it lets
 * icerx_recut_device_target_async / icerx_recut_device_budget_async of libicer_hip_dec.so (icer_hip_dec_quality.h) make
 * the cuts of icerx_encode_device_target / icerx_encode_device_budget from the master, without the pixels.
 *
 * icerx_distortion_sidecar_entries: n_families * (P + 1) + 1, the uint64 words of a row; 0 for NULL.
 * icerx_get_distortion_sidecar_device: rows 0 .. n_frames - 1 of the last target or budget call (both are synchronous, so
 * the tables are complete), row f to d_dst + f * stride_entries.  One kernel enqueued on `stream` (a hipStream_t): no host
 * copy, no allocation, no synchronisation, and nothing written outside the `entries` words of each row.  ICER_INVALID_INPUT,
 * with nothing enqueued or written, when the encoder has made no target or budget call yet, n_frames is outside 1 .. the
 * frames of that call, stride_entries is below the entries, or a pointer is null.  A frame that call dropped
 * (ICER_INTEGER_OVERFLOW) gets the row the encoder holds for it; its master is empty. */
#ifndef ICER_HIP_SIDECAR_H
#define ICER_HIP_SIDECAR_H
#ifndef ICER_HIP_H_SIDECAR_PART
#error "icer_hip_sidecar.h is a part of icer_hip.h: include icer_hip.h"
#endif

size_t icerx_distortion_sidecar_entries(const icerx_encoder *enc);
int icerx_get_distortion_sidecar_device(icerx_encoder *enc, int n_frames, uint64_t *d_dst, size_t stride_entries, void *stream);

#endif
