/* icer_hip_dec_quality.h -- quality-driven re-cuts of libicer_hip_dec.so.  A PART of icer_hip_dec.h, which includes it inside
 * its extern "C" block and behind its types: it has no includes of its own and refuses to be included alone.  Include
 * icer_hip_dec.h.
 *
 * ---- Re-cutting to a distortion target or a shared byte budget ---------------------------------------------------------
 * icerx_encode_device_target and icerx_encode_device_budget (icer_hip.h) cut a coded batch where a distortion target is met,
 * or so that its frames share a byte budget at equal distortion.  Where those cuts fall depends on the units' payload bits --
 * a stored master's packet table has them -- and on the frame's distortion sidecar (icer_hip_sidecar.h), stored beside the
 * master.  The two calls below make the same cuts from masters and sidecars, without the pixels and without re-coding.
 *
 * A QUALITY RECUTTER knows the filter the masters were made with: icerx_recutter_create_quality behaves as
 * icerx_recutter_create_reduced, every other recut or combine call works on it unchanged, and it also holds, for each geometry
 * r = 0 .. max_reduce, every family's weight (level lv of the geometry at 1/2^r size weighted as that level of an encoder of
 * that geometry), LL term and channel, and for r > 0 the map from that geometry's families to the master's.  It returns
 * ICER_INVALID_INPUT, beyond what icerx_recutter_create_reduced refuses, for a filter outside 0 .. 6, a geometry whose
 * distortion can leave 64 bits (the encoder's bound, with LL means of up to 0xFF00 since a stored sidecar may hold anything),
 * and, with max_reduce > 0, a geometry where a subband has fewer samples than segments (the planes of one chain can then code
 * different rectangles, and the families of a reduced geometry are not families of the master).
 * icerx_recut_sidecar_entries: the uint64 words of a sidecar row, equal to icerx_distortion_sidecar_entries of an encoder of
 * the geometry; 0 for NULL or a plain recutter.
 * icerx_recut_target_threshold: floor(mse * rw * rh * channels * 16) saturated to 64 bits, rw x rh the size at 1/2^reduce; 0
 * for a negative or NaN mse, a reduce out of range or NULL.  At reduce 0 it is icerx_target_threshold of such an encoder.
 *
 * DEFINITION.  For frame f and a cut at reduce r:
 *   1. the master is walked as by every recut call; a frame has the status it has there (ICER_INVALID_INPUT,
 *      ICER_DECODER_OUT_OF_DATA, no valid packet above level r);
 *   2. the bit counts are taken in the unit order of the geometry at 1/2^r size, a unit without a packet "does not fit";
 *   3. D_0 = sum over that geometry's families g of weight_g * E[fam(g)][P] + ll_term_g * (mean & 0xFF00)^2, and unit k of
 *      family g and bit plane lsb takes D_{k+1} = D_k - weight_g * (E[fam(g)][lsb + 1] - E[fam(g)][lsb]), with E and the means
 *      from row f of the sidecar;
 *   4. target call: the cut is the first k with D_k <= T (T = icerx_recut_target_threshold(r, target_mse[c], reduces[c])), or
 *      where the byte cap ends the quota walk, as in icerx_encode_device_target;
 *   5. budget call: the cuts of the call's frames are those of icerx_encode_device_budget -- the least common threshold whose
 *      streams fit the budget, then the rest handed out in the order (D descending, frame ascending);
 *   6. a frame with a status is a frame without a stream: it takes no bytes of a budget, size 0, reached / at_cap 0, dist 0,
 *      equiv = byte_cap, and its rc is the status;
 *   7. the kept packets are copied as by icerx_recut_device_cuts_async, with the header of the derived stream at r.
 * Consequences:
 *   - r = 0, masters that are complete or made at a cap not below byte_cap: every output -- streams, sizes, rcs, reached /
 *     at_cap, dist, equiv, threshold, total -- equals what icerx_encode_device_target / _budget give on the original frames
 *     with the same targets / budgets and cap, byte for byte and word for word.  (One corner: where the cut lands on a unit
 *     whose payload alone exceeds byte_cap, the encoder has no bit count for it and reports byte_cap as d_equiv_quota; a
 *     complete master has the count, and the quota reported here is used + 28 + bits / 8.  Both make the same stream.)
 *   - d_equiv_quota is a byte quota at which icerx_recut_device_async (r = 0) or icerx_recut_device_cuts_async (r > 0) on the
 *     same master makes that very stream.
 *   - a sidecar row is stored data: a frame whose row of E is not non-decreasing in b for some family, or whose E[g][P]
 *     exceeds coefficients_g * max_mag^2 (max_mag 32767; 128 for 8-bit samples), gets ICER_INVALID_INPUT and no stream, and
 *     its neighbours are untouched.  With the bound checked at creation, no sum of the curve can overflow or run backwards.
 * Arguments: masters, d_out / out_stride / d_sizes / d_rcs (row and entry c * n + f) as icerx_recut_device_cuts_async.
 * d_sidecar: DEVICE memory, row f at d_sidecar + f * sidecar_stride words.  `reduces` (NULL: every reduce 0), `target_mse`,
 * `budgets`: HOST arrays of n_cuts / n_budgets entries (1 .. ICERX_MAX_LADDER), passed by value; the budget call has one
 * reduce for all its budgets.  d_reached / d_at_cap, d_dist, d_equiv_quota: n_cuts * n entries; d_threshold, d_total:
 * n_budgets entries.  The whole call returns ICER_INVALID_INPUT -- nothing enqueued, nothing written -- for a plain
 * recutter, a null pointer (d_offsets, reduces and `stream` excepted), n outside 1 .. 65535, n_cuts / n_budgets outside
 * 1 .. 16, a reduce outside 0 .. max_reduce, a negative or NaN target, out_stride < byte_cap, sidecar_stride below the
 * entries, or a workspace below icerx_recut_*_workspace_bytes (the cuts call's, and per frame a record, 8 bytes per family
 * and plane of every geometry, and for the budget call 16 bytes per unit and 48 per budget); ICER_FATAL_ERROR for data_bytes
 * past the 32-bit limit.  Stream-ordered with every promise of the other recut calls: no blocking copy, no synchronisation,
 * no hipMalloc / hipFree, every check before the first launch. */
#ifndef ICER_HIP_DEC_QUALITY_H
#define ICER_HIP_DEC_QUALITY_H
#ifndef ICER_HIP_DEC_H_QUALITY_PART
#error "icer_hip_dec_quality.h is a part of icer_hip_dec.h: include icer_hip_dec.h"
#endif

int icerx_recutter_create_quality(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, int filt,
                                  unsigned segments, int sample_bits, int max_reduce);
size_t icerx_recut_sidecar_entries(const icerx_recutter *r);
uint64_t icerx_recut_target_threshold(const icerx_recutter *r, double target_mse, int reduce);

size_t icerx_recut_target_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts);
int icerx_recut_device_target_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                    size_t stream_stride, const uint64_t *d_lens, const uint64_t *d_sidecar,
                                    size_t sidecar_stride, const int *reduces, const double *target_mse, int n_cuts,
                                    size_t byte_cap, uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs,
                                    int32_t *d_reached, uint64_t *d_dist, uint64_t *d_equiv_quota, void *d_workspace,
                                    size_t workspace_bytes, void *stream);

size_t icerx_recut_budget_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_budgets);
int icerx_recut_device_budget_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                    size_t stream_stride, const uint64_t *d_lens, const uint64_t *d_sidecar,
                                    size_t sidecar_stride, int reduce, const uint64_t *budgets, int n_budgets, size_t byte_cap,
                                    uint8_t *d_out, size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, int32_t *d_at_cap,
                                    uint64_t *d_dist, uint64_t *d_equiv_quota, uint64_t *d_threshold, uint64_t *d_total,
                                    void *d_workspace, size_t workspace_bytes, void *stream);

#endif
