/* icer_hip_dec_session.h -- progressive decode sessions of libicer_hip_dec.so.  A PART of icer_hip_dec.h, which includes it
 * inside its extern "C" block and behind its types: it has no includes of its own and refuses to be included alone.  Include
 * icer_hip_dec.h.
 *
 * ---- Decode sessions: refine held images from new packets ------------------------------------------------------------------
 * The holder of a cut who receives an increment (icerx_combine_device_async, ICERX_COMBINE_DIFFERENCE) need not decode the
 * planes it has decoded before.  A session keeps, per frame ("slot"), the sign-magnitude words of every coefficient on the
 * device; a feed decodes only the bit planes its packets add and delivers the whole refined image.
 *
 * A session belongs to one decoder and takes its channels, stages, filter, segments, sample width, reduce and -- read at
 * every feed -- its reconstruction setting.  It holds n_slots frames of frame_stride samples per channel.  The decoder must
 * outlive the session; the session is as little thread-safe as the decoder, and its calls are synchronous like
 * icerx_decode_device.
 *
 * The definition (tests/session_model.py states it in Python).  A slot keeps a set T of accepted packets, keyed by
 * (channel, level, subband, segment, bit plane), the image size and the LL means.
 *   - A feed is walked on its own by the decoder's cursor rule: both CRCs must hold, an accepted packet is stepped over
 *     whole, the last packet of a kind wins; for a reduced decoder packets of level <= reduce move the cursor and nothing
 *     else.  Packets that name no entry of the decoder's table are dropped.
 *   - Size and means are those of the packets in T: a slot learns them from the first feed of which it accepts a packet (the
 *     mean of a channel: a packet of that channel).  A feed with a packet whose image size differs from the slot's (not yet
 *     known: from that of the feed's first packet), or whose LL mean differs from the slot's mean of that channel (not yet
 *     known: from the feed's first packet of that channel), is REFUSED for that frame: its rc is ICER_INVALID_INPUT, the slot
 *     is untouched and nothing is written for its row; ws / hs report the slot's size.  The same holds, with
 *     ICER_BYTE_QUOTA_EXCEEDED, for an image of more than frame_stride samples.
 *   - For every chain (one segment of one subband of one channel) the feed contributes the planes next, next - 1, ... for as
 *     long as it has them; next is one below the chain's lowest held plane, the top plane for a chain that holds none.
 *     Everything else is dropped and counted: planes already held, planes below a gap, packets of a stopped chain.
 *   - If the entropy decode of a plane fails, the chain has stopped for good, as in the plain decoder, which never starts the
 *     planes below a failed one: the failed packet stays in T, the planes of the feed below it do not enter T, and later
 *     packets of the chain are dropped.
 *   - The image, the size and the rc of a fed frame are those of the plain decode (icerx_decode_device /
 *     icerx_decode_host / icerx_decode_device_display of the same decoder, its reconstruction setting included) of the
 *     packets of T as one stream.  Every feed delivers the whole image, not a delta.  So a held cut A followed by
 *     DIFFERENCE(A, B) gives the plain decode of UNION(A, B): of B for nested cuts.  (The caveat of the increments applies: a
 *     chain that reads on past its own payload -- the reference has no end-of-packet check -- decodes by the bytes that happen
 *     to follow each packet, in a session as in any decoder.)
 *
 * Arguments.  slots[k] names the frame that feed k refines; the entries are distinct and in [0, n_slots); NULL means
 * 0 .. n - 1.  Feed k is the bytes [offsets[k], offsets[k] + lens[k]) of data; an empty feed delivers the image of the
 * state again.  Row k of the output holds slot slots[k], in the layout of the plain call of the same kind for n frames.  rcs,
 * ws, hs are per fed frame; the in-values of ws and hs are used only while the slot has seen no valid packet.  A call that
 * returns ICER_FATAL_ERROR (icerx_decoder_last_error) has reset the slots it was feeding.
 *
 * Which kernel runs a chain.  A feed routes like the plain decode and honours ICER_DEC_WAVE, read at every feed: unset, the
 * chains whose packets all take the fast entropy path run in the wave-per-plane kernel while the call brings at most 12 of them
 * per compute unit (the others, chains with a packet below 16 bits, then take one thread each), and above that load every
 * chain runs in the lane-per-plane kernel, which resumes over a row ring loaded from the state; 0 pins one thread per chain, 1 the lane-per-plane kernel, 2 the wave-per-plane kernel where it applies.  A chain
 * whose ring does not fit the lane-per-plane kernel's LDS runs on a thread.  The images do not depend on the route.
 *
 * Not here: the stream-ordered, device-planned twin (*_async) -- the next step, which wants the chain table on the device --
 * and window sessions. */
#ifndef ICER_HIP_DEC_SESSION_H
#define ICER_HIP_DEC_SESSION_H
#ifndef ICER_HIP_DEC_H_SESSION_PART
#error "icer_hip_dec_session.h is a part of icer_hip_dec.h: include icer_hip_dec.h"
#endif

typedef struct icerx_session icerx_session;

int icerx_session_create(icerx_session **out, icerx_decoder *dec, int n_slots, size_t frame_stride);
void icerx_session_destroy(icerx_session *s);
/* forget everything slot `slot` holds (-1: every slot) */
int icerx_session_reset(icerx_session *s, int slot);

int icerx_session_feed_host(icerx_session *s, int n, const int *slots, const uint8_t *data, const size_t *offsets, const size_t *lens,
                            void *const *planes_out, int *rcs, size_t *ws, size_t *hs);
int icerx_session_feed_device(icerx_session *s, int n, const int *slots, const void *d_data, const size_t *offsets, const size_t *lens,
                              void *d_out, int *rcs, size_t *ws, size_t *hs);
int icerx_session_feed_device_display(icerx_session *s, int n, const int *slots, const void *d_data, const size_t *offsets,
                                      const size_t *lens, uint8_t *d_out, int *rcs, size_t *ws, size_t *hs);

/* the planes the chain (chan, level, subband, segment) of a slot holds, counted from the top; level as the packets' headers
 * name it.  -1: the chain has stopped for good.  -2: no such slot or chain. */
int icerx_session_planes_held(const icerx_session *s, int slot, int chan, int level, int subband, int segment);
/* four counts since creation: chains resumed in the wave-per-plane kernel (a loader wave ran), chains run in the
 * thread-per-chain kernel, planes decoded, packets dropped */
int icerx_session_stats(const icerx_session *s, uint64_t out[4]);

#endif
