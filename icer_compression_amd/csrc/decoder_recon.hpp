// decoder_recon.hpp -- reconstruction of truncated coefficients inside their interval (include/icer_hip_dec.h,
// icerx_decoder_set_reconstruction).  Included by decoder.hip after its kernels (it needs FrameInfo).
//
// A chain whose lowest p bit planes never arrived leaves every coefficient at the low end m of its interval
// [m, m + 2^p - 1], as lib_icer does (icer_context_modeller.c, `*pos |= bit << lsb`).  With the decoder's setting k in 1..4
// every NON-ZERO magnitude of such a chain gets off(p, k) = (k * (2^p - 1)) >> 3 on top: k eighths of the way into the
// interval.  The rule, exact and in integers:
//   P       coded planes, 9 (16-bit decoder) or 7 (8-bit)
//   t       packets present consecutively from plane P - 1 downwards (ChainDesc::pkt, the planes the chain runs); p = P - t.
//           p is the planner's figure: a packet whose decode stops early inside still counts
//   words   every sign-magnitude word of the chain's rectangle with a non-zero magnitude: magnitude + off(p, k).  The bits
//           below p are zero, so nothing carries into the sign; zero magnitudes (with or without a set sign bit) and the sign
//           stay.  LL chains as well.  Only frames that reach the transform (FrameInfo::transform)
// It runs between the chain kernels and unsign_kernel, on the sign-magnitude words; everything behind it is unchanged.
//
// Memory bound: 2 bytes read and at most 2 written per sample of a truncated chain, nothing for a whole chain (off = 0).
#pragma once

namespace {

constexpr int kReconMax = 4;                       // the midpoint of the interval
constexpr uint32_t kReconThreads = 256, kReconParts = 8;

// p of a chain: the planes below the last one it runs
ICER_HD int recon_missing_planes(const ChainDesc &c, int nplanes)
{
    int t = 0;
    while (t < nplanes && c.pkt[nplanes - 1 - t] != kNoPacket) t++;
    return nplanes - t;
}
ICER_HD uint32_t recon_offset(int p, int eighths) { return ((uint32_t)eighths * ((1u << p) - 1u)) >> 3; }

// grid = (chain descriptors, kReconParts), block = kReconThreads.  `n_chains` descriptors, of which the empty slots of the
// device planner (frame = kNoChain, no frame of the batch) are skipped.  The parts of a chain take turns at runs of
// blockDim.x consecutive samples of its rectangle in row order: a wavefront's accesses are contiguous within a row.
__global__ void __launch_bounds__(kReconThreads)
reconstruct_kernel(uint16_t *__restrict__ planes, size_t frame_stride, int channels, const ChainDesc *__restrict__ chains,
                   uint32_t n_chains, const FrameInfo *__restrict__ frames, uint32_t n_frames, int nplanes, int sign_bit,
                   int eighths)
{
    if (blockIdx.x >= n_chains) return;
    const ChainDesc &c = chains[blockIdx.x];
    if (c.frame >= n_frames) return;
    const uint32_t off = recon_offset(recon_missing_planes(c, nplanes), eighths);
    if (off == 0) return;
    const FrameInfo f = frames[c.frame];
    if (!f.transform) return;
    const uint32_t w = c.w, total = w * (uint32_t)c.h, mag_mask = (1u << sign_bit) - 1u;      // (16-bit sides: no overflow)
    uint16_t *p = planes + ((size_t)c.frame * channels + c.chan) * frame_stride + c.first;
    for (uint32_t i = blockIdx.y * blockDim.x + threadIdx.x; i < total; i += gridDim.y * blockDim.x) {
        const size_t at = (size_t)(i / w) * f.w + i % w;
        const uint32_t v = p[at];
        if (v & mag_mask) p[at] = (uint16_t)(v + off);
    }
}

}  // namespace
