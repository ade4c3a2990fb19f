// combine.hpp -- icerx_combine_device_async (include/icer_hip_dec.h): the union or the difference of two stored streams of one
// frame, on the device.  A decoder files packets by (channel, level, subband, bit plane, segment) and does not mind their
// order, so a held stream followed by the packets it lacks decodes as the larger stream does; this call computes those packets
// (DIFFERENCE) and the canonical stream of both (UNION).  Included by decoder.hip after recut.hpp, whose recutter, blob stage,
// call record (RecutCall), masters (RecutMasters, one per operand), frame walk (recut_walk) and packet copy it uses; the rule
// itself is combine_core.hpp.
//
//   blob       enqueue_blob_stage, once over the blob that holds both operands; two packet tables per frame (A's of frame k
//              is table k, B's table n + k)
//   frames     combine_plan_kernel, one workgroup per frame: recut_walk for A, then for B; the frame's status; a workgroup scan
//              of the kept packets' lengths along the final order -> per unit its offset in the result (~0: not kept), where
//              its packet lies in the blob and its length; size, return code, counts
//   packets    combine_gather_kernel, one workgroup per (unit, frame): header and payload in one copy (copy_unit_recut)
// Everything is enqueued on the caller's stream; the caller owns the workspace (combine_layout).
#include "combine_core.hpp"

namespace {

#ifdef ICER_HOST_MOCK
constexpr uint32_t kCombinePlanThreads = 1, kCombineGatherThreads = 3;
#else
constexpr uint32_t kCombinePlanThreads = 256, kCombineGatherThreads = 256;
#endif
// combine_plan_kernel's dynamic LDS: the walk's, then a CombineSum per thread
constexpr uint32_t kCombinePartsAt = (kWalkLds + 15u) & ~15u;
constexpr uint32_t combine_plan_lds(uint32_t threads) { return kCombinePartsAt + threads * (uint32_t)sizeof(CombineSum); }

// the blob stage with 2 n packet tables; per frame and unit of the plan the offset in the result, the packet's place in the
// blob and its length
struct CombineLayout {
    BlobLayout blob;
    size_t foff, from, bytes, total;
};
CombineLayout combine_layout(const icerx_recutter *r, int n, size_t data_bytes)
{
    CombineLayout L;
    const size_t per = (size_t)n * r->red[0].n_units;
    Carver c;
    const size_t head = c.take(sizeof(AsyncHead));
    L.blob = blob_layout(c, head, 2u * (size_t)n, data_bytes, r->geom.slots());
    L.foff = c.take(sizeof(uint64_t) * per);
    L.from = c.take(sizeof(uint32_t) * per);
    L.bytes = c.take(sizeof(uint32_t) * per);
    L.total = c.at;
    return L;
}

// what the plan leaves of every frame: row k of foff / from / bytes (n_units entries a row) in the workspace; entries 2 k and
// 2 k + 1 of the caller's counts
struct CombinePlan {
    uint64_t *foff;
    uint32_t *from, *bytes, *counts;
};

// one workgroup per frame, of any size: the operands `a` and `b` as RecutMasters of one blob (A's tables are the first n, B's
// the n behind them), the plan of the full geometry.  Entry k of o.sizes / o.rcs.  A frame with a status, or whose result is
// longer than o.out_stride, keeps nothing (every foff ~0).
__global__ void __launch_bounds__(256)
combine_plan_kernel(RecutMasters a, RecutMasters b, int op, const uint32_t *__restrict__ unit_slot, const uint32_t *__restrict__ final_order,
                    uint32_t n_units, CombinePlan p, RecutOut o)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // combine_plan_lds(blockDim.x)
    const uint32_t k = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const RecutTabRows ta = a.rows(k), tb = b.rows(k);
    const uint64_t off_a = a.offset(k), off_b = b.offset(k);
    const int status_a = recut_walk(lds, a, off_a, a.lens[k], ta).status;
    ICER_BARRIER();                                            // (every thread has read the first walk's result out of the LDS)
    const int status_b = recut_walk(lds, b, off_b, b.lens[k], tb).status;
    const int status = combine_frame_status(op, status_a, status_b);

    // thread t takes positions [t * per, (t + 1) * per) of the final order: its sum, then its start from the sums before it
    const CombineTables t{ta.off, ta.bits, tb.off, tb.bits};
    CombineSum *parts = reinterpret_cast<CombineSum *>(lds + kCombinePartsAt);
    const uint32_t per = (n_units + nth - 1u) / nth;
    const uint32_t i0 = tid * per < n_units ? tid * per : n_units, i1 = n_units - i0 < per ? n_units : i0 + per;
    CombineSum mine;
    mine.bytes = 0; mine.packets = 0; mine.from_a = 0;
    if (status == kOk) mine = combine_sum_range(op, t, unit_slot, final_order, i0, i1);
    parts[tid] = mine;
    ICER_BARRIER();
    CombineSum all;
    all.bytes = 0; all.packets = 0; all.from_a = 0;
    uint64_t at = 0;
    for (uint32_t j = 0; j < nth; j++) {
        if (j == tid) at = all.bytes;
        all.bytes += parts[j].bytes; all.packets += parts[j].packets; all.from_a += parts[j].from_a;
    }
    const bool place = status == kOk && all.bytes <= o.out_stride;
    // (an operand with a status of its own has no packet in its table, and its offset is not looked at)
    combine_place_range(op, t, unit_slot, final_order, i0, i1, place, at, (uint32_t)off_a, (uint32_t)off_b, p.foff + (size_t)k * n_units,
                        p.from + (size_t)k * n_units, p.bytes + (size_t)k * n_units);
    if (tid == 0) {
        o.sizes[k] = status == kOk ? all.bytes : 0ull;
        o.rcs[k] = status != kOk ? status : place ? kOk : kOutputBufTooSmall;
        p.counts[2u * (size_t)k] = all.packets;
        p.counts[2u * (size_t)k + 1u] = all.from_a;
    }
}

// one workgroup per (unit of the plan, frame): the kept packet, header and payload, from wherever it lies in the blob
__global__ void __launch_bounds__(256)
combine_gather_kernel(const uint8_t *__restrict__ blob, uint32_t n_units, const uint64_t *__restrict__ foff, const uint32_t *__restrict__ from,
                      const uint32_t *__restrict__ bytes, uint8_t *__restrict__ out, size_t out_stride)
{
    const uint32_t frame = blockIdx.y;
    const size_t at = (size_t)frame * n_units + blockIdx.x;
    if (foff[at] == ~0ull) return;
    // (the walk accepted this packet: it lies inside its operand, and the operand inside the blob)
    copy_unit_recut(blob + from[at], bytes[at], foff + at, 0, 1u, out + (size_t)frame * out_stride, 0, threadIdx.x, blockDim.x);
}

// where the frames of an operand lie: frame k = blob bytes [off, off + lens[k]), off = offsets[k] or base + k * stream_stride
struct CombineOperand {
    const uint64_t *offsets, *lens;
    uint64_t base;
};

// The call is a RecutCall without cuts and with no masters of its own (d_offsets, d_lens): the operands stand beside it.
// Every check comes before the first thing enqueued: a refused call writes nothing.
int combine_async(icerx_recutter *r, const RecutCall &c, int op, const CombineOperand &a, const CombineOperand &b, uint32_t *d_counts)
{
    g_error.clear();
    if (!r || c.n < 1 || c.n > kRecutMaxFrames || (op != kCombineUnion && op != kCombineDifference)) return ICER_INVALID_INPUT;
    if (!c.d_data || !a.lens || !b.lens || !c.d_out || !c.d_sizes || !c.d_rcs || !d_counts || !c.workspace) return ICER_INVALID_INPUT;
    if (c.data_bytes >= 0xFFFFFFFFull - 64u) return fail("batch of %zu stream bytes: 32-bit offsets only", c.data_bytes);
    const CombineLayout L = combine_layout(r, c.n, c.data_bytes);
    if (c.workspace_bytes < L.total) return ICER_INVALID_INPUT;
    int rc = ICER_RESULT_OK;
    uint8_t *ws = (uint8_t *)c.workspace;
    const uint32_t n_units = r->red[0].n_units;
    const size_t tabs_a = (size_t)c.n * r->geom.slots();         // (A's packet tables: the first n; B's lie behind them)
    const CombinePlan p{(uint64_t *)(ws + L.foff), (uint32_t *)(ws + L.from), (uint32_t *)(ws + L.bytes), d_counts};
    const RecutOut o{c.d_out, c.out_stride, (unsigned long long *)c.d_sizes, c.d_rcs};
    const RecutMasters ma{c.d_data, (uint32_t)c.data_bytes, a.offsets, a.lens, a.base, (uint64_t)c.stream_stride,
                          (const DCandRec *)(ws + L.blob.cands), (const AsyncHead *)(ws + L.blob.head), r->geom, r->w, r->h,
                          (uint32_t *)(ws + L.blob.tab_off), (uint32_t *)(ws + L.blob.tab_bits)};
    RecutMasters mb = ma;
    mb.offsets = b.offsets; mb.lens = b.lens; mb.base = b.base; mb.tab_off += tabs_a; mb.tab_bits += tabs_a;

    // 1. candidates over the blob
    if ((rc = enqueue_blob_stage(L.blob, ws, 2u * (size_t)c.n, r->geom.slots(), c.d_data, c.data_bytes, (const uint32_t *)r->crc, r->n_cus, c.st)) !=
        ICER_RESULT_OK)
        return rc;
    // 2. per frame: both packet tables, the kept units and their places
    ICER_LAUNCH_ON(c.st, combine_plan_kernel, (unsigned)c.n, kCombinePlanThreads, combine_plan_lds(kCombinePlanThreads), ma, mb, op,
                   (const uint32_t *)r->red[0].unit_slot, (const uint32_t *)r->red[0].final_order, n_units, p, o);
    HIP_TRY(hipGetLastError());
    // 3. the kept packets
    ICER_LAUNCH_ON(c.st, combine_gather_kernel, dim3(n_units, (unsigned)c.n), kCombineGatherThreads, 0, c.d_data, n_units, (const uint64_t *)p.foff,
                   (const uint32_t *)p.from, (const uint32_t *)p.bytes, c.d_out, c.out_stride);
    HIP_TRY(hipGetLastError());
done:
    return rc;
}

}  // namespace

extern "C" {

size_t icerx_combine_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes)
{
    if (!r || n <= 0 || n > kRecutMaxFrames) return 0;
    return combine_layout(r, n, data_bytes).total;
}

int icerx_combine_device_async(icerx_recutter *r, int n, int op, const void *d_data, size_t data_bytes, const uint64_t *d_offsets_a,
                               size_t base_a, const uint64_t *d_lens_a, const uint64_t *d_offsets_b, size_t base_b,
                               const uint64_t *d_lens_b, size_t stream_stride, uint8_t *d_out, size_t out_stride, uint64_t *d_sizes,
                               int32_t *d_rcs, uint32_t *d_counts, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const RecutCall c{n, (const uint8_t *)d_data, data_bytes, nullptr, stream_stride, nullptr, nullptr, nullptr, 0, d_out, out_stride, d_sizes, d_rcs,
                      d_workspace, workspace_bytes, (hipStream_t)stream};
    return combine_async(r, c, op, CombineOperand{d_offsets_a, d_lens_a, (uint64_t)base_a}, CombineOperand{d_offsets_b, d_lens_b, (uint64_t)base_b},
                         d_counts);
}

}  // extern "C"
