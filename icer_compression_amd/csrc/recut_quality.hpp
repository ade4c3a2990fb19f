// recut_quality.hpp -- icerx_recut_device_target_async and icerx_recut_device_budget_async (include/icer_hip_dec_quality.h):
// stored masters re-cut where a distortion target is met, or so that the frames of a call share a byte budget at equal
// distortion -- the two quality-driven cuts of the encoder (icerx_encode_device_target / _budget), without the pixels and
// without re-coding.  Included by decoder.hip after recut.hpp, whose blob stage, frame walk, tables and gather serve here too.
//
// What decides such a cut is the units' payload bits (the master's packet table) and the frame's residual-energy table
// E[family][b] with its LL means (distortion_core.hpp), which the encoder exports once per frame beside the master: the
// distortion sidecar, n_families x (P + 1) + 1 words.  A cut at reduce r runs over the units and families of the geometry at
// 1/2^r size; its E rows are the master's, read through the family map of the recutter (recut_quality_build).
//
//   blob       enqueue_blob_stage
//   frames     recut_quality_frame_kernel, one workgroup per frame: walk_frame and recut_unit_bits as recut_plan_kernel; the
//              frame's record -- status, top level, LL means --; its sidecar row checked; the E rows of every geometry in use
//              gathered through that geometry's family map
//   target     recut_target_scan_kernel, one wavefront per (frame, cut): scan_target_wave
//   budget     recut_budget_curve_kernel, one wavefront per frame: curve_frame_wave; recut_budget_search_kernel, one workgroup
//              per budget: budget_search_wave (state in the workspace), then budget_finish_wave, a wavefront a frame
//   packets    recut_gather_kernel
// The unit tables of a recutter have cap_is_bound 0 and no bit count is kUnitFailed: the wave functions' redo flags are 0.
#include "budget_core.hpp"
#include "subband_gain.hpp"

namespace {

#ifdef ICER_HOST_MOCK
constexpr uint32_t kRecutQualityScanThreads = 1, kRecutBudgetThreads = 1;
#else
constexpr uint32_t kRecutQualityScanThreads = 64, kRecutBudgetThreads = 64 * 16;
#endif

// what the frame stage leaves of a frame: the walk's status and top level (recut_cut_status), whether its sidecar row is
// unusable, its LL means as scan_target_wave reads them
struct RecutQualityFrame {
    int32_t status;
    uint32_t max_level, bad_sidecar, pad;
    uint16_t means[4];
};

// the family tables of every geometry, passed by value with the launches; e_at: where a frame's gathered E rows at r start
struct RecutQualityTables {
    const uint32_t *weight[kRecutMaxReduce + 1], *chan[kRecutMaxReduce + 1], *fam_map[kRecutMaxReduce + 1];
    const unsigned long long *ll_term[kRecutMaxReduce + 1], *fam_cap;
    uint32_t n_families[kRecutMaxReduce + 1], e_at[kRecutMaxReduce + 1];
    uint32_t P, e_stride;                             // coded planes; gathered E entries a frame
};

ICER_HD int recut_quality_status(const RecutQualityFrame &f, uint32_t reduce)
{
    const int s = recut_cut_status(f.status, f.max_level, reduce);
    return s != kOk ? s : f.bad_sidecar ? kInvalidInput : kOk;
}

// The cuts call's workspace, then: a record per frame, the gathered E rows (every geometry's, a frame after the other), and
// for the budget call the frames' curves (pitch: units of the full geometry + 1), their heads and a search state per budget
// and frame.
struct RecutQualityLayout {
    RecutLayout cut;
    size_t frames, energy, curve_d, curve_used, head, state, total;
};
RecutQualityLayout recut_quality_layout(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts, bool budget)
{
    RecutQualityLayout L;
    L.cut = recut_layout(r, n, data_bytes, n_cuts, true);
    const size_t N = (size_t)n, pitch = (size_t)r->red[0].n_units + 1u;
    Carver c;
    c.at = L.cut.total;
    L.frames = c.take(sizeof(RecutQualityFrame) * N);
    L.energy = c.take(sizeof(uint64_t) * N * r->families_total * ((size_t)r->geom.planes + 1u));
    L.curve_d = L.curve_used = L.head = L.state = c.at;
    if (budget) {
        L.curve_d = c.take(sizeof(uint64_t) * N * pitch);
        L.curve_used = c.take(sizeof(uint64_t) * N * pitch);
        L.head = c.take(sizeof(uint32_t) * N * kCurveHeadWords);
        L.state = c.take(sizeof(BudgetState) * N * (size_t)n_cuts);
    }
    L.total = c.at;
    return L;
}

// one workgroup per frame, as recut_plan_kernel up to its first barrier; then the frame's sidecar row sidecar[k * stride ..]:
// the means word into the record; every row of E checked -- non-decreasing in b, E[g][P] at most fam_cap[g] --; and for every
// geometry in use at which the frame has a stream, its families' rows through fam_map (r = 0: as they are) into `energy`.
// A row that fails the check is still gathered: nothing reads it, the frame has a status.
__global__ void __launch_bounds__(256)
recut_quality_frame_kernel(const uint8_t *__restrict__ blob, uint32_t blob_len, const uint64_t *__restrict__ offsets, uint64_t stream_stride,
                           const uint64_t *__restrict__ lens, const DCandRec *__restrict__ recs, const AsyncHead *__restrict__ head,
                           DPlanGeom geom, uint64_t image_w, uint64_t image_h, RecutCutTables tabs, uint32_t bits_stride, uint32_t used,
                           RecutQualityTables q, const unsigned long long *__restrict__ sidecar, size_t sidecar_stride,
                           uint32_t *__restrict__ tab_off, uint32_t *__restrict__ tab_bits, uint32_t *__restrict__ unit_bits,
                           RecutQualityFrame *__restrict__ frames, unsigned long long *__restrict__ energy)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // kWalkLds
    const uint32_t k = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const uint64_t off = offsets ? offsets[k] : (uint64_t)k * stream_stride, len = lens[k];
    uint32_t *to = tab_off + (size_t)k * geom.slots(), *tb = tab_bits + (size_t)k * geom.slots();
    uint32_t *bits = unit_bits + (size_t)k * bits_stride;
    WalkNotes notes;
    const DWalk s = walk_frame(lds, blob, blob_len, off, len, recs, head, geom, image_w, image_h, to, tb, &notes);
    const int status = recut_frame_status(notes.inside != 0u, s.cursor, notes.other_size != 0u);
    for (uint32_t r = 0; r <= (uint32_t)kRecutMaxReduce; r++)
        if (((used >> r) & 1u) && recut_cut_status(status, notes.max_level, r) == kOk)
            recut_unit_bits(to, tb, tabs.unit_slot[r], tabs.n_units[r], bits + tabs.bits_at[r], tid, nth);
    const uint32_t row_len = q.P + 1u, n_fam = q.n_families[0];
    const unsigned long long *E = sidecar + (size_t)k * sidecar_stride;
    if (tid == 0) {
        RecutQualityFrame f;
        f.status = status; f.max_level = notes.max_level; f.bad_sidecar = 0u; f.pad = 0u;
        const unsigned long long word = E[(size_t)n_fam * row_len];
        for (uint32_t c = 0; c < 4u; c++) f.means[c] = (uint16_t)(word >> (16u * c));
        frames[k] = f;
    }
    ICER_BARRIER();
    for (uint32_t g = tid; g < n_fam; g += nth) {
        const unsigned long long *e = E + (size_t)g * row_len;
        bool bad = e[q.P] > q.fam_cap[g];
        for (uint32_t b = 0; b < q.P; b++) bad |= e[b] > e[b + 1u];
        if (bad) frames[k].bad_sidecar = 1u;                    // (every thread that writes writes the same)
    }
    unsigned long long *out = energy + (size_t)k * q.e_stride;
    for (uint32_t r = 0; r <= (uint32_t)kRecutMaxReduce; r++) {
        if (!((used >> r) & 1u) || recut_cut_status(status, notes.max_level, r) != kOk) continue;
        const uint32_t *map = tabs.full_to_cut[r] ? q.fam_map[r] : nullptr;
        for (uint32_t i = tid; i < q.n_families[r] * row_len; i += nth) {
            const uint32_t g = i / row_len, b = i - g * row_len;
            out[q.e_at[r] + i] = E[(size_t)(map ? map[g] : g) * row_len + b];
        }
    }
}

// one wavefront per (frame, cut): scan_target_wave with the tables of the geometry at 1/2^r size, the cut's threshold and the
// call's byte cap.  Rows c * n + k as recut_plan_kernel's.  A frame with a status is a frame without a stream: what
// recut_scan_wave writes, reached 0, dist 0, equiv the cap.
__global__ void __launch_bounds__(64)
recut_target_scan_kernel(RecutCutTables tabs, uint32_t bits_stride, RecutCuts cuts, TargetList targets, uint64_t byte_cap, RecutQualityTables q,
                         const RecutQualityFrame *__restrict__ frames, const uint32_t *__restrict__ unit_bits,
                         const unsigned long long *__restrict__ energy, uint64_t *foff, uint64_t *by_unit,
                         unsigned long long *__restrict__ sizes, int32_t *__restrict__ rcs, int32_t *__restrict__ reached,
                         unsigned long long *__restrict__ dist, unsigned long long *__restrict__ equiv)
{
    const uint32_t k = blockIdx.x, c = blockIdx.y, n = gridDim.x, tid = threadIdx.x, n_full = tabs.n_units[0];
    const uint32_t r = cuts.reduce[c];
    const size_t row = (size_t)c * n + k;
    const RecutQualityFrame &fr = frames[k];
    const int status = recut_quality_status(fr, r);
    const uint32_t *bits = unit_bits + (size_t)k * bits_stride + tabs.bits_at[r];
    uint64_t *cut_off = (r ? by_unit : foff) + row * n_full;
    if (status != kOk) {
        recut_scan_wave(status, bits, tabs.final_order[r], tabs.n_units[r], byte_cap, tabs.units[r], cut_off, sizes + row, rcs + row);
        if (tid == 0) { reached[row] = 0; dist[row] = 0; equiv[row] = byte_cap; }
    } else
        (void)scan_target_wave(bits, tabs.final_order[r], tabs.n_units[r], targets.t[c], byte_cap, 0, tabs.units[r],
                               energy + (size_t)k * q.e_stride + q.e_at[r], q.weight[r], q.n_families[r], q.P, q.ll_term[r], q.chan[r],
                               fr.means, cut_off, sizes + row, rcs + row, reached + row, dist + row, equiv + row);
    if (r) {
        ICER_BARRIER();
        recut_offsets_by_master_unit(cut_off, tabs.full_to_cut[r], n_full, foff + row * n_full, tid, blockDim.x);
    }
}

// one wavefront per frame: its curve at reduce r under the byte cap (curve_frame_wave); a frame with a status is a skipped one
__global__ void __launch_bounds__(64)
recut_budget_curve_kernel(RecutCutTables tabs, uint32_t bits_stride, uint32_t r, uint64_t byte_cap, RecutQualityTables q,
                          const RecutQualityFrame *__restrict__ frames, const uint32_t *__restrict__ unit_bits,
                          const unsigned long long *__restrict__ energy, uint32_t pitch, unsigned long long *__restrict__ curve_d,
                          unsigned long long *__restrict__ curve_used, uint32_t *__restrict__ head)
{
    const uint32_t k = blockIdx.x;
    const RecutQualityFrame &fr = frames[k];
    curve_frame_wave(unit_bits + (size_t)k * bits_stride + tabs.bits_at[r], tabs.n_units[r], byte_cap, recut_quality_status(fr, r) != kOk,
                     tabs.units[r], energy + (size_t)k * q.e_stride + q.e_at[r], q.weight[r], q.n_families[r], q.P, q.ll_term[r], q.chan[r],
                     fr.means, curve_d + (size_t)k * pitch, curve_used + (size_t)k * pitch, head + (size_t)k * kCurveHeadWords);
}

// one workgroup per budget over all frames of the call: wavefront 0 finds the common threshold and hands out what it leaves
// over (budget_search_wave; its state: n entries of `state` per budget), then every wavefront finishes frames
// (budget_finish_wave; a frame with a status: as in recut_target_scan_kernel), and the workgroup turns the final offsets of a
// cut at r > 0 into the order of the master's units.  Rows b * n + k.
__global__ void __launch_bounds__(64 * 16)
recut_budget_search_kernel(RecutCutTables tabs, uint32_t bits_stride, uint32_t r, BudgetList budgets, uint64_t byte_cap, uint32_t n,
                           const RecutQualityFrame *__restrict__ frames, const uint32_t *__restrict__ unit_bits, uint32_t pitch,
                           const unsigned long long *__restrict__ curve_d, const unsigned long long *__restrict__ curve_used,
                           const uint32_t *__restrict__ head, BudgetState *state, uint64_t *foff, uint64_t *by_unit,
                           unsigned long long *__restrict__ sizes, int32_t *__restrict__ rcs, int32_t *__restrict__ at_cap,
                           unsigned long long *__restrict__ dist, unsigned long long *__restrict__ equiv,
                           unsigned long long *__restrict__ threshold, unsigned long long *__restrict__ total)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x, n_full = tabs.n_units[0];
#ifdef ICER_HOST_MOCK
    const uint32_t wave = 0, waves = 1, lane0 = 1;
#else
    const uint32_t wave = tid >> 6, waves = blockDim.x >> 6, lane0 = (tid & 63u) == 0u;
#endif
    BudgetState *st = state + (size_t)b * n;
    if (wave == 0) budget_search_wave(curve_d, curve_used, head, pitch, n, budgets.b[b], st, threshold + b, total + b);
    ICER_BARRIER();
    for (uint32_t k = wave; k < n; k += waves) {
        const size_t row = (size_t)b * n + k;
        const int status = recut_quality_status(frames[k], r);
        const uint32_t *bits = unit_bits + (size_t)k * bits_stride + tabs.bits_at[r];
        uint64_t *cut_off = (r ? by_unit : foff) + row * n_full;
        if (status != kOk) {
            recut_scan_wave(status, bits, tabs.final_order[r], tabs.n_units[r], byte_cap, tabs.units[r], cut_off, sizes + row, rcs + row);
            if (lane0) { at_cap[row] = 0; dist[row] = 0; equiv[row] = byte_cap; }
        } else
            (void)budget_finish_wave(bits, tabs.final_order[r], tabs.n_units[r], st[k].lo, head[(size_t)k * kCurveHeadWords], st[k].d_lo, byte_cap, 0,
                                     tabs.units[r], cut_off, sizes + row, rcs + row, at_cap + row, dist + row, equiv + row);
    }
    if (r) {
        ICER_BARRIER();
        for (uint32_t k = 0; k < n; k++) {
            const size_t row = (size_t)b * n + k;
            recut_offsets_by_master_unit(by_unit + row * n_full, tabs.full_to_cut[r], n_full, foff + row * n_full, tid, blockDim.x);
        }
    }
}

// ---- the tables of a quality recutter ---------------------------------------------------------------------------------------
// Per geometry r: every family's weight, channel and LL term as prepare_target of the encoder library builds them, level lv of
// that geometry weighted as kSubbandGainQ4[filt][lv - 1][sb]; the bound of the frame's distortion must fit 64 bits.  The bound
// counts an LL mean of up to 0xFF00 where the encoder's counts 0x7F00: a mean read from a stored sidecar can be anything, and
// with this bound and the per-frame check of the E rows no sum of the curve can overflow.  For r > 0 the family map, through
// the unit correspondence (unit (ch, lv, sb, sg, lsb) there is the master's slot (ch, lv + r, sb, sg, lsb)): it must be a
// function that keeps the coefficient count, which it is unless a grid was kept from the packet before (quirk P1, plan.hpp).
int recut_quality_refuse(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_error = buf;
    return ICER_INVALID_INPUT;
}

int recut_quality_build(const std::vector<Plan> &plans, const DPlanGeom &geom, int filt, int sample_bits, RecutQualityHost *q)
{
    if (filt < 0 || filt > 6) return recut_quality_refuse("icerx_recutter_create_quality: filter %d", filt);
    const uint64_t max_mag = sample_bits == 8 ? 128u : 32767u;
    std::vector<uint32_t> master_of_slot(geom.slots(), kNoPacket);
    std::vector<uint64_t> coef0;
    for (size_t k = 0; k < plans.size(); k++) {
        const Plan &plan = plans[k];
        const size_t n_fam = plan.n_families;
        std::vector<uint32_t> &weight = q->weight[k], &chan = q->chan[k], &map = q->fam_map[k];
        std::vector<unsigned long long> &ll_term = q->ll_term[k];
        weight.assign(n_fam, 0u); chan.assign(n_fam, 0u); ll_term.assign(n_fam, 0ull); map.assign(n_fam, kNoPacket);
        std::vector<uint64_t> coef(n_fam, 0);
        unsigned __int128 bound = 0;
        for (size_t v = 0; v < plan.units.size(); v++) {
            const UnitDesc &u = plan.units[v];
            const uint32_t slot = geom.slot(u.chan, u.level + (uint32_t)k, u.subband, u.seg, u.lsb);
            if (k == 0) master_of_slot[slot] = (uint32_t)v;
            else {
                const uint32_t m = master_of_slot[slot];
                const uint32_t fam = m == kNoPacket ? kNoPacket : plans[0].units[m].family;
                if (fam == kNoPacket || (map[u.family] != kNoPacket && map[u.family] != fam) || coef0[fam] != (uint64_t)u.w * u.h)
                    return recut_quality_refuse("icerx_recutter_create_quality: the families of the geometry at 1/2^%d size do not map to the master's "
                                                "(a subband with fewer samples than segments)", (int)k);
                map[u.family] = fam;
            }
            if (weight[u.family]) continue;
            weight[u.family] = kSubbandGainQ4[filt][u.level - 1][u.subband];
            chan[u.family] = u.chan;
            coef[u.family] = (uint64_t)u.w * u.h;
            bound += (unsigned __int128)coef[u.family] * (max_mag * max_mag) * weight[u.family];
            if (u.subband == kLL && sample_bits == 16) {
                ll_term[u.family] = (unsigned long long)coef[u.family] * weight[u.family];
                bound += (unsigned __int128)ll_term[u.family] * (0xFF00ull * 0xFF00ull);
            }
        }
        if (bound >> 64)
            return recut_quality_refuse("icerx_recutter_create_quality: the distortion of the geometry at 1/2^%d size can exceed 64 bits", (int)k);
        if (k == 0) {
            coef0 = coef;
            q->fam_cap.resize(n_fam);
            for (size_t g = 0; g < n_fam; g++) q->fam_cap[g] = coef[g] * (max_mag * max_mag);
        }
    }
    return ICER_RESULT_OK;
}

int recut_quality_upload(icerx_recutter *r, const RecutQualityHost &q)
{
    int rc = ICER_RESULT_OK;
    for (int k = 0; k <= r->max_reduce; k++) {
        icerx_recutter::Quality &g = r->qual[k];
        g.n_families = (uint32_t)q.weight[k].size();
        r->families_total += g.n_families;
        HIP_TRY(recut_upload(&g.weight, q.weight[k].data(), sizeof(uint32_t) * g.n_families));
        HIP_TRY(recut_upload(&g.chan, q.chan[k].data(), sizeof(uint32_t) * g.n_families));
        HIP_TRY(recut_upload(&g.ll_term, q.ll_term[k].data(), sizeof(unsigned long long) * g.n_families));
        if (k) HIP_TRY(recut_upload(&g.fam_map, q.fam_map[k].data(), sizeof(uint32_t) * g.n_families));
    }
    HIP_TRY(recut_upload(&r->fam_cap, q.fam_cap.data(), sizeof(unsigned long long) * q.fam_cap.size()));
done:
    return rc;
}

RecutQualityTables recut_quality_tables(const icerx_recutter *r)
{
    RecutQualityTables q = {};
    uint32_t at = 0;
    q.P = r->geom.planes;
    for (int k = 0; k <= r->max_reduce; k++) {
        const icerx_recutter::Quality &g = r->qual[k];
        q.weight[k] = (const uint32_t *)g.weight; q.chan[k] = (const uint32_t *)g.chan; q.fam_map[k] = (const uint32_t *)g.fam_map;
        q.ll_term[k] = (const unsigned long long *)g.ll_term;
        q.n_families[k] = g.n_families; q.e_at[k] = at;
        at += g.n_families * (q.P + 1u);
    }
    q.fam_cap = (const unsigned long long *)r->fam_cap;
    q.e_stride = at;
    return q;
}

size_t recut_sidecar_entries(const icerx_recutter *r)
{
    return r && r->filt >= 0 ? (size_t)r->qual[0].n_families * ((size_t)r->geom.planes + 1u) + 1u : 0u;
}

// floor(mse x samples at 1/2^reduce size x 16) saturated to 64 bits (target_threshold of the encoder library); false: negative or
// not a number
bool recut_target_threshold(const icerx_recutter *r, double target_mse, int reduce, uint64_t *T)
{
    if (!(target_mse >= 0.0)) return false;
    const double t = target_mse * (double)(reduced_dim(r->w, reduce) * reduced_dim(r->h, reduce) * (uint64_t)r->geom.channels * 16u);
    *T = t >= 18446744073709551616.0 ? ~0ull : (uint64_t)t;
    return true;
}

// Both calls: `reduces` and the thresholds or budgets are the call's cuts.  Every check before the first launch.
struct RecutQualityCall {
    int n;
    const uint8_t *d_data;
    size_t data_bytes;
    const uint64_t *d_offsets;
    size_t stream_stride;
    const uint64_t *d_lens, *d_sidecar;
    size_t sidecar_stride;
    int n_cuts;
    size_t byte_cap;
    uint8_t *d_out;
    size_t out_stride;
    uint64_t *d_sizes;
    int32_t *d_rcs, *d_flag;                           // reached / at_cap
    uint64_t *d_dist, *d_equiv;
    void *workspace;
    size_t workspace_bytes;
    hipStream_t st;
};

int recut_quality_async(icerx_recutter *r, const RecutQualityCall &c, const int *reduces, const TargetList *targets, const BudgetList *budgets,
                        uint64_t *d_threshold, uint64_t *d_total)
{
    if (!r || r->filt < 0 || !c.d_sidecar || !c.d_flag || !c.d_dist || !c.d_equiv) return ICER_INVALID_INPUT;
    if (c.n_cuts < 1 || c.n_cuts > kMaxLadder) return ICER_INVALID_INPUT;
    if (c.sidecar_stride < recut_sidecar_entries(r)) return ICER_INVALID_INPUT;
    size_t caps[kMaxLadder];
    for (int k = 0; k < c.n_cuts; k++) caps[k] = c.byte_cap;
    RecutCuts cuts = {};
    uint32_t used = 0;
    int rc = recut_check(r, c.n, c.d_data, c.data_bytes, c.d_lens, reduces, caps, c.n_cuts, c.d_out, c.out_stride, c.d_sizes, c.d_rcs, c.workspace,
                         &cuts, &used);
    if (rc != ICER_RESULT_OK) return rc;
    const RecutQualityLayout L = recut_quality_layout(r, c.n, c.data_bytes, c.n_cuts, budgets != nullptr);
    if (c.workspace_bytes < L.total) return ICER_INVALID_INPUT;
    uint8_t *ws = (uint8_t *)c.workspace;
    uint32_t *tab_off = (uint32_t *)(ws + L.cut.blob.tab_off), *tab_bits = (uint32_t *)(ws + L.cut.blob.tab_bits);
    uint32_t *unit_bits = (uint32_t *)(ws + L.cut.bits);
    uint64_t *foff = (uint64_t *)(ws + L.cut.foff), *by_unit = (uint64_t *)(ws + L.cut.by_unit);
    RecutQualityFrame *frames = (RecutQualityFrame *)(ws + L.frames);
    unsigned long long *energy = (unsigned long long *)(ws + L.energy);
    const uint32_t n_full = r->red[0].n_units, n = (uint32_t)c.n;
    const RecutCutTables tabs = recut_cut_tables(r);
    const RecutQualityTables q = recut_quality_tables(r);

    // 1. candidates over the blob
    if ((rc = enqueue_blob_stage(L.cut.blob, ws, (size_t)n, r->geom.slots(), c.d_data, c.data_bytes, (const uint32_t *)r->crc, r->n_cus, c.st)) !=
        ICER_RESULT_OK)
        return rc;
    // 2. per frame: packet table, bit counts, the sidecar row checked and gathered
    ICER_LAUNCH_ON(c.st, recut_quality_frame_kernel, n, kRecutPlanThreads, kWalkLds, c.d_data, (uint32_t)c.data_bytes, c.d_offsets,
                   (uint64_t)c.stream_stride, c.d_lens, (const DCandRec *)(ws + L.cut.blob.cands), (const AsyncHead *)(ws + L.cut.blob.head), r->geom,
                   r->w, r->h, tabs, L.cut.bits_stride, used, q, (const unsigned long long *)c.d_sidecar, c.sidecar_stride, tab_off, tab_bits,
                   unit_bits, frames, energy);
    HIP_TRY(hipGetLastError());
    if (targets) {
        // 3. per frame and cut: the walk to the cut's threshold
        ICER_LAUNCH_ON(c.st, recut_target_scan_kernel, dim3(n, (unsigned)c.n_cuts), kRecutQualityScanThreads, 0, tabs, L.cut.bits_stride, cuts,
                       *targets, (uint64_t)c.byte_cap, q, (const RecutQualityFrame *)frames, (const uint32_t *)unit_bits,
                       (const unsigned long long *)energy, foff, by_unit, (unsigned long long *)c.d_sizes, c.d_rcs, c.d_flag,
                       (unsigned long long *)c.d_dist, (unsigned long long *)c.d_equiv);
        HIP_TRY(hipGetLastError());
    } else {
        // 3. per frame: its curve; per budget: the common threshold, the fill, every frame's cut
        const uint32_t pitch = n_full + 1u, reduce = cuts.reduce[0];
        unsigned long long *curve_d = (unsigned long long *)(ws + L.curve_d), *curve_used = (unsigned long long *)(ws + L.curve_used);
        uint32_t *head = (uint32_t *)(ws + L.head);
        ICER_LAUNCH_ON(c.st, recut_budget_curve_kernel, n, kRecutQualityScanThreads, 0, tabs, L.cut.bits_stride, reduce, (uint64_t)c.byte_cap, q,
                       (const RecutQualityFrame *)frames, (const uint32_t *)unit_bits, (const unsigned long long *)energy, pitch, curve_d,
                       curve_used, head);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(c.st, recut_budget_search_kernel, (unsigned)c.n_cuts, kRecutBudgetThreads, 0, tabs, L.cut.bits_stride, reduce, *budgets,
                       (uint64_t)c.byte_cap, n, (const RecutQualityFrame *)frames, (const uint32_t *)unit_bits, pitch,
                       (const unsigned long long *)curve_d, (const unsigned long long *)curve_used, (const uint32_t *)head,
                       (BudgetState *)(ws + L.state), foff, by_unit, (unsigned long long *)c.d_sizes, c.d_rcs, c.d_flag,
                       (unsigned long long *)c.d_dist, (unsigned long long *)c.d_equiv, (unsigned long long *)d_threshold,
                       (unsigned long long *)d_total);
        HIP_TRY(hipGetLastError());
    }
    // 4. the kept packets, each with its cut's header
    ICER_LAUNCH_ON(c.st, recut_gather_kernel, dim3(n_full, n), kRecutGatherThreads, 0, c.d_data, c.d_offsets, (uint64_t)c.stream_stride, r->geom,
                   (const uint32_t *)r->red[0].unit_slot, n_full, tab_off, tab_bits, foff, cuts, (uint32_t)c.n_cuts, (const uint32_t *)r->crc,
                   c.d_out, c.out_stride);
    HIP_TRY(hipGetLastError());
done:
    return rc;
}

}  // namespace

extern "C" {

int icerx_recutter_create_quality(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, int filt, unsigned segments,
                                  int sample_bits, int max_reduce)
{
    return recutter_create(out, device, w, h, channels, stages, segments, sample_bits, max_reduce, true, filt);
}

size_t icerx_recut_sidecar_entries(const icerx_recutter *r) { return recut_sidecar_entries(r); }

uint64_t icerx_recut_target_threshold(const icerx_recutter *r, double target_mse, int reduce)
{
    uint64_t T = 0;
    return r && reduce >= 0 && reduce <= r->max_reduce && recut_target_threshold(r, target_mse, reduce, &T) ? T : 0;
}

size_t icerx_recut_target_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts)
{
    if (!r || r->filt < 0 || n <= 0 || n_cuts < 1 || n_cuts > kMaxLadder) return 0;
    return recut_quality_layout(r, n, data_bytes, n_cuts, false).total;
}

int icerx_recut_device_target_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                    size_t stream_stride, const uint64_t *d_lens, const uint64_t *d_sidecar, size_t sidecar_stride,
                                    const int *reduces, const double *target_mse, int n_cuts, size_t byte_cap, uint8_t *d_out,
                                    size_t out_stride, uint64_t *d_sizes, int32_t *d_rcs, int32_t *d_reached, uint64_t *d_dist,
                                    uint64_t *d_equiv_quota, void *d_workspace, size_t workspace_bytes, void *stream)
{
    g_error.clear();
    if (!r || r->filt < 0 || !target_mse || n_cuts < 1 || n_cuts > kMaxLadder) return ICER_INVALID_INPUT;
    TargetList targets = {};
    for (int c = 0; c < n_cuts; c++) {
        const int reduce = reduces ? reduces[c] : 0;
        if (reduce < 0 || reduce > r->max_reduce || !recut_target_threshold(r, target_mse[c], reduce, &targets.t[c])) return ICER_INVALID_INPUT;
    }
    const RecutQualityCall c{n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, d_sidecar, sidecar_stride, n_cuts, byte_cap,
                             d_out, out_stride, d_sizes, d_rcs, d_reached, d_dist, d_equiv_quota, d_workspace, workspace_bytes, (hipStream_t)stream};
    return recut_quality_async(r, c, reduces, &targets, nullptr, nullptr, nullptr);
}

size_t icerx_recut_budget_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_budgets)
{
    if (!r || r->filt < 0 || n <= 0 || n_budgets < 1 || n_budgets > kMaxLadder) return 0;
    return recut_quality_layout(r, n, data_bytes, n_budgets, true).total;
}

int icerx_recut_device_budget_async(icerx_recutter *r, int n, const void *d_data, size_t data_bytes, const uint64_t *d_offsets,
                                    size_t stream_stride, const uint64_t *d_lens, const uint64_t *d_sidecar, size_t sidecar_stride, int reduce,
                                    const uint64_t *budgets, int n_budgets, size_t byte_cap, uint8_t *d_out, size_t out_stride,
                                    uint64_t *d_sizes, int32_t *d_rcs, int32_t *d_at_cap, uint64_t *d_dist, uint64_t *d_equiv_quota,
                                    uint64_t *d_threshold, uint64_t *d_total, void *d_workspace, size_t workspace_bytes, void *stream)
{
    g_error.clear();
    if (!r || r->filt < 0 || !budgets || !d_threshold || !d_total || n_budgets < 1 || n_budgets > kMaxLadder) return ICER_INVALID_INPUT;
    BudgetList list = {};
    int reduces[kMaxLadder];
    for (int b = 0; b < n_budgets; b++) { list.b[b] = budgets[b]; reduces[b] = reduce; }
    const RecutQualityCall c{n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, d_sidecar, sidecar_stride, n_budgets, byte_cap,
                             d_out, out_stride, d_sizes, d_rcs, d_at_cap, d_dist, d_equiv_quota, d_workspace, workspace_bytes, (hipStream_t)stream};
    return recut_quality_async(r, c, reduces, nullptr, &list, d_threshold, d_total);
}

}  // extern "C"
