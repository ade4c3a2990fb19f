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
//   frames     recut_quality_frame_kernel, one workgroup per frame: recut_frame_stage; the frame's record -- the walk's head,
//              LL means --; its sidecar row checked; the E rows of every geometry in use gathered through that geometry's
//              family map
//   target     recut_target_scan_kernel, one wavefront per (frame, cut): scan_target_wave
//   budget     recut_budget_curve_kernel, one wavefront per frame: curve_frame_wave; recut_budget_search_kernel, one workgroup
//              per budget: budget_search_wave (state in the workspace), then budget_finish_wave, a wavefront a frame
//   packets    recut_gather_kernel
// Both calls run through one driver, recut_quality_async, on recut.hpp's RecutCall and RecutRun.
// The unit tables of a recutter have cap_is_bound 0 and no bit count is kUnitFailed: the wave functions' redo flags are 0.
#include "budget_core.hpp"
#include "subband_gain.hpp"

namespace {

#ifdef ICER_HOST_MOCK
constexpr uint32_t kRecutQualityScanThreads = 1, kRecutBudgetThreads = 1;
#else
constexpr uint32_t kRecutQualityScanThreads = 64, kRecutBudgetThreads = 64 * 16;
#endif

// what the frame stage leaves of a frame: the walk's, whether its sidecar row is unusable, its LL means as scan_target_wave
// reads them
struct RecutQualityFrame {
    RecutFrameHead head;
    uint32_t bad_sidecar, pad;
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
    const int s = recut_cut_status(f.head, reduce);
    return s != kOk ? s : f.bad_sidecar ? kInvalidInput : kOk;
}

// The cuts call's workspace, then: a record per frame, the gathered E rows (every geometry's, a frame after the other), and
// for the budget call the frames' curves (pitch: units of the full geometry + 1), their heads and a search state per budget
// and frame.  RecutQualityWork: the same as pointers, by value with the launches; RecutQualityOut: the outputs of both calls.
struct RecutQualityLayout {
    RecutLayout cut;
    size_t frames, energy, curve_d, curve_used, head, state, total;
};
struct RecutQualityWork {
    RecutQualityFrame *frames;
    unsigned long long *energy, *curve_d, *curve_used;
    uint32_t *head, pitch;
    BudgetState *state;
};
struct RecutQualityOut {
    RecutOut cut;
    int32_t *flag;                                    // reached / at_cap
    unsigned long long *dist, *equiv, *threshold, *total;
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

// one workgroup per frame: recut_frame_stage; then the frame's sidecar row sidecar[k * stride ..]: the means word into the
// record; every row of E checked -- non-decreasing in b, E[g][P] at most fam_cap[g] --; and for every geometry in use at which
// the frame has a stream, its families' rows through fam_map (r = 0: as they are) into `energy`.  A row that fails the check
// is still gathered: nothing reads it, the frame has a status.
__global__ void __launch_bounds__(256)
recut_quality_frame_kernel(RecutMasters m, RecutCutTables tabs, RecutWork w, uint32_t used, RecutQualityTables q,
                           const unsigned long long *__restrict__ sidecar, size_t sidecar_stride, RecutQualityWork qw)
{
    ICER_DYNAMIC_LDS(uint8_t, lds);                            // kWalkLds
    const uint32_t k = blockIdx.x, tid = threadIdx.x, nth = blockDim.x;
    const RecutFrameHead head = recut_frame_stage(lds, m, k, tabs, w, used, tid, nth);
    RecutQualityFrame *frames = qw.frames;
    const uint32_t row_len = q.P + 1u, n_fam = q.n_families[0];
    const unsigned long long *E = sidecar + (size_t)k * sidecar_stride;
    if (tid == 0) {
        RecutQualityFrame f;
        f.head = head; f.bad_sidecar = 0u; f.pad = 0u;
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
    unsigned long long *out = qw.energy + (size_t)k * q.e_stride;
    for (uint32_t r = 0; r <= (uint32_t)kRecutMaxReduce; r++) {
        if (!((used >> r) & 1u) || recut_cut_status(head, r) != kOk) continue;
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
recut_target_scan_kernel(RecutCutTables tabs, RecutWork w, RecutCuts cuts, TargetList targets, uint64_t byte_cap, RecutQualityTables q,
                         RecutQualityWork qw, RecutQualityOut o)
{
    const uint32_t k = blockIdx.x, c = blockIdx.y, n = gridDim.x, tid = threadIdx.x;
    const uint32_t r = cuts.reduce[c];
    const size_t row = (size_t)c * n + k;
    const RecutQualityFrame &fr = qw.frames[k];
    const int status = recut_quality_status(fr, r);
    const uint32_t *bits = w.bits(k) + tabs.bits_at[r];
    uint64_t *cut_off = w.cut_row(r, row);
    if (status != kOk) {
        recut_scan_wave(status, bits, tabs.final_order[r], tabs.n_units[r], byte_cap, tabs.units[r], cut_off, o.cut.sizes + row, o.cut.rcs + row);
        if (tid == 0) { o.flag[row] = 0; o.dist[row] = 0; o.equiv[row] = byte_cap; }
    } else
        (void)scan_target_wave(bits, tabs.final_order[r], tabs.n_units[r], targets.t[c], byte_cap, 0, tabs.units[r],
                               qw.energy + (size_t)k * q.e_stride + q.e_at[r], q.weight[r], q.n_families[r], q.P, q.ll_term[r], q.chan[r],
                               fr.means, cut_off, o.cut.sizes + row, o.cut.rcs + row, o.flag + row, o.dist + row, o.equiv + row);
    if (r) {
        ICER_BARRIER();
        recut_row_by_master(w, tabs, r, row, tid, blockDim.x);
    }
}

// one wavefront per frame: its curve at reduce r under the byte cap (curve_frame_wave); a frame with a status is a skipped one
__global__ void __launch_bounds__(64)
recut_budget_curve_kernel(RecutCutTables tabs, RecutWork w, uint32_t r, uint64_t byte_cap, RecutQualityTables q, RecutQualityWork qw)
{
    const uint32_t k = blockIdx.x;
    const RecutQualityFrame &fr = qw.frames[k];
    curve_frame_wave(w.bits(k) + tabs.bits_at[r], tabs.n_units[r], byte_cap, recut_quality_status(fr, r) != kOk, tabs.units[r],
                     qw.energy + (size_t)k * q.e_stride + q.e_at[r], q.weight[r], q.n_families[r], q.P, q.ll_term[r], q.chan[r], fr.means,
                     qw.curve_d + (size_t)k * qw.pitch, qw.curve_used + (size_t)k * qw.pitch, qw.head + (size_t)k * kCurveHeadWords);
}

// one workgroup per budget over all frames of the call: wavefront 0 finds the common threshold and hands out what it leaves
// over (budget_search_wave; its state: n entries of `state` per budget), then every wavefront finishes frames
// (budget_finish_wave; a frame with a status: as in recut_target_scan_kernel), and the workgroup turns the final offsets of a
// cut at r > 0 into the order of the master's units.  Rows b * n + k.
__global__ void __launch_bounds__(64 * 16)
recut_budget_search_kernel(RecutCutTables tabs, RecutWork w, uint32_t r, BudgetList budgets, uint64_t byte_cap, uint32_t n, RecutQualityWork qw,
                           RecutQualityOut o)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
#ifdef ICER_HOST_MOCK
    const uint32_t wave = 0, waves = 1, lane0 = 1;
#else
    const uint32_t wave = tid >> 6, waves = blockDim.x >> 6, lane0 = (tid & 63u) == 0u;
#endif
    BudgetState *st = qw.state + (size_t)b * n;
    if (wave == 0) budget_search_wave(qw.curve_d, qw.curve_used, qw.head, qw.pitch, n, budgets.b[b], st, o.threshold + b, o.total + b);
    ICER_BARRIER();
    for (uint32_t k = wave; k < n; k += waves) {
        const size_t row = (size_t)b * n + k;
        const int status = recut_quality_status(qw.frames[k], r);
        const uint32_t *bits = w.bits(k) + tabs.bits_at[r];
        uint64_t *cut_off = w.cut_row(r, row);
        if (status != kOk) {
            recut_scan_wave(status, bits, tabs.final_order[r], tabs.n_units[r], byte_cap, tabs.units[r], cut_off, o.cut.sizes + row, o.cut.rcs + row);
            if (lane0) { o.flag[row] = 0; o.dist[row] = 0; o.equiv[row] = byte_cap; }
        } else
            (void)budget_finish_wave(bits, tabs.final_order[r], tabs.n_units[r], st[k].lo, qw.head[(size_t)k * kCurveHeadWords], st[k].d_lo, byte_cap,
                                     0, tabs.units[r], cut_off, o.cut.sizes + row, o.cut.rcs + row, o.flag + row, o.dist + row, o.equiv + row);
    }
    if (r) {
        ICER_BARRIER();
        for (uint32_t k = 0; k < n; k++) recut_row_by_master(w, tabs, r, (size_t)b * n + k, tid, blockDim.x);
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
        HIP_TRY(recut_upload(r, &g.weight, q.weight[k].data(), sizeof(uint32_t) * g.n_families));
        HIP_TRY(recut_upload(r, &g.chan, q.chan[k].data(), sizeof(uint32_t) * g.n_families));
        HIP_TRY(recut_upload(r, &g.ll_term, q.ll_term[k].data(), sizeof(unsigned long long) * g.n_families));
        if (k) HIP_TRY(recut_upload(r, &g.fam_map, q.fam_map[k].data(), sizeof(uint32_t) * g.n_families));
    }
    HIP_TRY(recut_upload(r, &r->fam_cap, q.fam_cap.data(), sizeof(unsigned long long) * q.fam_cap.size()));
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

// what the two calls have beyond a RecutCall: the sidecars, the byte cap, their own outputs (d_threshold / d_total: the budget call's)
struct RecutQualityArgs {
    const uint64_t *d_sidecar;
    size_t sidecar_stride, byte_cap;
    int32_t *d_flag;                                  // reached / at_cap
    uint64_t *d_dist, *d_equiv, *d_threshold, *d_total;
};

// Both calls: the call's reduces and the thresholds or budgets are its cuts, the byte cap every cut's quota.  Every check
// before the first launch.
int recut_quality_async(icerx_recutter *r, const RecutCall &call, const RecutQualityArgs &a, const TargetList *targets, const BudgetList *budgets)
{
    if (!r || r->filt < 0 || !a.d_sidecar || !a.d_flag || !a.d_dist || !a.d_equiv) return ICER_INVALID_INPUT;
    if (call.n_cuts < 1 || call.n_cuts > kMaxLadder) return ICER_INVALID_INPUT;
    if (a.sidecar_stride < recut_sidecar_entries(r)) return ICER_INVALID_INPUT;
    size_t caps[kMaxLadder];
    for (int k = 0; k < call.n_cuts; k++) caps[k] = a.byte_cap;
    RecutCall c = call;
    c.quotas = caps;
    RecutRun run;
    int rc = recut_check(r, c, &run);
    if (rc != ICER_RESULT_OK) return rc;
    const RecutQualityLayout L = recut_quality_layout(r, c.n, c.data_bytes, c.n_cuts, budgets != nullptr);
    if ((rc = recut_begin(r, c, L.cut, L.total, &run)) != ICER_RESULT_OK) return rc;
    uint8_t *ws = (uint8_t *)c.workspace;
    const uint32_t n = (uint32_t)c.n, reduce = run.cuts.reduce[0];
    const RecutQualityWork qw{(RecutQualityFrame *)(ws + L.frames), (unsigned long long *)(ws + L.energy), (unsigned long long *)(ws + L.curve_d),
                              (unsigned long long *)(ws + L.curve_used), (uint32_t *)(ws + L.head), run.work.n_full + 1u,
                              (BudgetState *)(ws + L.state)};
    const RecutQualityOut o{run.out, a.d_flag, (unsigned long long *)a.d_dist, (unsigned long long *)a.d_equiv,
                            (unsigned long long *)a.d_threshold, (unsigned long long *)a.d_total};
    const RecutQualityTables q = recut_quality_tables(r);

    // per frame: packet table, bit counts, the sidecar row checked and gathered
    ICER_LAUNCH_ON(c.st, recut_quality_frame_kernel, n, kRecutPlanThreads, kWalkLds, run.masters, run.tabs, run.work, run.used, q,
                   (const unsigned long long *)a.d_sidecar, a.sidecar_stride, qw);
    HIP_TRY(hipGetLastError());
    if (targets) {
        // per frame and cut: the walk to the cut's threshold
        ICER_LAUNCH_ON(c.st, recut_target_scan_kernel, dim3(n, (unsigned)c.n_cuts), kRecutQualityScanThreads, 0, run.tabs, run.work, run.cuts,
                       *targets, (uint64_t)a.byte_cap, q, qw, o);
        HIP_TRY(hipGetLastError());
    } else {
        // per frame: its curve; per budget: the common threshold, the fill, every frame's cut
        ICER_LAUNCH_ON(c.st, recut_budget_curve_kernel, n, kRecutQualityScanThreads, 0, run.tabs, run.work, reduce, (uint64_t)a.byte_cap, q, qw);
        HIP_TRY(hipGetLastError());
        ICER_LAUNCH_ON(c.st, recut_budget_search_kernel, (unsigned)c.n_cuts, kRecutBudgetThreads, 0, run.tabs, run.work, reduce, *budgets,
                       (uint64_t)a.byte_cap, n, qw, o);
        HIP_TRY(hipGetLastError());
    }
    rc = recut_finish(run);
done:
    return rc;
}

}  // namespace

extern "C" {

int icerx_recutter_create_quality(icerx_recutter **out, int device, size_t w, size_t h, int channels, int stages, int filt, unsigned segments,
                                  int sample_bits, int max_reduce)
{
    return recutter_create(out, w, h, channels, stages, segments, sample_bits, RecutterOptions{device, max_reduce, true, filt});
}

size_t icerx_recut_sidecar_entries(const icerx_recutter *r) { return recut_sidecar_entries(r); }

uint64_t icerx_recut_target_threshold(const icerx_recutter *r, double target_mse, int reduce)
{
    uint64_t T = 0;
    return r && reduce >= 0 && reduce <= r->max_reduce && recut_target_threshold(r, target_mse, reduce, &T) ? T : 0;
}

size_t icerx_recut_target_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_cuts)
{
    return recut_sizable(r, n, n_cuts, true) ? recut_quality_layout(r, n, data_bytes, n_cuts, false).total : 0;
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
    const RecutCall c{n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, reduces, nullptr, n_cuts, d_out, out_stride, d_sizes,
                      d_rcs, d_workspace, workspace_bytes, (hipStream_t)stream};
    const RecutQualityArgs a{d_sidecar, sidecar_stride, byte_cap, d_reached, d_dist, d_equiv_quota, nullptr, nullptr};
    return recut_quality_async(r, c, a, &targets, nullptr);
}

size_t icerx_recut_budget_workspace_bytes(const icerx_recutter *r, int n, size_t data_bytes, int n_budgets)
{
    return recut_sizable(r, n, n_budgets, true) ? recut_quality_layout(r, n, data_bytes, n_budgets, true).total : 0;
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
    const RecutCall c{n, (const uint8_t *)d_data, data_bytes, d_offsets, stream_stride, d_lens, reduces, nullptr, n_budgets, d_out, out_stride,
                      d_sizes, d_rcs, d_workspace, workspace_bytes, (hipStream_t)stream};
    const RecutQualityArgs a{d_sidecar, sidecar_stride, byte_cap, d_at_cap, d_dist, d_equiv_quota, d_threshold, d_total};
    return recut_quality_async(r, c, a, nullptr, &list);
}

}  // extern "C"
