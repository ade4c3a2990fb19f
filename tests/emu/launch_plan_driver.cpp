// TESTS ONLY: a C ABI over csrc/launch_plan.hpp for tests/test_launch_plan.py.  `env` is "NAME=value,NAME=value" and stands in
// for the process environment.
#include "../../icer_compression_amd/csrc/launch_plan.hpp"
#include <map>
#include <string>

using namespace icer;

static Tuning tuning_of(const char *env)
{
    std::map<std::string, std::string> vars;
    std::string s = env ? env : "";
    for (size_t at = 0; at < s.size();) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        const std::string kv = s.substr(at, end - at);
        const size_t eq = kv.find('=');
        if (eq != std::string::npos) vars[kv.substr(0, eq)] = kv.substr(eq + 1);
        at = end + 1;
    }
    return parse_tuning([&](const char *name) -> const char * {
        auto it = vars.find(name);
        return it == vars.end() ? nullptr : it->second.c_str();
    });
}

extern "C" void lp_tuning(const char *env, int *out)
{
    const Tuning t = tuning_of(env);
    const int v[] = {t.coder, t.pipe_waves, t.hybrid_percent, t.hybrid_frames, (int)t.split_chunks, t.list_waves, (int)t.slot_bpp,
                     t.overlap_parts, t.fail_frame, t.fail_unit, t.fail_calls};
    for (int i = 0; i < 11; i++) out[i] = v[i];
}

// The decision of one call, the way the library reaches it: the encoder plans sub-ranges (`planned_subs` workgroups per frame)
// only if plans_sub_ranges says so, and has the stream of the odd parts only if its window coder was granted and
// wants_half_stream says so.  out: progressive, use_wg, parts, sub-ranges planned, then kMaxParts x 11 words per part.
extern "C" void lp_plan(const char *env, int channels, long w, long h, int max_frames, int n_cus, int planned_subs, int wg_available, int wg_once,
                        int n_frames, unsigned long long quota, int overlap_ok, int *out)
{
    const Tuning t = tuning_of(env);
    LaunchShape s;
    s.channels = channels; s.w = (size_t)w; s.h = (size_t)h; s.max_frames = max_frames; s.n_cus = n_cus;
    const bool planned = plans_sub_ranges(s, t, wg_available != 0);
    s.n_subs = planned ? (uint32_t)planned_subs : 0u;
    CoderState st;
    st.wg_available = wg_available != 0; st.wg_once = wg_once != 0; st.half_stream = st.wg_available && wants_half_stream(s, t);
    const LaunchPlan p = plan_launch(s, t, st, n_frames, (size_t)quota, overlap_ok != 0);
    out[0] = p.progressive; out[1] = p.use_wg; out[2] = p.n_parts; out[3] = planned;
    for (int k = 0; k < kMaxParts; k++) {
        const PartPlan &q = p.part[k];
        const int v[] = {q.f0, q.n_frames, q.hybrid, q.split, (int)q.subs, (int)q.list_grid, (int)q.list, (int)q.route_percent, (int)q.pipe,
                         q.position_major, (int)q.window};
        for (int i = 0; i < 11; i++) out[4 + 11 * k + i] = v[i];
    }
}
