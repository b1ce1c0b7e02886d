// combine_plan.cpp -- see combine_plan.hpp.
#include "combine_plan.hpp"

#include <algorithm>

namespace rsmi {

namespace {
void clear(CombinePlan* plan) {
    plan->jobs.clear();
    plan->addrs.clear();
    plan->coef.clear();
    plan->max_nsrc = plan->max_nout = 0;
    plan->rows = 0;
}

// Whether a destination range meets a source range or another destination
// range; all ranges are `span` bytes long, so two of them meet exactly when
// their starts are less than span apart.
bool forbidden_overlap(const CombinePlan& plan, uint64_t span) {
    std::vector<uint64_t> dst;
    dst.reserve(static_cast<size_t>(plan.rows));
    for (const CombineJob& j : plan.jobs)
        dst.insert(dst.end(), plan.addrs.begin() + j.addr + j.nsrc, plan.addrs.begin() + j.addr + j.nsrc + j.nout);
    // Destinations in address order (a caller carving them out of one buffer
    // lists them so already): neighbours closer than span intersect.
    if (!std::is_sorted(dst.begin(), dst.end())) std::sort(dst.begin(), dst.end());
    for (size_t i = 1; i < dst.size(); ++i)
        if (dst[i] - dst[i - 1] < span) return true;
    // A source meets a destination if the first destination at or above it,
    // or the one below that, starts less than span away.  Sources clear of
    // the whole extent of the destinations (the usual case: outputs in a
    // buffer of their own) are not looked up, and consecutive equal sources
    // (one buffer shared by many jobs) only once.
    const uint64_t lo = dst.front(), hi = dst.back();
    uint64_t prev = 0;  // no valid address
    for (const CombineJob& j : plan.jobs)
        for (uint32_t i = j.addr; i < j.addr + j.nsrc; ++i) {
            const uint64_t s = plan.addrs[i];
            if (s == prev || (s < lo && lo - s >= span) || (s > hi && s - hi >= span)) continue;
            prev = s;
            const auto up = std::lower_bound(dst.begin(), dst.end(), s);
            if (up != dst.end() && *up - s < span) return true;
            if (up != dst.begin() && s - *(up - 1) < span) return true;
        }
    return false;
}
}  // namespace

int plan_combine(const rs_combine_job* jobs, size_t count, size_t len, CombinePlan* plan) {
    if (!plan) return RS_EINVAL;
    clear(plan);
    if (count == 0 || len == 0) return RS_OK;
    if (!jobs || count > 0xFFFFFFFFull) return RS_EINVAL;
    if ((len + 15) / 16 >= (size_t(1) << 28)) return RS_EINVAL;  // 32-bit column offsets, as the stripe calls
    const auto bad_addr = [](uint64_t v) { return v == 0 || (v & 15u) != 0; };
    uint64_t naddr = 0, ncoef = 0;
    for (size_t b = 0; b < count; ++b) {
        const rs_combine_job& j = jobs[b];
        if (!j.src || !j.dst || !j.coef) return RS_EINVAL;
        if (j.nsrc < 1 || j.nsrc > 256 || j.nout < 1 || j.nout > 256) return RS_EINVAL;
        if (j.accumulate > 1 || j.reserved != 0) return RS_EINVAL;
        for (uint32_t i = 0; i < j.nsrc; ++i)
            if (bad_addr(j.src[i])) return RS_EINVAL;
        for (uint32_t i = 0; i < j.nout; ++i)
            if (bad_addr(j.dst[i])) return RS_EINVAL;
        naddr += j.nsrc + j.nout;
        ncoef += static_cast<uint64_t>(j.nsrc) * j.nout;
    }
    if (naddr > 0xFFFFFFFFull || ncoef > 0xFFFFFFFFull) return RS_EINVAL;  // 32-bit table offsets
    plan->jobs.reserve(count);
    plan->addrs.reserve(static_cast<size_t>(naddr));
    plan->coef.reserve(static_cast<size_t>(ncoef));
    for (size_t b = 0; b < count; ++b) {
        const rs_combine_job& j = jobs[b];
        plan->jobs.push_back(CombineJob{static_cast<uint32_t>(plan->addrs.size()), static_cast<uint32_t>(plan->coef.size()),
                                        static_cast<uint16_t>(j.nsrc), static_cast<uint16_t>(j.nout), j.accumulate});
        plan->addrs.insert(plan->addrs.end(), j.src, j.src + j.nsrc);
        plan->addrs.insert(plan->addrs.end(), j.dst, j.dst + j.nout);
        plan->coef.insert(plan->coef.end(), j.coef, j.coef + static_cast<size_t>(j.nsrc) * j.nout);
        plan->max_nsrc = std::max(plan->max_nsrc, j.nsrc);
        plan->max_nout = std::max(plan->max_nout, j.nout);
        plan->rows += j.nout;
    }
    if (forbidden_overlap(*plan, (static_cast<uint64_t>(len) + 15) / 16 * 16)) {
        clear(plan);
        return RS_EINVAL;
    }
    return RS_OK;
}

}  // namespace rsmi
