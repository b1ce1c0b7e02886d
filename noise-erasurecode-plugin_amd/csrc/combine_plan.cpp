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
    plan->ncols.clear();
    plan->first_block.clear();
    plan->mg = plan->groups = plan->iters = plan->ncols_all = plan->live = plan->first_live = 0;
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
// The per-job checks of both planners, in job order; the table sizes.
bool check_jobs(const rs_combine_job* jobs, size_t count, uint64_t* naddr, uint64_t* ncoef) {
    const auto bad_addr = [](uint64_t v) { return v == 0 || (v & 15u) != 0; };
    *naddr = *ncoef = 0;
    for (size_t b = 0; b < count; ++b) {
        const rs_combine_job& j = jobs[b];
        if (!j.src || !j.dst || !j.coef) return false;
        if (j.nsrc < 1 || j.nsrc > 256 || j.nout < 1 || j.nout > 256) return false;
        if (j.accumulate > 1 || j.reserved != 0) return false;
        for (uint32_t i = 0; i < j.nsrc; ++i)
            if (bad_addr(j.src[i])) return false;
        for (uint32_t i = 0; i < j.nout; ++i)
            if (bad_addr(j.dst[i])) return false;
        *naddr += j.nsrc + j.nout;
        *ncoef += static_cast<uint64_t>(j.nsrc) * j.nout;
    }
    return *naddr <= 0xFFFFFFFFull && *ncoef <= 0xFFFFFFFFull;  // 32-bit table offsets
}

// The checked jobs into the plan's tables; a job that `lens` gives no bytes
// keeps its place but counts for nothing.
void flatten(const rs_combine_job* jobs, size_t count, const size_t* lens, uint64_t naddr, uint64_t ncoef, CombinePlan* plan) {
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
        if (lens && lens[b] == 0) continue;
        plan->max_nsrc = std::max(plan->max_nsrc, j.nsrc);
        plan->max_nout = std::max(plan->max_nout, j.nout);
        plan->rows += j.nout;
    }
}

// forbidden_overlap for jobs of their own spans (16 * ncols[b] bytes; none: no
// ranges): the destinations, sorted by start, may not reach their successor,
// and a source range may meet neither the first destination at or above its
// start nor the one below it (the destinations being disjoint, no other can
// cover its start).
bool forbidden_overlap_lens(const CombinePlan& plan) {
    struct Range {
        uint64_t lo, hi;
    };
    std::vector<Range> dst;
    dst.reserve(static_cast<size_t>(plan.rows));
    for (size_t b = 0; b < plan.jobs.size(); ++b) {
        const CombineJob& j = plan.jobs[b];
        const uint64_t span = static_cast<uint64_t>(plan.ncols[b]) * 16;
        if (span == 0) continue;
        for (uint32_t i = j.addr + j.nsrc; i < j.addr + j.nsrc + j.nout; ++i) dst.push_back(Range{plan.addrs[i], plan.addrs[i] + span});
    }
    const auto by_start = [](const Range& a, const Range& b) { return a.lo < b.lo; };
    if (!std::is_sorted(dst.begin(), dst.end(), by_start)) std::sort(dst.begin(), dst.end(), by_start);
    uint64_t top = 0;  // the highest end of any destination
    for (size_t i = 0; i < dst.size(); ++i) {
        if (i > 0 && dst[i].lo < dst[i - 1].hi) return true;
        top = std::max(top, dst[i].hi);
    }
    const uint64_t bottom = dst.front().lo;
    uint64_t prev = 0, prev_span = 0;  // no valid address
    for (size_t b = 0; b < plan.jobs.size(); ++b) {
        const CombineJob& j = plan.jobs[b];
        const uint64_t span = static_cast<uint64_t>(plan.ncols[b]) * 16;
        if (span == 0) continue;
        for (uint32_t i = j.addr; i < j.addr + j.nsrc; ++i) {
            const uint64_t s = plan.addrs[i];
            if ((s == prev && span == prev_span) || s + span <= bottom || s >= top) continue;
            prev = s, prev_span = span;
            const auto up = std::lower_bound(dst.begin(), dst.end(), Range{s, 0}, by_start);
            if (up != dst.end() && up->lo < s + span) return true;
            if (up != dst.begin() && (up - 1)->hi > s) return true;
        }
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
    uint64_t naddr = 0, ncoef = 0;
    if (!check_jobs(jobs, count, &naddr, &ncoef)) return RS_EINVAL;
    flatten(jobs, count, nullptr, naddr, ncoef, plan);
    if (forbidden_overlap(*plan, (static_cast<uint64_t>(len) + 15) / 16 * 16)) {
        clear(plan);
        return RS_EINVAL;
    }
    return RS_OK;
}

int plan_combine_lens(const rs_combine_job* jobs, size_t count, const size_t* lens, CombinePlan* plan, uint32_t iters) {
    if (!plan) return RS_EINVAL;
    clear(plan);
    if (count == 0) return RS_OK;
    if (!jobs || !lens || count > 0xFFFFFFFEull || iters == 0) return RS_EINVAL;
    bool any = false;
    for (size_t b = 0; b < count; ++b) {
        if (lens[b] > (size_t(1) << 32) - 16) return RS_EINVAL;  // 2^28 or more columns: 32-bit column offsets, as the stripe calls
        any |= lens[b] != 0;
    }
    uint64_t naddr = 0, ncoef = 0;
    if (!check_jobs(jobs, count, &naddr, &ncoef)) return RS_EINVAL;
    if (!any) return RS_OK;
    flatten(jobs, count, lens, naddr, ncoef, plan);
    plan->mg = combine_row_group(plan->max_nsrc, plan->max_nout);
    plan->groups = (plan->max_nout + plan->mg - 1) / plan->mg;
    plan->iters = iters;
    plan->ncols.reserve(count);
    plan->first_block.reserve(count + 1);
    uint64_t blocks = 0;
    bool same = true;
    for (size_t b = 0; b < count; ++b) {
        const uint32_t nc = static_cast<uint32_t>((lens[b] + 15) / 16);
        plan->ncols.push_back(nc);
        plan->first_block.push_back(static_cast<uint32_t>(blocks));
        if (nc == 0) continue;
        if (plan->live++ == 0) plan->first_live = static_cast<uint32_t>(b), plan->ncols_all = nc;
        same &= nc == plan->ncols_all;
        blocks += static_cast<uint64_t>(combine_lens_chunks(nc, iters)) * plan->groups;
        if (blocks > 0x7FFFFFFFull) {
            clear(plan);
            return RS_EINVAL;
        }
    }
    plan->first_block.push_back(static_cast<uint32_t>(blocks));
    if (!same) plan->ncols_all = 0;
    if (forbidden_overlap_lens(*plan)) {
        clear(plan);
        return RS_EINVAL;
    }
    return RS_OK;
}

}  // namespace rsmi
