// update_degraded_plan.cpp -- see update_degraded_plan.hpp.
#include "update_degraded_plan.hpp"

#include <algorithm>

namespace rsmi {

namespace {
void clear(UpdateDegradedPlan* plan) {
    plan->jobs.clear();
    plan->entries.clear();
    plan->rows.clear();
    plan->erased.clear();
    plan->decode_jobs = 0;
    plan->max_j = 0;
    plan->max_src = 0;
    plan->absorbed = 0;
    plan->degraded = false;
}
}  // namespace

int plan_update_degraded(int k, int n, size_t stripes, const uint8_t* erased, const rs_shard_update* updates,
                         size_t count, const UpdateExtent* extent, UpdateDegradedPlan* plan) {
    if (!plan || k <= 0 || n < k) return RS_EINVAL;
    clear(plan);
    if (count == 0) return RS_OK;
    if (!erased) return RS_EINVAL;
    UpdatePlan base;
    const int rc = plan_updates(k, stripes, updates, count, &base);
    if (rc != RS_OK) return rc;
    if (extent) {
        for (const UpdateEntry& e : base.entries) {
            const uintptr_t s0 = static_cast<uintptr_t>(e.src), s1 = s0 + extent->span;
            if ((s0 < extent->d1 && extent->d0 < s1) || (s0 < extent->p1 && extent->p0 < s1)) return RS_EINVAL;
        }
    }
    const int m = n - k;
    plan->entries.reserve(base.entries.size());
    for (const UpdateJob& bj : base.jobs) {
        const uint8_t* fl = erased + static_cast<size_t>(bj.stripe) * static_cast<size_t>(n);
        int e = 0;
        for (int id = 0; id < n; ++id) e += fl[id] != 0;
        DegJob job{bj.stripe, static_cast<uint32_t>(plan->entries.size()), bj.j, 0u,
                   static_cast<uint32_t>(plan->rows.size()), 0u, kDegNoPattern};
        // The base job's entries are in shard order: the present ones first ...
        for (uint32_t i = bj.first; i < bj.first + bj.j; ++i) {
            const UpdateEntry& u = base.entries[i];
            if (!fl[u.shard]) plan->entries.push_back(DegEntry{u.src, 0u, u.shard, kDegPresent});
        }
        // ... then the erased ones: the rank of an erased id is the number of
        // erased ids below it, counted in one walk.
        uint32_t rank = 0, id = 0;
        for (uint32_t i = bj.first; i < bj.first + bj.j; ++i) {
            const UpdateEntry& u = base.entries[i];
            if (!fl[u.shard]) continue;
            for (; id < u.shard; ++id) rank += fl[id] != 0;
            plan->entries.push_back(DegEntry{u.src, 0u, u.shard, rank});
            ++job.jx;
        }
        if (job.jx > 0 && e > m) {
            clear(plan);
            return RS_ENOT_ENOUGH;
        }
        for (int r = 0; r < m; ++r)
            if (!fl[k + r]) plan->rows.push_back(static_cast<uint32_t>(r));
        job.nrows = static_cast<uint32_t>(plan->rows.size()) - job.row_first;
        if (job.jx > 0) {
            for (int i = 0; i < n; ++i) plan->erased.push_back(fl[i] != 0 ? 1 : 0);
            ++plan->decode_jobs;
            plan->absorbed += job.jx;
        }
        plan->degraded |= e > 0;
        plan->max_j = std::max(plan->max_j, job.j);
        plan->max_src = std::max(plan->max_src, job.jx > 0 ? static_cast<uint32_t>(k) + job.j : job.j);
        plan->jobs.push_back(job);
    }
    return RS_OK;
}

}  // namespace rsmi
