// update_plan.cpp -- see update_plan.hpp.
#include "update_plan.hpp"

#include <algorithm>
#include <numeric>

namespace rsmi {

int plan_updates(int k, size_t stripes, const rs_shard_update* updates, size_t count, UpdatePlan* plan) {
    if (!plan || k <= 0) return RS_EINVAL;
    plan->jobs.clear();
    plan->entries.clear();
    plan->max_j = 0;
    if (count == 0) return RS_OK;
    if (!updates || count > 0xFFFFFFFFull) return RS_EINVAL;
    for (size_t i = 0; i < count; ++i) {
        const rs_shard_update& u = updates[i];
        if (u.reserved != 0 || u.stripe >= stripes) return RS_EINVAL;
        if (u.shard >= static_cast<uint32_t>(k)) return RS_EBAD_SHARE_ID;
        if (!u.src || (reinterpret_cast<uintptr_t>(u.src) & 15u)) return RS_EINVAL;
    }
    // Input positions in (stripe, shard) order: a stripe's entries become
    // adjacent, and so do duplicates.
    std::vector<uint32_t> order(count);
    std::iota(order.begin(), order.end(), 0u);
    const auto before = [&](uint32_t a, uint32_t b) {
        const rs_shard_update &x = updates[a], &y = updates[b];
        return x.stripe != y.stripe ? x.stripe < y.stripe : x.shard < y.shard;
    };
    // A list already in order (a store walking its stripes) is not sorted again.
    if (!std::is_sorted(order.begin(), order.end(), before)) std::sort(order.begin(), order.end(), before);
    for (size_t i = 1; i < count; ++i) {
        const rs_shard_update &x = updates[order[i - 1]], &y = updates[order[i]];
        if (x.stripe == y.stripe && x.shard == y.shard) return RS_EINVAL;
    }
    plan->entries.reserve(count);
    for (size_t i = 0; i < count; ++i) {
        const rs_shard_update& u = updates[order[i]];
        if (plan->jobs.empty() || plan->jobs.back().stripe != u.stripe)
            plan->jobs.push_back(UpdateJob{u.stripe, static_cast<uint32_t>(i), 0u});
        plan->max_j = std::max(plan->max_j, ++plan->jobs.back().j);
        plan->entries.push_back(UpdateEntry{static_cast<uint64_t>(reinterpret_cast<uintptr_t>(u.src)), u.shard, 0u});
    }
    return RS_OK;
}

}  // namespace rsmi
