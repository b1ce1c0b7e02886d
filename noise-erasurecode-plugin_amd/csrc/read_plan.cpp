// read_plan.cpp -- see read_plan.hpp.
#include "read_plan.hpp"

#include <algorithm>
#include <numeric>

namespace rsmi {

namespace {
void clear(ReadPlan* plan) {
    plan->jobs.clear();
    plan->entries.clear();
    plan->copies.clear();
    plan->erased.clear();
    plan->max_j = 0;
}
}  // namespace

int plan_reads(int k, int n, size_t stripes, const uint8_t* erased, size_t dst_bytes, const rs_shard_read* reads,
               size_t count, ReadPlan* plan) {
    if (!plan || k <= 0 || n < k) return RS_EINVAL;
    clear(plan);
    if (count == 0) return RS_OK;
    if (!reads || !erased || count > 0xFFFFFFFFull) return RS_EINVAL;
    for (size_t i = 0; i < count; ++i) {
        const rs_shard_read& r = reads[i];
        if (r.reserved != 0 || r.stripe >= stripes) return RS_EINVAL;
        if (r.shard >= static_cast<uint32_t>(n)) return RS_EBAD_SHARE_ID;
        if (!r.dst || (reinterpret_cast<uintptr_t>(r.dst) & 15u)) return RS_EINVAL;
    }
    // Input positions in (stripe, shard) order: a stripe's entries become
    // adjacent, and so do duplicates.
    std::vector<uint32_t> order(count);
    std::iota(order.begin(), order.end(), 0u);
    const auto before = [&](uint32_t a, uint32_t b) {
        const rs_shard_read &x = reads[a], &y = reads[b];
        return x.stripe != y.stripe ? x.stripe < y.stripe : x.shard < y.shard;
    };
    // A list already in order (a store walking its stripes) is not sorted again.
    if (!std::is_sorted(order.begin(), order.end(), before)) std::sort(order.begin(), order.end(), before);
    for (size_t i = 1; i < count; ++i) {
        const rs_shard_read &x = reads[order[i - 1]], &y = reads[order[i]];
        if (x.stripe == y.stripe && x.shard == y.shard) return RS_EINVAL;
    }
    // Destinations in address order: neighbours closer than dst_bytes intersect.
    {
        std::vector<uintptr_t> at(count);
        for (size_t i = 0; i < count; ++i) at[i] = reinterpret_cast<uintptr_t>(reads[i].dst);
        if (!std::is_sorted(at.begin(), at.end())) std::sort(at.begin(), at.end());
        for (size_t i = 1; i < count; ++i)
            if (at[i] - at[i - 1] < dst_bytes) return RS_EINVAL;
    }
    for (size_t i = 0; i < count;) {
        const uint64_t stripe = reads[order[i]].stripe;
        const uint8_t* fl = erased + static_cast<size_t>(stripe) * static_cast<size_t>(n);
        size_t end = i;
        bool wants_missing = false;
        for (; end < count && reads[order[end]].stripe == stripe; ++end) wants_missing |= fl[reads[order[end]].shard] != 0;
        if (wants_missing) {
            int e = 0;
            for (int id = 0; id < n; ++id) e += fl[id] != 0;
            if (e > n - k) {
                clear(plan);
                return RS_ENOT_ENOUGH;
            }
            plan->jobs.push_back(ReadJob{stripe, static_cast<uint32_t>(plan->entries.size()), 0u});
            for (int id = 0; id < n; ++id) plan->erased.push_back(fl[id] != 0 ? 1 : 0);
        }
        // The stripe's entries are in shard order: the rank of a wanted erased
        // id is the number of erased ids below it, counted in one walk.
        uint32_t rank = 0, id = 0;
        for (; i < end; ++i) {
            const rs_shard_read& r = reads[order[i]];
            const uint64_t dst = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(r.dst));
            if (!fl[r.shard]) {
                plan->copies.push_back(ReadCopy{stripe, r.shard, 0u, dst});
                continue;
            }
            for (; id < r.shard; ++id) rank += fl[id] != 0;
            plan->entries.push_back(ReadEntry{dst, rank, 0u});
            plan->max_j = std::max(plan->max_j, ++plan->jobs.back().j);
        }
    }
    return RS_OK;
}

}  // namespace rsmi
