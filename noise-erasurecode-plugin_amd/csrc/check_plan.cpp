// check_plan.cpp -- see check_plan.hpp.
#include "check_plan.hpp"

#include <algorithm>

namespace rsmi {

namespace {
void clear(CheckPlan* plan) {
    plan->intact.clear();
    plan->jobs.clear();
    plan->entries.clear();
    plan->flags.clear();
    plan->saturated = 0;
    plan->max_j = 0;
}

// The planner of both placements: dst_of(stripe, id) is what an entry carries
// for the shard `id` of `stripe`.  Repair (plan_repairs): saturated stripes
// get a job too and every id of X' an entry, its pad saying stored or compared.
template <bool Repair, class DstOf>
int plan_impl(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count, DstOf dst_of,
              CheckPlan* plan) {
    if (!plan) return RS_EINVAL;
    clear(plan);
    if (k < 1 || n < k || n > 256 || stripes > 0xFFFFFFFFull) return RS_EINVAL;
    const size_t total = list ? count : stripes;
    if (total == 0) return RS_OK;
    if (!erased) return RS_EINVAL;
    const int m = n - k;
    for (size_t i = 0; i < total; ++i) {
        const uint32_t stripe = list ? list[i] : static_cast<uint32_t>(i);
        if (list && (stripe >= stripes || (i > 0 && list[i - 1] >= stripe))) {
            clear(plan);
            return RS_EINVAL;
        }
        const uint8_t* fl = erased + static_cast<size_t>(stripe) * static_cast<size_t>(n);
        int e = 0;
        for (int id = 0; id < n; ++id) e += fl[id] != 0;
        if (e > m) {
            clear(plan);
            return RS_ENOT_ENOUGH;
        }
        if (e == 0) {
            plan->intact.push_back(stripe);
            continue;
        }
        if (e == m) {
            ++plan->saturated;
            if (!Repair) continue;
        }
        // Rebuild takes every present data share and fills up to k with the
        // highest-numbered present parity: the m - e present parity shards it
        // leaves out, the lowest-numbered ones, are U (always parity shards).
        const int j = m - e;
        const uint32_t nent = static_cast<uint32_t>(Repair ? m : j);
        plan->jobs.push_back(ReadJob{stripe, static_cast<uint32_t>(plan->entries.size()), nent});
        plan->max_j = std::max(plan->max_j, nent);
        const size_t f0 = plan->flags.size();
        plan->flags.resize(f0 + static_cast<size_t>(n));
        uint8_t* xf = &plan->flags[f0];
        int left = j;  // shards of U still to come
        for (int id = 0; id < n; ++id) {
            xf[id] = fl[id] != 0 ? 1 : 0;
            if (id >= k && !xf[id] && left > 0) {
                xf[id] = 1;
                --left;
            }
        }
        // Entries in id order; the rank of an id of U is the number of ids of
        // X' below it, counted in the same walk.
        uint32_t rank = 0;
        for (int id = 0; id < n; ++id) {
            if (!xf[id]) continue;
            if (Repair)
                plan->entries.push_back(ReadEntry{dst_of(stripe, id), rank, fl[id] ? kRepairStore : kRepairCompare});
            else if (!fl[id])
                plan->entries.push_back(ReadEntry{dst_of(stripe, id), rank, 0u});
            ++rank;
        }
    }
    return RS_OK;
}
}  // namespace

int plan_checks(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                const CheckLayout& lay, CheckPlan* plan) {
    return plan_impl<false>(k, n, stripes, erased, list, count,
                            [&](uint32_t stripe, int id) {
                                return lay.parity + static_cast<uint64_t>(stripe) * lay.parity_ss +
                                       static_cast<uint64_t>(id - k) * lay.pitch;
                            },
                            plan);
}

int plan_checks_ptrs(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                     CheckPlan* plan) {
    return plan_impl<false>(k, n, stripes, erased, list, count,
                            [](uint32_t, int id) { return static_cast<uint64_t>(id); }, plan);
}

int plan_repairs(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                 const CheckLayout& lay, CheckPlan* plan) {
    return plan_impl<true>(k, n, stripes, erased, list, count,
                           [&](uint32_t stripe, int id) {
                               return id < k ? lay.data + static_cast<uint64_t>(stripe) * lay.data_ss +
                                                   static_cast<uint64_t>(id) * lay.pitch
                                             : lay.parity + static_cast<uint64_t>(stripe) * lay.parity_ss +
                                                   static_cast<uint64_t>(id - k) * lay.pitch;
                           },
                           plan);
}

int plan_repairs_ptrs(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                      CheckPlan* plan) {
    return plan_impl<true>(k, n, stripes, erased, list, count,
                           [](uint32_t, int id) { return static_cast<uint64_t>(id); }, plan);
}

}  // namespace rsmi
