// scrub_lens_plan.cpp -- see scrub_lens_plan.hpp.
#include "scrub_lens_plan.hpp"

namespace rsmi {

namespace {
void clear(ScrubLensPlan* plan) { *plan = ScrubLensPlan{}; }

// The block map of one list; returns its blocks (64 bits: the caller refuses).
template <class StripeOf>
uint64_t lay_blocks(size_t count, StripeOf stripe_of, const size_t* lens, uint32_t groups, uint32_t iters,
                    ScrubLensList* out) {
    out->groups = count ? groups : 0;
    if (count == 0) return 0;
    out->ncols.reserve(count);
    out->lens.reserve(count);
    out->first_block.reserve(count + 1);
    uint64_t blocks = 0;
    for (size_t b = 0; b < count; ++b) {
        const size_t len = lens[stripe_of(b)];
        const uint32_t ncols = static_cast<uint32_t>((len + 15) / 16);
        out->ncols.push_back(ncols);
        out->lens.push_back(static_cast<uint32_t>(len));
        // Past the limit the prefix values are never used: the call is refused.
        out->first_block.push_back(static_cast<uint32_t>(blocks));
        blocks += static_cast<uint64_t>(combine_lens_chunks(ncols, iters)) * groups;
    }
    out->first_block.push_back(static_cast<uint32_t>(blocks));
    return blocks;
}
}  // namespace

int plan_scrub_lens(int k, int n, size_t stripes, const uint8_t* erased, const size_t* lens, bool repair,
                    uint32_t intact_groups, uint32_t iters, ScrubLensPlan* plan) {
    if (!plan) return RS_EINVAL;
    clear(plan);
    if (k < 1 || n < k || n > 256 || stripes > 0xFFFFFFFFull || iters == 0) return RS_EINVAL;
    if (stripes == 0) return RS_OK;
    if (!lens || (repair && !erased)) return RS_EINVAL;
    const int m = n - k;
    // The stripes that have bytes; every stripe's flags count, with or without.
    std::vector<uint32_t> list;
    bool same = true;
    for (size_t s = 0; s < stripes; ++s) {
        if (lens[s] > ((size_t(1) << 28) - 1) * 16) return RS_EINVAL;  // 32-bit column offsets: below 2^28 columns
        if (lens[s] != lens[0]) same = false;
        if (lens[s] != 0) list.push_back(static_cast<uint32_t>(s));
    }
    if (erased) {
        for (size_t s = 0; s < stripes; ++s) {
            const uint8_t* fl = erased + s * static_cast<size_t>(n);
            int e = 0;
            for (int id = 0; id < n; ++id) e += fl[id] != 0;
            if (e > m) return RS_ENOT_ENOUGH;
        }
    }
    plan->iters = iters;
    plan->live = list.size();
    plan->len_all = same ? static_cast<uint32_t>(lens[0]) : 0u;
    if (list.empty()) return RS_OK;
    if (erased) {
        const int rc = repair ? plan_repairs_ptrs(k, n, stripes, erased, list.data(), list.size(), &plan->checks)
                              : plan_checks_ptrs(k, n, stripes, erased, list.data(), list.size(), &plan->checks);
        if (rc != RS_OK) {
            clear(plan);
            return rc;
        }
    } else {
        plan->checks.intact = list;
    }
    const CheckPlan& cp = plan->checks;
    const uint32_t job_groups = (cp.max_j + kScrubLensJobRows - 1) / kScrubLensJobRows;
    uint64_t blocks =
        lay_blocks(cp.intact.size(), [&](size_t b) { return cp.intact[b]; }, lens, intact_groups, iters, &plan->intact);
    blocks += lay_blocks(cp.jobs.size(), [&](size_t b) { return cp.jobs[b].stripe; }, lens, job_groups, iters, &plan->jobs);
    if (blocks > kScrubLensMaxBlocks) {
        clear(plan);
        return RS_EINVAL;
    }
    return RS_OK;
}

}  // namespace rsmi
