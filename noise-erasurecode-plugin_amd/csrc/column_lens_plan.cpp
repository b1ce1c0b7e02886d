// column_lens_plan.cpp -- see column_lens_plan.hpp.
#include "column_lens_plan.hpp"

#include <map>

namespace rsmi {

static_assert(kColumnLensClean == RS_VERIFY_CLEAN, "the verify calls' clean verdict");

int plan_column_lens(int k, int n, size_t stripes, const uint8_t* erased, const size_t* lens, ColumnLensPlan* plan) {
    if (!plan) return RS_EINVAL;
    *plan = ColumnLensPlan{};
    if (k < 1 || n < k || n > 256 || n - k > kColumnLensMaxParity || stripes > 0xFFFFFFFFull) return RS_EINVAL;
    if (stripes == 0) return RS_OK;
    if (!lens) return RS_EINVAL;
    const int m = n - k;
    bool same = true;
    for (size_t s = 0; s < stripes; ++s) {
        if (lens[s] > ((size_t(1) << 28) - 1) * 16) return RS_EINVAL;  // 32-bit column offsets: below 2^28 columns
        if (lens[s] != lens[0]) same = false;
    }
    bool degraded = false;
    for (size_t s = 0; erased && s < stripes; ++s) {
        const uint8_t* fl = erased + s * static_cast<size_t>(n);
        int e = 0;
        for (int id = 0; id < n; ++id) e += fl[id] != 0;
        if (e > m) return RS_ENOT_ENOUGH;
        degraded |= e > 0;
    }
    uint64_t blocks = 0;
    for (size_t s = 0; s < stripes; ++s)
        if (lens[s] != 0) blocks += column_lens_blocks(static_cast<uint32_t>((lens[s] + 15) / 16));
    if (blocks > kColumnLensMaxBlocks) return RS_EINVAL;
    for (size_t s = 0; s < stripes; ++s)
        if (lens[s] != 0) plan->live.push_back(static_cast<uint32_t>(s));
    plan->worst_blocks = blocks;
    plan->len_all = same ? static_cast<uint32_t>(lens[0]) : 0u;
    plan->degraded = degraded;
    return RS_OK;
}

void plan_column_lens_jobs(int k, int n, size_t stripes, const uint8_t* erased, const size_t* lens,
                           const ColumnLensPlan& plan, const uint32_t* first_bad, ColumnLensJobs* out) {
    *out = ColumnLensJobs{};
    out->masked.assign(stripes, 0);
    std::map<std::vector<uint8_t>, uint32_t> index;
    std::vector<uint8_t> flags(static_cast<size_t>(n), 0);
    uint32_t blocks = 0;  // at most plan.worst_blocks <= 2^31 - 1
    for (const uint32_t s : plan.live) {
        if (first_bad[s] == kColumnLensClean) continue;
        int r = n;
        for (int id = 0; id < n; ++id) {
            flags[id] = erased && erased[static_cast<size_t>(s) * n + id] != 0 ? 1 : 0;
            r -= flags[id];
        }
        if (r - k < 2) {
            out->hopeless.push_back(s);
            continue;
        }
        const auto at = index.emplace(flags, static_cast<uint32_t>(out->sets.size()));
        if (at.second) out->sets.push_back(flags);
        const uint32_t ncols = static_cast<uint32_t>((lens[s] + 15) / 16);
        out->jobs.push_back(ColumnLensJob{s, at.first->second, static_cast<uint32_t>(r), static_cast<uint32_t>(r - k)});
        out->ncols.push_back(ncols);
        out->lens.push_back(static_cast<uint32_t>(lens[s]));
        out->first_block.push_back(blocks);
        blocks += column_lens_blocks(ncols);
        out->masked[s] = lens[s];
    }
    if (!out->jobs.empty()) out->first_block.push_back(blocks);
}

}  // namespace rsmi
