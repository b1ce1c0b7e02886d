// scrub_lens_plan.hpp -- host-side planner of rs_verify_ptrs_lens /
// rs_reconstruct_checked_ptrs_lens: the pointer-mode scrub of stripes that
// each have a shard length of their own.  It validates the lengths and every
// stripe's flags, leaves the stripes without bytes out, plans the others with
// plan_checks_ptrs / plan_repairs_ptrs, and lays the block map
// (combine_lens_map.hpp) over the two lists the kernels run: the intact
// stripes (the verify kernel) and the jobs (the check or the repair kernel).
// Pure host code: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "check_plan.hpp"
#include "combine_lens_map.hpp"

namespace rsmi {

// One list of the plan: entry b is a stripe of ncols[b] >= 1 16-byte columns
// and lens[b] bytes that owns the blocks [first_block[b], first_block[b + 1])
// of its launch, combine_lens_chunks(ncols[b], iters) * groups of them.
struct ScrubLensList {
    std::vector<uint32_t> ncols;
    std::vector<uint32_t> lens;
    std::vector<uint32_t> first_block;  // [entries + 1]; empty without entries
    uint32_t groups = 0;                // row groups per column chunk (0: nothing to launch)
    uint32_t blocks() const { return first_block.empty() ? 0u : first_block.back(); }
};

struct ScrubLensPlan {
    CheckPlan checks;      // plan_checks_ptrs' / plan_repairs_ptrs' plan of the stripes that have bytes
    ScrubLensList intact;  // over checks.intact
    ScrubLensList jobs;    // over checks.jobs
    uint32_t iters = 1;    // the most iterations a block runs
    size_t live = 0;       // stripes that have bytes
    uint32_t len_all = 0;  // the one length of every stripe of the call (all live), or 0
};

constexpr uint64_t kScrubLensMaxBlocks = 0x7FFFFFFFull;  // over both launches
constexpr uint32_t kScrubLensJobRows = 4;                // row group of the check and repair kernels

// Plans the scrub of RS(k, n) stripes [0, stripes) with the erasure flags
// erased[stripes][n] (non-zero = missing; NULL: nothing is missing, verify
// only) and the shard lengths lens[stripes].  repair: plan_repairs_ptrs' jobs
// (every stripe with 1..m erasures), else plan_checks_ptrs'.  intact_groups:
// the row groups of the verify variant for the code (0 when m is 0); the
// jobs' are ceil(max_j / 4).  iters: the cap on a block's iterations (>= 1).
// RS_OK and the plan, or, with the plan left empty:
//   RS_EINVAL       plan or lens NULL (stripes > 0), erased NULL for a repair,
//                   k < 1, n < k, n > 256, stripes >= 2^32, iters == 0, a
//                   length of 2^28 or more 16-byte columns, more than 2^31 - 1
//                   blocks in all
//   RS_ENOT_ENOUGH  a stripe -- with or without bytes -- has more than n - k
//                   erasures
int plan_scrub_lens(int k, int n, size_t stripes, const uint8_t* erased, const size_t* lens, bool repair,
                    uint32_t intact_groups, uint32_t iters, ScrubLensPlan* plan);

}  // namespace rsmi
