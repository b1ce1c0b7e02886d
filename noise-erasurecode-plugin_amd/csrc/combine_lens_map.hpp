// combine_lens_map.hpp -- the block map of rs_combine_lens: which {job, column
// chunk, row group} a block of the per-job-length combine kernel codes.
//
// Shared by the kernel (rs_kernels.hip, rs_combine_kernel<.., VARLEN = true>)
// and the host planner (combine_plan.cpp), so the CPU tests run the very
// search the kernel runs: RSMI_HD is __host__ __device__ under hipcc and empty
// under g++.  The per-stripe-length twins of the verify, check and repair
// kernels (rs_verify_ptrs_lens, rs_reconstruct_checked_ptrs_lens) and their
// planner (scrub_lens_plan.cpp) use the same map, a "job" being a stripe.
//
// Job j of ncols[j] 16-byte columns owns the blocks
//     [first_block[j], first_block[j + 1])
// of the grid, combine_lens_chunks(ncols[j], iters) * groups of them, the row
// group changing fastest (as in the equal-length kernel).  A job of no
// columns owns none and shows as a repeated prefix value.  The tables grow
// with the jobs, never with the bytes.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#ifndef RSMI_HD
#define RSMI_HD __host__ __device__
#endif
#else
#ifndef RSMI_HD
#define RSMI_HD
#endif
#endif

namespace rsmi {

constexpr uint32_t kCombineBlockCols = 256;  // columns a block codes per iteration (its lanes)

// The row-group size of a call whose widest job has max_nsrc sources and
// max_nout outputs: the smallest of 4, 8, 16 that holds max_nout (16 beyond),
// 8 where row groups of 16 would not fit the 64 KiB LDS (328 bytes per source
// against 168: more than 199 sources).
RSMI_HD inline uint32_t combine_row_group(uint32_t max_nsrc, uint32_t max_nout) {
    const uint32_t mg = max_nout <= 4 ? 4u : max_nout <= 8 ? 8u : 16u;
    return max_nsrc * (mg / 4 * 80 + 8) <= 64 * 1024 ? mg : 8u;
}

// Column chunks of a job of `ncols` columns when a block runs up to `iters`
// iterations: block chunk c codes the columns (c + it * chunks) * 256 + lane,
// it < iters, that the job has.
RSMI_HD inline uint32_t combine_lens_chunks(uint32_t ncols, uint32_t iters) {
    const uint32_t total_it = (ncols + kCombineBlockCols - 1) / kCombineBlockCols;
    const uint32_t it = total_it < iters ? total_it : iters;
    return it ? (total_it + it - 1) / it : 0;
}

struct CombineBlock {
    uint32_t job, chunk, grp;
    uint32_t chunks;  // the job's column chunks: its blocks / groups
};

// The one job with first_block[job] <= b < first_block[job + 1], and b's place
// in it.  Needs njobs >= 1, first_block[0] == 0 and b < first_block[njobs].
// Every operand is uniform across a block, so on the device the search is
// scalar loads and scalar compares.
RSMI_HD inline CombineBlock combine_lens_block(const uint32_t* first_block, uint32_t njobs, uint32_t groups, uint32_t b) {
    uint32_t lo = 0, hi = njobs;  // first_block[lo] <= b < first_block[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first_block[mid] <= b) lo = mid;
        else hi = mid;
    }
    const uint32_t base = first_block[lo], r = b - base;
    CombineBlock out;
    out.job = lo;
    out.grp = r % groups;
    out.chunk = r / groups;
    out.chunks = (first_block[lo + 1] - base) / groups;
    return out;
}

}  // namespace rsmi
