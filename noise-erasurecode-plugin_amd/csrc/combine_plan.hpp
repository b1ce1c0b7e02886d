// combine_plan.hpp -- host-side planner of rs_combine (caller-chosen GF(2^8)
// combinations of device buffers): validates the caller's job list, the
// overlap rule included, and flattens it into the device tables of the
// combine kernel.  Pure host code: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rsmi.h"
#include "combine_lens_map.hpp"

namespace rsmi {

// One job: addresses [addr, addr + nsrc) of the address table are its sources,
// [addr + nsrc, addr + nsrc + nout) its destinations; its nout x nsrc row-major
// coefficients start at byte `coef` of the coefficient table.
struct CombineJob {
    uint32_t addr;
    uint32_t coef;
    uint16_t nsrc;        // 1..256
    uint16_t nout;        // 1..256
    uint32_t accumulate;  // 0: dst = sum, 1: dst ^= sum
};
static_assert(sizeof(CombineJob) == 16, "device table record");

struct CombinePlan {
    std::vector<CombineJob> jobs;  // in the caller's order
    std::vector<uint64_t> addrs;   // device addresses: a job's sources, then its destinations
    std::vector<uint8_t> coef;     // the jobs' coefficient matrices, one after another
    uint32_t max_nsrc = 0;         // the largest nsrc of any job
    uint32_t max_nout = 0;         // the largest nout of any job
    uint64_t rows = 0;             // output rows of all jobs
    // plan_combine_lens only (combine_lens_map.hpp); empty after plan_combine.
    std::vector<uint32_t> ncols;        // 16-byte columns of each job
    std::vector<uint32_t> first_block;  // jobs + 1 entries: exclusive prefix sum of the jobs' block counts
    uint32_t mg = 0, groups = 0;        // combine_row_group(max_nsrc, max_nout) and the row groups of the widest job
    uint32_t iters = 0;                 // iterations per block the block counts were made for
    uint32_t ncols_all = 0;             // the common column count of the jobs that have columns, 0 when they differ
    uint32_t live = 0;                  // jobs that have columns
    uint32_t first_live = 0;            // the first of them
};

// Plans `count` jobs over buffers of `len` bytes.  RS_OK and the plan (empty
// for count == 0 or len == 0), or RS_EINVAL with the plan left empty for:
// jobs == NULL, count >= 2^32, a len the stripe calls refuse (2^28 or more
// 16-byte columns), a job with src, dst or coef NULL, nsrc or nout outside
// 1..256, accumulate > 1, reserved != 0, a NULL or misaligned address, tables
// of 2^32 or more addresses or coefficient bytes, or a forbidden overlap: with
// span = round_up(len, 16), a dst range [d, d + span) that meets the range of
// any src or of any other dst of the call.  Sources may repeat and overlap.
// The jobs are checked in order; overlaps are looked for last, by sorting the
// destinations (never pair by pair).
int plan_combine(const rs_combine_job* jobs, size_t count, size_t len, CombinePlan* plan);

// plan_combine with job b over buffers of lens[b] bytes: span_b =
// round_up(lens[b], 16) in the overlap rule -- a dst range [d, d + span_b) may
// meet neither [s, s + span_b') of a src of any job b' nor another dst range
// -- and the block map of the per-job-length kernel (ncols, first_block, for
// blocks of up to `iters` iterations and the call-wide row groups).  A job
// with lens[b] == 0 is validated like any other and keeps its place in the
// tables, but contributes no ranges to the overlap check, no blocks (a
// repeated prefix value) and nothing to max_nsrc, max_nout and rows.
// RS_EINVAL additionally for lens == NULL with count > 0, any lens[b] of 2^28
// or more columns, or more than 2^31 - 1 blocks in all.  count == 0 or all
// lengths 0: RS_OK and an empty plan.
int plan_combine_lens(const rs_combine_job* jobs, size_t count, const size_t* lens, CombinePlan* plan, uint32_t iters = 1);

}  // namespace rsmi
