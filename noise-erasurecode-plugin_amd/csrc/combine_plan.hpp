// combine_plan.hpp -- host-side planner of rs_combine (caller-chosen GF(2^8)
// combinations of device buffers): validates the caller's job list, the
// overlap rule included, and flattens it into the device tables of the
// combine kernel.  Pure host code: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rsmi.h"

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

}  // namespace rsmi
