// update_degraded_plan.hpp -- host-side planner of rs_update_degraded (the
// in-place parity update of device-resident stripes with missing shards):
// plan_updates' list checks, then, per stripe, the changed shards split into
// present and erased ones, the present parity rows and the erasure flags of
// the stripes that need a decode pattern.  Pure host code: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rsmi.h"
#include "update_plan.hpp"

namespace rsmi {

constexpr uint32_t kDegPresent = 0xFFFFFFFFu;    // DegEntry::rank of a present shard
constexpr uint32_t kDegNoPattern = 0xFFFFFFFFu;  // DegJob::pat of a job coded in pair form

// One stripe's updates: entries [first, first + j) of the entry table, the
// j - jx present ones first, then the jx erased ones; its outputs are parity
// rows rows[row_first .. row_first + nrows), the present ones.  All updates of
// a stripe are in one job (UpdateJob).
struct DegJob {
    uint64_t stripe;
    uint32_t first;
    uint32_t j;
    uint32_t jx;
    uint32_t row_first;
    uint32_t nrows;
    uint32_t pat;  // kDegNoPattern from the planner; the caller stores the pattern id of a
                   // job it launches in decode form (jx > 0)
};
// One changed data shard.  rank: kDegPresent, or the shard's rank among the
// stripe's erased ids in increasing order -- the row of the stripe's decode
// pattern that regenerates its old contents (rs_pattern_rows).  old: 0 from
// the planner (a present shard's old contents are in its slot); the caller
// stores the address of regenerated old contents for the pair form.
struct DegEntry {
    uint64_t src;
    uint64_t old;
    uint32_t shard;
    uint32_t rank;
};
static_assert(sizeof(DegJob) == 32 && sizeof(DegEntry) == 24, "device table records");

// The extent of the call's data and parity regions, [d0, d1) and [p0, p1),
// and the bytes read at every src (round_up(shard_len, 16)).
struct UpdateExtent {
    uintptr_t d0, d1, p0, p1;
    size_t span;
};

struct UpdateDegradedPlan {
    std::vector<DegJob> jobs;       // ordered by stripe index
    std::vector<DegEntry> entries;  // a job's present entries, then its erased ones, each by shard id
    std::vector<uint32_t> rows;     // the jobs' present parity rows (0 .. m - 1), increasing per job
    std::vector<uint8_t> erased;    // [decode_jobs][n]: the erasure flags, 0 / 1, of the jobs with
                                    // jx > 0, in job order (the pattern lookup's input)
    uint32_t decode_jobs = 0;       // jobs with jx > 0
    uint32_t max_j = 0;             // the largest j of any job
    uint32_t max_src = 0;           // the widest source count: k + j for a job with jx > 0, else j
    uint64_t absorbed = 0;          // erased changed shards of all jobs
    bool degraded = false;          // some listed stripe has a flag set
};

// Plans `count` updates of RS(k, n) stripes [0, stripes) with the erasure
// flags erased[stripes][n] (non-zero = missing).  RS_OK and the plan (empty for
// count == 0), or, with the plan left empty:
//   RS_EINVAL, RS_EBAD_SHARE_ID   as plan_updates, plus NULL erased with
//                     count > 0 and, with `extent`, a src range that meets the
//                     data or the parity region
//   RS_ENOT_ENOUGH    a listed stripe with an erased changed shard has more
//                     than n - k erasures
// Defects of the list are reported first; the flags are looked at last, and
// only those of listed stripes.  A listed stripe with more than n - k erasures
// whose changed shards are all present is planned: its patch needs no decode.
int plan_update_degraded(int k, int n, size_t stripes, const uint8_t* erased, const rs_shard_update* updates,
                         size_t count, const UpdateExtent* extent, UpdateDegradedPlan* plan);

}  // namespace rsmi
