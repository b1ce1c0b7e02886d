// check_plan.hpp -- host-side planner of rs_verify_degraded / rs_correct_degraded
// (the scrub of device-resident stripes with missing shards): counts every
// stripe's erasures, splits the stripes into intact, degraded and saturated
// ones, and turns each degraded stripe into one job of the check kernel.
// Pure host code: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rsmi.h"
#include "read_plan.hpp"

namespace rsmi {

// The strided layout of rs_encode_stripes, as addresses.
struct CheckLayout {
    uint64_t data, parity;               // device addresses of the two regions
    uint64_t data_ss, parity_ss, pitch;  // stripe strides and shard pitch (bytes)
};

// A degraded stripe with erasure set X, |X| = e, 1 <= e < m, is checked
// against the k survivors C that Rebuild chooses for X (data shares first,
// then the highest-numbered parity): its present shards lie on one codeword
// iff every shard of U = present \ C equals its value computed from C.  The
// decode pattern of the erasure set X' = X + U (exactly m ids, the same
// survivors C) holds those rows: row t regenerates the t-th id of X'.
struct CheckPlan {
    std::vector<uint32_t> intact;    // stripes without erasures, increasing: the verify kernel's
    std::vector<ReadJob> jobs;       // one per degraded stripe, in stripe order
    std::vector<ReadEntry> entries;  // a job's entries are its shards of U in id order:
                                     // {dst = address of the stored shard (plan_checks_ptrs: its
                                     // id), row = rank of the id in X'}
    std::vector<uint8_t> flags;      // [jobs.size()][n]: X' of every job, 0 / 1
    size_t saturated = 0;            // stripes with exactly m erasures (and m > 0): nothing to check
    uint32_t max_j = 0;              // the largest j = m - e of any job
};

// Plans the check of RS(k, n) stripes [0, stripes) -- or, with list != nullptr,
// of the `count` stripes list[0 .. count), strictly increasing -- with the
// erasure flags erased[stripes][n] (non-zero = missing; only the flags of the
// planned stripes are examined).  RS_OK and the plan, or, with the plan left
// empty:
//   RS_EINVAL       plan or erased NULL, k < 1, n < k, n > 256, stripes >= 2^32,
//                   a listed stripe >= stripes or out of order
//   RS_ENOT_ENOUGH  a planned stripe has more than n - k erasures
int plan_checks(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                const CheckLayout& lay, CheckPlan* plan);

// The same plan for the pointer placement (rs_verify_ptrs,
// rs_correct_columns_ptrs), where shard i of stripe s is at the device table's
// shard_ptrs[s * n + i] and the host knows no address: an entry's dst is the
// shard ID of the stored shard, which the check kernel resolves through the
// table.  Everything else -- the splits, the jobs, the rows, the flags, the
// refusals -- is plan_checks'.
int plan_checks_ptrs(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                     CheckPlan* plan);

// The plan of rs_reconstruct_checked / rs_reconstruct_checked_ptrs (the repair
// kernel): one launch regenerates the erased shards X of a stripe and checks
// its present shards U = present \ C, both from the same k survivors C, so
// every row of the pattern of X' = X + U is wanted.  The splits, survivors,
// flags and refusals are plan_checks', except that
//   - every stripe with 1 <= e <= m becomes a job, the saturated ones (still
//     counted in `saturated`) included: they have shards to regenerate;
//   - a job has exactly m entries, the ids of X' in increasing order, entry t
//     with row t; dst is the address of the shard's slot (plan_repairs_ptrs:
//     the shard's id), data shards included;
//   - an entry's pad says what becomes of its row: kRepairStore (id in X, the
//     slot is written and never read) or kRepairCompare (id in U, the slot is
//     read and never written);
//   - max_j is m whenever there is a job.
constexpr uint32_t kRepairCompare = 0u, kRepairStore = 1u;
int plan_repairs(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                 const CheckLayout& lay, CheckPlan* plan);
int plan_repairs_ptrs(int k, int n, size_t stripes, const uint8_t* erased, const uint32_t* list, size_t count,
                      CheckPlan* plan);

}  // namespace rsmi
