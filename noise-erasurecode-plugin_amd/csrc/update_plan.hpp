// update_plan.hpp -- host-side planner of rs_update_stripes (the in-place
// parity update of device-resident stripes): validates the caller's list of
// changed data shards and groups it into one job per stripe.  Pure host code:
// no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rsmi.h"

namespace rsmi {

// One stripe's updates: entries [first, first + j) of the entry table.  All
// updates of a stripe are in one job -- the kernel gives a job's parity
// columns to one block per row group, and two blocks patching the same
// column would lose one of the two XORs.
struct UpdateJob {
    uint64_t stripe;
    uint32_t first;
    uint32_t j;
};
// One changed data shard: its id and the device address of the new contents.
struct UpdateEntry {
    uint64_t src;
    uint32_t shard;
    uint32_t pad;
};
static_assert(sizeof(UpdateJob) == 16 && sizeof(UpdateEntry) == 16, "device table records");

struct UpdatePlan {
    std::vector<UpdateJob> jobs;        // ordered by stripe index
    std::vector<UpdateEntry> entries;   // a job's entries are consecutive, ordered by shard id
    uint32_t max_j = 0;                 // the largest j of any job
};

// Plans `count` updates of RS(k, .) stripes [0, stripes).  RS_OK and the plan
// (empty for count == 0), or, with the plan left empty:
//   RS_EINVAL         updates == NULL with count > 0, stripe >= stripes,
//                     reserved != 0, src NULL or not 16-byte aligned, the same
//                     (stripe, shard) listed twice, count >= 2^32
//   RS_EBAD_SHARE_ID  shard >= k
// The entries are checked in order; duplicates are looked for last.
int plan_updates(int k, size_t stripes, const rs_shard_update* updates, size_t count, UpdatePlan* plan);

}  // namespace rsmi
