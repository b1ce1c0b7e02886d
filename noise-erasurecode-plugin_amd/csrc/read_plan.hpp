// read_plan.hpp -- host-side planner of rs_read_stripes (the degraded read of
// device-resident stripes): validates the caller's list of wanted shards,
// splits it into shards to regenerate and shards to copy, and groups the
// former into one job per stripe.  Pure host code: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rsmi.h"

namespace rsmi {

// One stripe's wanted missing shards: entries [first, first + j) of the entry
// table.  Only stripes that want at least one erased shard get a job.
struct ReadJob {
    uint64_t stripe;
    uint32_t first;
    uint32_t j;
};
// One wanted missing shard: where it goes, and its rank among the stripe's
// erased ids in increasing order -- the row of the stripe's decode pattern
// that regenerates it (rs_pattern_rows).
struct ReadEntry {
    uint64_t dst;
    uint32_t row;
    uint32_t pad;
};
static_assert(sizeof(ReadJob) == 16 && sizeof(ReadEntry) == 16, "device table records");
// One wanted present shard: served by a copy (host-side record; the caller
// turns (stripe, shard) into an address).
struct ReadCopy {
    uint64_t stripe;
    uint32_t shard;
    uint32_t pad;
    uint64_t dst;
};

struct ReadPlan {
    std::vector<ReadJob> jobs;       // ordered by stripe index
    std::vector<ReadEntry> entries;  // a job's entries are consecutive, ordered by shard id (= by row)
    std::vector<ReadCopy> copies;    // ordered by (stripe, shard)
    std::vector<uint8_t> erased;     // [jobs.size()][n]: the erasure flags of the jobs' stripes, 0 / 1
    uint32_t max_j = 0;              // the largest j of any job
};

// Plans `count` reads of RS(k, n) stripes [0, stripes) with the erasure flags
// erased[stripes][n] (non-zero = missing).  Every dst receives dst_bytes bytes
// (round_up(shard_len, 16)).  RS_OK and the plan (empty for count == 0), or,
// with the plan left empty:
//   RS_EINVAL         reads or erased NULL with count > 0, stripe >= stripes,
//                     reserved != 0, dst NULL or not 16-byte aligned, the same
//                     (stripe, shard) listed twice, two dst ranges that
//                     intersect, count >= 2^32
//   RS_EBAD_SHARE_ID  shard >= n
//   RS_ENOT_ENOUGH    a listed stripe that wants an erased shard has more than
//                     n - k erasures
// The entries are checked in order, then duplicates, then the dst ranges; the
// erasure flags are looked at last, and only those of listed stripes.
int plan_reads(int k, int n, size_t stripes, const uint8_t* erased, size_t dst_bytes, const rs_shard_read* reads,
               size_t count, ReadPlan* plan);

}  // namespace rsmi
