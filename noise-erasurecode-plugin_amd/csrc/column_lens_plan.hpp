// column_lens_plan.hpp -- host-side planner of rs_correct_columns_ptrs_lens:
// the column scrub of the pointer placement for stripes that each have a shard
// length of their own.  plan_column_lens validates the call before anything is
// launched (lengths, erasure counts, the worst-case grid of the column launch)
// and lists the stripes that have bytes; plan_column_lens_jobs turns the first
// verify's verdicts into the column launch -- the jobs, their erasure sets, the
// per-job column counts, lengths and block map (combine_lens_map.hpp, one row
// group) -- and into the lengths of the second verify, which covers the jobs'
// stripes only.  Pure host code: no HIP, no context.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rsmi.h"
#include "combine_lens_map.hpp"

namespace rsmi {

constexpr uint64_t kColumnLensMaxBlocks = 0x7FFFFFFFull;  // of the column launch
constexpr int kColumnLensMaxParity = 16;                  // the kernel keeps at most 16 syndromes per column
constexpr uint32_t kColumnLensClean = 0xFFFFFFFFu;        // RS_VERIFY_CLEAN

// Blocks of the column kernel for a stripe of `ncols` 16-byte columns: one per
// 4 KiB chunk (combine_lens_chunks with one iteration).
inline uint32_t column_lens_blocks(uint32_t ncols) { return combine_lens_chunks(ncols, 1); }

struct ColumnLensPlan {
    std::vector<uint32_t> live;  // the stripes that have bytes, ascending
    uint64_t worst_blocks = 0;   // the column launch if every live stripe were dirty
    uint32_t len_all = 0;        // the one length of every stripe of the call (all live), or 0
    bool degraded = false;       // some flag of some stripe is set
};

// Validates rs_correct_columns_ptrs_lens over RS(k, n) stripes [0, stripes)
// with the erasure flags erased[stripes][n] (non-zero = missing; NULL: nothing
// is missing) and the shard lengths lens[stripes].  RS_OK and the plan, or,
// with the plan left empty:
//   RS_EINVAL       plan or lens NULL (stripes > 0), k < 1, n < k, n > 256,
//                   n - k > 16, stripes >= 2^32, a length of 2^28 or more
//                   16-byte columns, worst_blocks above 2^31 - 1 (checked up
//                   front: the refusal does not depend on the verdicts)
//   RS_ENOT_ENOUGH  a stripe -- with or without bytes -- has more than n - k
//                   erasures
// Lengths are judged before flags, flags before the block bound.
int plan_column_lens(int k, int n, size_t stripes, const uint8_t* erased, const size_t* lens, ColumnLensPlan* plan);

// A job of the column kernel, laid out as the uint4 the kernel loads
// (column_correct.hpp): stripe, index of its erasure set's tables, r present
// shards, d = r - k >= 2 syndromes.
struct ColumnLensJob {
    uint32_t stripe, table, r, d;
};

struct ColumnLensJobs {
    std::vector<ColumnLensJob> jobs;         // the dirty stripes that have a radius, ascending
    std::vector<uint32_t> hopeless;          // the dirty stripes with r - k < 2: failed, never written
    std::vector<std::vector<uint8_t>> sets;  // sets[t]: n flags (0 / 1) of erasure set t, in order of first use
    std::vector<uint32_t> ncols;             // [jobs] 16-byte columns, >= 1
    std::vector<uint32_t> lens;              // [jobs] bytes
    std::vector<uint32_t> first_block;       // [jobs + 1]; empty without jobs
    std::vector<size_t> masked;              // [stripes] lens[s] for a job's stripe, 0 for every other
    uint32_t blocks() const { return first_block.empty() ? 0u : first_block.back(); }
};

// From a plan_column_lens plan of the same call and the verdicts of the verify
// over all stripes (first_bad[stripes]; kColumnLensClean = consistent): the
// column launch and the second verify's lengths.  A stripe outside plan.live
// is never a job, whatever its verdict says.
void plan_column_lens_jobs(int k, int n, size_t stripes, const uint8_t* erased, const size_t* lens,
                           const ColumnLensPlan& plan, const uint32_t* first_bad, ColumnLensJobs* out);

}  // namespace rsmi
