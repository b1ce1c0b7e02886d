// column_correct.hpp -- launch interface of the per-column correction kernel
// (rs_correct_columns; column_correct.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rsmi {

// Job b = {stripe, table, r, d} of `jobs`: an inconsistent stripe with r
// present shards and d = r - k >= 2 syndromes, whose erasure set's tables
// (column_decode.hpp column_tables) are tables[table].  Every byte column
// below shard_len of the stripe is decoded on its own: a column with non-zero
// syndromes and a codeword within d / 2 gets exactly its wrong bytes
// overwritten, and counts[b * n + id] receives the bytes changed in shard id;
// a column without one is left alone and sets fail[b].  Slots of shards that
// are not in the table's present list are never addressed.
// A block is {job, 4 KiB column chunk}; a lane owns one 16-byte column.
struct ColArgs {
    uint8_t* data;
    uint8_t* parity;
    uint64_t data_ss, parity_ss, pitch;  // strided layout, as MatArgs
    uint32_t ncols16;                    // 16-byte columns per shard
    uint32_t shard_len;
    uint32_t k, n;
    const uint4* jobs;      // [njobs] (device)
    const uint8_t* tables;  // [.][column_table_bytes(n)] (device)
    const uint8_t* gf;      // exp [512] | log [256] (device)
    uint32_t* counts;       // [njobs][n] (device), zero at launch
    uint32_t* fail;         // [njobs] (device), zero at launch
    uint32_t njobs;
    uint32_t chunks;  // filled in by plan_column_correct
    // Pointer placement: [stripe][n] device address of every shard (device, only
    // read; data / parity / strides / pitch unused), or nullptr.  The kernel's
    // pointer-mode twin loads the entries of the job's present shards only.
    const uint64_t* shard_ptrs;
    // Per-job lengths (the pointer-mode twin of rs_correct_columns_ptrs_lens
    // only; device, nullptr otherwise): job b has job_ncols[b] >= 1 16-byte
    // columns and job_lens[b] bytes and owns the blocks [first_block[b],
    // first_block[b + 1]) of the grid, ceil(job_ncols[b] / 256) of them
    // (combine_lens_map.hpp, groups = 1); ncols16, shard_len and chunks are
    // unused.  At the end: no other member's kernarg offset moves.
    const uint32_t* first_block;  // [njobs + 1]
    const uint32_t* job_ncols;    // [njobs]
    const uint32_t* job_lens;     // [njobs]
};
// Whether a code with m parity shards is served (1 <= m <= 16).
bool column_correct_supported(int m);
// Fills in the launch plan; false when the grid would exceed 2^31 - 1 blocks.
bool plan_column_correct(ColArgs* a);
hipError_t launch_column_correct(const ColArgs& a, int m, hipStream_t stream);  // a: planned
// The per-job-length twin: a.shard_ptrs and the three per-job tables set,
// `blocks` == first_block[njobs] <= 2^31 - 1 (column_lens_plan.hpp).
hipError_t launch_column_correct_lens(const ColArgs& a, int m, uint32_t blocks, hipStream_t stream);
const char* column_variant_name(int m);  // "columns_MG4_B256" etc.; "none" for a code that is not served
const char* column_ptrs_variant_name(int m);  // the pointer-mode twin: "columns_MG4_B256_ptrs" etc.
const char* column_lens_variant_name(int m);  // its per-job-length twin: "columns_MG4_B256_ptrs_lens" etc.

}  // namespace rsmi
