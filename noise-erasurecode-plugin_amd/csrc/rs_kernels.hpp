// rs_kernels.hpp -- launch interface of the GF(2^8) matrix x stripe kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "combine_plan.hpp"
#include "read_plan.hpp"
#include "update_degraded_plan.hpp"
#include "update_plan.hpp"

namespace rsmi {

// One launch codes many stripes.  For stripe s the kernel reads the k
// survivor shards src[pat][0..k-1] and writes the e = cnt[pat] output shards
// dst[pat][0..e-1]:  out_t = sum_c coef[pat][t][c] * shard[src[pat][c]].
// Encode is the single pattern {src = 0..k-1, dst = k..n-1, coef = E_bottom}.
// Pattern p's outputs count lives in the stripe word (stripe_desc[b].y & 0xFF).
// Reconstruct lists stripes grouped by pattern: concurrently running blocks
// then read and write the same shard positions (measured ~6% faster than
// address order with mixed patterns).
// Shard id i < k lives in the data region, i >= k in the parity region
// (see rsmi.h, rs_encode_stripes).
struct MatArgs {
    uint8_t* data;
    uint8_t* parity;
    uint64_t data_ss;    // data stripe stride (bytes)
    uint64_t parity_ss;  // parity stripe stride (bytes)
    uint64_t pitch;      // shard pitch (bytes)
    uint64_t stripes;
    uint32_t ncols16;    // 16-byte columns per shard = ceil(shard_len / 16)
    uint32_t chunks;     // column chunks per stripe
    uint32_t groups;     // output-row groups per stripe
    uint32_t iters;      // block iterations per chunk
    uint32_t k, m;
    const uint8_t* coef;         // [npat][m][k]
    const uint32_t* src;         // [npat][k]   survivor shard ids, or nullptr: survivor j is
                                 // shard id j (single-pattern launches whose shard table or
                                 // strided layout is already in survivor order)
    const uint32_t* dst;         // [npat][dst_stride] output shard ids (padded, >= 16)
    uint32_t dst_stride;
    const uint2* stripe_desc;    // [stripes] {stripe index, pattern id << 8 | outputs}
                                 // in processing order, or nullptr: stripe b, pattern 0
                                 // with all m rows (encode)
    const uint64_t* shard_ptrs;  // [stripe][k + m] device address of every shard (pointer
                                 // mode: data/parity/strides/pitch unused), or nullptr
    uint32_t xcd;                // XCD-aware block order (xcd.hpp): blocks per region, or 0
                                 // (natural); ~0u = all of a stripe's blocks (set at launch)
    uint32_t desc0;              // stripe_desc == nullptr: every stripe's {pattern << 8 |
                                 // outputs} word (0: pattern 0 with all m rows, the encode)
    // Small reconstructs (at most kInlineDesc descriptors): the descriptors
    // ride in the kernel arguments (stripe_desc == nullptr, n_inline > 0) --
    // no upload of a descriptor array ahead of the kernel.
    static constexpr int kInlineDesc = 16;
    uint32_t n_inline;
    uint2 inl_desc[kInlineDesc];
};

// Fills in chunks/groups/iters from k, m, ncols16 and launches the kernel
// variant for (k, m).  max_e bounds cnt[] over all patterns.
hipError_t launch_matmul(MatArgs a, int max_e, hipStream_t stream);

// Mailbox grid (rs_encode / rs_decode of one small message): one launch per
// call of the split-table kernel, a group of blocks per column-chunk job,
// each group coding its job as soon as the host has staged it and bumped
// `posted` -- instead of a launch, a dispatch and a completion event per
// chunk.  Every job's arguments are known before the staging starts and go
// in the launch's kernel arguments; the host's post is one word, and job j's
// group writes done[j - 1] = j.  quit (host) makes the groups still waiting
// for their job leave.
constexpr int kMailboxJobs = 4;
struct MailboxJob {
    MatArgs a;        // chunks / groups / iters planned (plan_mailbox_job), xcd 0
    uint32_t blocks;  // logical blocks of the job
    uint32_t pad[3];
};
struct MailboxJobs {  // by value in the kernel arguments
    MailboxJob job[kMailboxJobs];
};
struct MailboxHost {  // pinned (coherent), device-mapped; read by the grid with system-scope loads
    uint64_t posted;  // host: jobs posted (staged) so far
    uint64_t quit;    // host: nonzero = groups still waiting leave
    uint64_t pad0[14];
    uint64_t done[kMailboxJobs];  // grid: done[j - 1] = j once job j is coded
    uint64_t gave_up;             // grid: nonzero once a group left without its job (timeout or quit)
    uint64_t pad1[11];
};
struct MailboxDev {  // device memory: zero between launches (the grid's last block out zeroes it)
    uint32_t left;    // blocks that have left
    uint32_t arrive[kMailboxJobs];  // blocks of job j's group finished with it
    uint32_t pad[11];
    // Diagnostics (launch_mailbox's stamps flag, RSMI_MAILBOX_STAMPS):
    // device wall clock at block 0's entry, then per job when its group's
    // first block saw it posted, had its arguments, and when the group's
    // last block stored done.
    uint64_t stamp[1 + 3 * kMailboxJobs];
};

// Whether a mailbox grid serves jobs of k survivors and up to `rows`
// outputs per stripe (the split-table variants for RS(10,4) and RS(4,2)).
bool mailbox_supported(int k, int rows);
// Fills job->a's launch plan (as launch_matmul would) and job->blocks.
void plan_mailbox_job(const MatArgs& a, int max_e, MailboxJob* job);
// Launches njobs (1..kMailboxJobs) groups of per_job blocks for jobs[0 ..
// njobs) (a group codes its job's logical blocks in turn).  A block waits at most `timeout` device
// wall-clock ticks (hipDeviceAttributeWallClockRate) for its job to be
// posted; a job whose group gave up stays undone (the caller codes it with
// an ordinary launch after the stream drained).  h is the device alias of
// the MailboxHost.
hipError_t launch_mailbox(MailboxHost* h, MailboxDev* d, const MailboxJobs& jobs, int njobs, int k, int rows,
                          uint32_t per_job, uint64_t timeout, hipStream_t stream, bool stamps = false);

// Which compiled variant serves (k, m): "K10_MG4" etc. (diagnostics).
const char* variant_name(int k, int rows);  // kernel coding up to `rows` outputs per stripe
// The blocks launch_matmul would launch for `stripes` stripes of ncols16
// columns and up to max_e outputs (a caller that must refuse a grid of more
// than 2^31 - 1 blocks before it queues anything; stripes < 2^32).
uint64_t matmul_blocks(int k, int max_e, uint32_t ncols16, uint64_t stripes);

// Verify twin of the encode launch (a: the encode pattern, all m rows of
// every stripe, optionally a stripe list {stripe index, 0 << 8 | m}): the
// kernel recomputes each stripe's parity and compares it with the stored
// parity in registers.  first_bad[stripe] (device, preset to 0xFF bytes on
// `stream` by the caller) receives by atomicMin the lowest byte offset below
// shard_len at which a stored parity shard differs; parity is only read.
hipError_t launch_verify(MatArgs a, uint32_t* first_bad, uint32_t shard_len, hipStream_t stream);
const char* verify_variant_name(int k, int rows);  // "verify_K10_MG4_B256" etc.

// In-place parity update (rs_update_stripes): job b = {stripe, first, j} of
// `jobs` overwrites data shards entries[first .. first + j) of its stripe with
// the contents at their src and patches every parity row r of the stripe,
//     parity[r] ^= enc[(k + r) * k + shard_c] * (old_c ^ new_c).
// A block is {job, 4 KiB column chunk, row group of MG parity rows}.
struct UpdArgs {
    uint8_t* data;
    uint8_t* parity;
    uint64_t data_ss, parity_ss, pitch;  // strided layout, as MatArgs
    uint32_t ncols16;                    // 16-byte columns per shard
    uint32_t k, m;
    const uint8_t* enc;          // [k + m][k] encode matrix (device)
    const UpdateJob* jobs;       // [njobs] (device), at most one per stripe
    const UpdateEntry* entries;  // (device)
    uint32_t njobs;
    uint32_t xcd;                // XCD-aware block order, as MatArgs
    // Filled in by plan_update:
    uint32_t chunks, groups, iters;
    uint32_t mg;      // row-group size of the variant chosen
    uint32_t commit;  // 1: one row group covers all m rows and the block stores the new
                      // contents over the old itself; 0 (several row groups, each reading
                      // the old data): the kernel leaves the data alone and the caller
                      // copies it in behind the kernel
};
// Chooses the variant for (a->m, max_j = the largest j of any job) and fills
// in the launch plan; false when the grid would exceed 2^31 - 1 blocks.
bool plan_update(UpdArgs* a, uint32_t max_j);
hipError_t launch_update(const UpdArgs& a, uint32_t max_j, hipStream_t stream);  // a: planned
const char* update_variant_name(int m);  // "update_MG4_B256" etc.
// Its twin for the pointer placement (rs_update_ptrs): shard i of stripe s is
// at shard_ptrs[s * (k + m) + i] (device table, only read) and the layout
// fields of `a` are unused.  The old-shard bases and the row group's parity
// bases come from the stripe's row of the table, shard_off (a multiple of 16:
// the byte offset of the call's slice within every slot) added once to each;
// entries[..].src holds the slice from its start.  Only the entries of a job's
// changed shards and of its m parity rows are loaded.  A compile-time twin of
// the update kernel: the strided instantiations keep their code.
hipError_t launch_update_ptrs(const UpdArgs& a, const uint64_t* shard_ptrs, uint64_t shard_off, uint32_t max_j,
                              hipStream_t stream);  // a: planned
const char* update_ptrs_variant_name(int m);  // "update_MG4_B256_ptrs" etc.

// In-place parity update of stripes with missing shards (rs_update_degraded):
// job b of `jobs` (update_degraded_plan.hpp) patches the present parity rows
// rows[row_first .. row_first + nrows) of its stripe,
//     parity[r] ^= sum_c enc[(k + r) * k + shard_c] * (old_c ^ new_c),
// and never dereferences the slot of an erased shard.  Two forms, per job:
//   pair form   (pat == kDegNoPattern): the sources are (old, new) pairs as in
//               the update kernel; old is the entry's slot, or entries[].old
//               where the caller regenerated it.
//   decode form (pat = the stripe's pattern in the ctx's pattern cache): the
//               sources are the pattern's k survivors and the j new buffers,
//               the old contents of the erased changed shards folded into the
//               survivors' coefficients (rs_update_degraded_kernel).  Needs
//               groups == 1: a parity survivor is a source and an output.
// A block is {job, 4 KiB column chunk, row group of MG present parity rows}.
struct DegArgs {
    uint8_t* data;
    uint8_t* parity;
    uint64_t data_ss, parity_ss, pitch;  // strided layout, as MatArgs
    uint32_t ncols16;                    // 16-byte columns per shard
    uint32_t k, m;
    const uint8_t* enc;     // [k + m][k] encode matrix, then the exp[512] and log[256] tables (device)
    const uint8_t* coef;    // [npat][m][k] (the pattern cache, as MatArgs); decode form only
    const uint32_t* src;    // [npat][k]
    const DegJob* jobs;     // [njobs] (device), at most one per stripe
    const DegEntry* entries;  // (device)
    const uint32_t* rows;     // (device)
    uint32_t njobs;
    uint32_t xcd;           // XCD-aware block order, as MatArgs
    // Filled in by plan_update_degraded_launch:
    uint32_t chunks, groups, iters;
    uint32_t mg;      // row-group size of the variant chosen
    uint32_t commit;  // 1 (one row group): the block stores the new contents of present changed
                      // shards over the old itself; 0: the caller copies them in behind the kernel
};
// Whether one row group and the LDS serve a call of this m whose widest job
// has max_src sources (UpdateDegradedPlan::max_src) -- the decode form's needs.
bool update_degraded_fused(int m, uint32_t max_src);
// Chooses the variant for a->m and fills in the launch plan.  fused: one row
// group, in-kernel commit, max_src as above; else row groups as the update
// kernel's, no commit, every job in pair form and max_src = the largest j.
// false when the grid would exceed 2^31 - 1 blocks.
bool plan_update_degraded_launch(DegArgs* a, uint32_t max_src, bool fused);
hipError_t launch_update_degraded(const DegArgs& a, uint32_t max_src, hipStream_t stream);  // a: planned
const char* update_degraded_variant_name(int m);  // "update_degraded_MG4_B256" etc.

// Caller-chosen combinations (rs_combine): job b of `jobs` (combine_plan.hpp)
// multiplies its nsrc source buffers by its nout x nsrc coefficients and
// stores the nout sums at its destinations, or XORs them in (accumulate):
//     *dst[r] (^)= sum_c coef[job.coef + r * nsrc + c] * *src[c]
// A block is {job, 4 KiB column chunk, row group of MG outputs}; a job with
// fewer row groups than the call's widest leaves its surplus blocks idle.
struct CombArgs {
    const CombineJob* jobs;  // [njobs] (device)
    const uint64_t* addrs;   // (device) a job's sources, then its destinations
    const uint8_t* coef;     // (device)
    uint32_t ncols16;        // 16-byte columns per buffer
    uint32_t njobs;
    uint32_t xcd;            // XCD-aware block order, as MatArgs
    // Filled in by plan_combine_launch:
    uint32_t chunks, groups, iters;
    uint32_t mg;  // row-group size of the variant chosen
};
// Chooses the variant for the call's largest nsrc and nout and fills in the
// launch plan; false when the grid would exceed 2^31 - 1 blocks.
bool plan_combine_launch(CombArgs* a, uint32_t max_nsrc, uint32_t max_nout);
hipError_t launch_combine(const CombArgs& a, uint32_t max_nsrc, hipStream_t stream);  // a: planned
const char* combine_variant_name(int nsrc, int nout);  // "combine_MG4_B256" etc.

// rs_combine_lens: CombArgs for jobs of their own lengths.  Job b has ncols[b]
// 16-byte columns and owns the blocks [first_block[b], first_block[b + 1]) of
// the grid (combine_lens_map.hpp); ncols16, chunks and xcd are unused (natural
// block order), iters is the most iterations any block runs.
struct CombLensArgs : CombArgs {
    const uint32_t* ncols;        // [njobs] (device)
    const uint32_t* first_block;  // [njobs + 1] (device)
};
// The iterations a block of the combine kernels may run (RSMI_ITERS, 1 unless
// set): what plan_combine_lens makes its block counts for.
uint32_t combine_iters_cap();
// Fills in the launch plan from a plan_combine_lens plan (njobs, groups, mg,
// iters); false when the plan's row groups are not those of the kernel
// variants.
bool plan_combine_lens_launch(CombLensArgs* a, const CombinePlan& plan);
// a: planned; blocks = the plan's first_block.back().
hipError_t launch_combine_lens(const CombLensArgs& a, uint32_t max_nsrc, uint32_t blocks, hipStream_t stream);
const char* combine_lens_variant_name(int nsrc, int nout);  // "combine_lens_MG4_B256" etc.

// Degraded read (rs_read_stripes): job b = {stripe, first, j} of `jobs`, whose
// stripe uses decode pattern pats[b] of the ctx's pattern cache, regenerates
// the j wanted missing shards entries[first .. first + j) from the pattern's k
// survivors (strided layout, src[pat]):
//     *entries[first + t].dst = sum_c coef[(pat * m + entries[first + t].row) * k + c] * shard[src[pat * k + c]]
// A block is {job, 4 KiB column chunk, row group of MG wanted rows}.  The
// stripes are only read; rows of the pattern that nobody wants are not coded.
struct ReadArgs {
    const uint8_t* data;
    const uint8_t* parity;
    uint64_t data_ss, parity_ss, pitch;  // strided layout, as MatArgs
    uint32_t ncols16;                    // 16-byte columns per shard
    uint32_t k, m;
    const uint8_t* coef;       // [npat][m][k] (the pattern cache, as MatArgs)
    const uint32_t* src;       // [npat][k]
    const ReadJob* jobs;       // [njobs] (device), at most one per stripe
    const ReadEntry* entries;  // (device)
    const uint32_t* pats;      // [njobs] (device) pattern id of each job's stripe
    uint32_t njobs;
    uint32_t xcd;              // XCD-aware block order, as MatArgs
    // Filled in by plan_read:
    uint32_t chunks, groups, iters;
};
// Fills in the launch plan for max_j = the largest j of any job; false when
// the grid would exceed 2^31 - 1 blocks.
bool plan_read(ReadArgs* a, uint32_t max_j);
hipError_t launch_read(const ReadArgs& a, hipStream_t stream);  // a: planned
const char* read_variant_name(int k);  // "read_K10_MG4_B256" etc.
// Its twin for the pointer placement (rs_read_ptrs), as launch_update_ptrs:
// the survivors' addresses come from the table (resolved as the check
// kernel's twin resolves them), shard_off added once to each;
// entries[..].dst stays a destination address and receives the slice from its
// start.  The table entries of erased shards are never loaded.
hipError_t launch_read_ptrs(const ReadArgs& a, const uint64_t* shard_ptrs, uint64_t shard_off,
                            hipStream_t stream);  // a: planned
const char* read_ptrs_variant_name(int k);  // "read_K10_MG4_B256_ptrs" etc.

// Degraded check (rs_verify_degraded): the verify twin of the read launch,
// with the same arguments and plan (plan_read).  Job b's entries are the
// present shards of its stripe that the pattern pats[b] does not use as
// survivors: entries[..].dst is the address of the STORED shard, .row the
// pattern row that recomputes it.  The kernel compares the two in registers
// and first_bad[stripe] (device, preset to 0xFF bytes on `stream` by the
// caller) receives by atomicMin the lowest byte offset below shard_len at
// which they differ.  Everything is only read: (k + j) * S bytes per job.
hipError_t launch_check(const ReadArgs& a, uint32_t* first_bad, uint32_t shard_len, hipStream_t stream);  // a: planned
const char* check_variant_name(int k);  // "check_K10_MG4_B256" etc.

// The degraded check of the pointer placement (rs_verify_ptrs): shard i of
// stripe s is at shard_ptrs[s * (k + m) + i] (device table, only read) and the
// layout fields of `a` are unused.  The survivors' addresses come from the
// table, and entries[..].dst holds the shard ID of the stored shard
// (plan_checks_ptrs), resolved through the table as well.  A compile-time twin
// of the check kernel: the strided instantiations keep their code.
hipError_t launch_check_ptrs(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad, uint32_t shard_len,
                             hipStream_t stream);  // a: planned
const char* check_ptrs_variant_name(int k);  // "check_K10_MG4_B256_ptrs" etc.

// Checked repair (rs_reconstruct_checked): the read and the check launch in
// one, with the same arguments and plan (plan_read, max_j = m).  Job b's
// entries are all m ids of the erasure set X' that pats[b] was built for
// (plan_repairs), entry t with row t; entries[..].dst is the address of the
// shard's slot and .pad says what happens to the row: kRepairStore -- the
// shard is erased, the regenerated row is stored there and the slot is never
// read -- or kRepairCompare -- the shard is present, the row is compared with
// it as by launch_check, and the slot is never written.  (k + j) * S bytes
// read and e * S written per job, j = m - e: n * S in all.
hipError_t launch_repair(const ReadArgs& a, uint32_t* first_bad, uint32_t shard_len, hipStream_t stream);  // a: planned
const char* repair_variant_name(int k);  // "repair_K10_MG4_B256" etc.
// Its twin for the pointer placement (rs_reconstruct_checked_ptrs), as
// launch_check_ptrs: entries[..].dst holds shard ids (plan_repairs_ptrs), and
// the table entries of the erased shards are loaded too, as destinations.
hipError_t launch_repair_ptrs(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad, uint32_t shard_len,
                              hipStream_t stream);  // a: planned
const char* repair_ptrs_variant_name(int k);  // "repair_K10_MG4_B256_ptrs" etc.

// Per-stripe lengths for the pointer-mode scrub (rs_verify_ptrs_lens,
// rs_reconstruct_checked_ptrs_lens; scrub_lens_plan.hpp): entry b of a
// launch's list -- the stripe list of the verify kernel, the jobs of the check
// and the repair kernel -- has ncols[b] >= 1 16-byte columns and lens[b] bytes
// and owns the blocks [first_block[b], first_block[b + 1]) of the grid
// (combine_lens_map.hpp), in natural block order.
struct ScrubLensTables {
    const uint32_t* first_block;  // [njobs + 1] (device)
    const uint32_t* ncols;        // [njobs] (device)
    const uint32_t* lens;         // [njobs] (device)
    uint32_t njobs;
};
// Row groups per column chunk of the verify variant that serves (k, m).
uint32_t verify_row_groups(int k, int m);
// The per-stripe-length twin of launch_verify, pointer mode only: a.stripe_desc
// lists t.njobs stripes {stripe index, 0 << 8 | m}, a.shard_ptrs is the table,
// a.iters the most iterations a block runs (the plan's), and `blocks` the
// plan's block count for verify_row_groups(k, m) row groups.
hipError_t launch_verify_lens(MatArgs a, uint32_t* first_bad, const ScrubLensTables& t, uint32_t blocks,
                              hipStream_t stream);
const char* verify_lens_variant_name(int k, int rows);  // "verify_K10_MG4_B256_lens" etc.
// The twins of launch_check_ptrs and launch_repair_ptrs: job b of a.jobs
// (a.njobs == t.njobs) takes its columns and length from t.  a.groups =
// ceil(max_j / 4) and a.iters are the plan's; a.ncols16, a.chunks and a.xcd are
// unused.
hipError_t launch_check_lens(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad,
                             const ScrubLensTables& t, uint32_t blocks, hipStream_t stream);
const char* check_lens_variant_name(int k);  // "check_K10_MG4_B256_ptrs_lens" etc.
hipError_t launch_repair_lens(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad,
                              const ScrubLensTables& t, uint32_t blocks, hipStream_t stream);
const char* repair_lens_variant_name(int k);  // "repair_K10_MG4_B256_ptrs_lens" etc.

// Column gather of the scrub's locate step: for pairs[i] = {stripe, byte
// offset} (device, offset < shard_len) out[i * n + id] = that byte of shard
// id, for every shard of the stripe (a: strided layout, k, m).
hipError_t launch_gather_columns(const MatArgs& a, const uint2* pairs, uint32_t count, uint8_t* out,
                                 hipStream_t stream);
// The same with missing shards: flags[i * n + id] (device) non-zero = shard id
// of pair i's stripe is missing; out gets 0 there and the slot is not read.
hipError_t launch_gather_columns_masked(const MatArgs& a, const uint2* pairs, const uint8_t* flags, uint32_t count,
                                        uint8_t* out, hipStream_t stream);

// Device-side copy of `count` pieces of `bytes` bytes (a multiple of 16):
// piece i copies src + pieces[2i] to dst + pieces[2i+1] (16-byte aligned
// offsets).  rs_decode_batch packs survivors / unpacks regenerated shards
// with it so PCIe carries only those.
hipError_t launch_copy_pieces(const uint8_t* src, uint8_t* dst, const uint64_t* pieces, uint32_t count,
                              size_t bytes, hipStream_t stream);

// Its twin for the pointer placement: piece i copies `bytes` bytes between
// the slot shard_ptrs[pieces[2i]] + slot_off and the address pieces[2i+1] --
// into the slot (to_slot: the commit of rs_update_ptrs) or out of it (the
// present shards of rs_read_ptrs).  Only the named table entries are loaded.
hipError_t launch_copy_table(const uint64_t* shard_ptrs, const uint64_t* pieces, uint32_t count, size_t bytes,
                             uint64_t slot_off, bool to_slot, hipStream_t stream);

// splitmix64 byte stream fill (bench/test utility).
hipError_t launch_fill_splitmix(void* dev, size_t len, uint64_t seed, hipStream_t stream);

}  // namespace rsmi
