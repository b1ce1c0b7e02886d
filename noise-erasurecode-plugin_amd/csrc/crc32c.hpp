// crc32c.hpp -- launch interface of the sector-checksum kernel (rs_crc32c_*,
// rs_correct_crc32c; crc32c.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rsmi {

// CRC-32C of every sector of `nshards` shards.  Shard index x = s * n + i is
// shard i of stripe s; a block serves {shard, run of sectors}, the shard being
// shards[b] (device list, e.g. the present shards of a call with erasures) or
// b itself when shards is nullptr.  Sector j of shard x covers the bytes
// [j * sector_len, min((j + 1) * sector_len, shard_len)) and its checksum is
// crcs[x * crc_pitch + j]: stored (compute), or compared with the computed one
// (check), a mismatch doing atomicMin(&first_bad[x], j).  Only
// round_up(shard_len, 16) bytes of a listed shard are loaded, bytes at or past
// shard_len never enter a checksum, and nothing else is written.
struct CrcArgs {
    const uint8_t* data;
    const uint8_t* parity;
    uint64_t data_ss, parity_ss, pitch;  // strided layout, as MatArgs
    const uint64_t* shard_ptrs;          // pointer placement: [stripe][n] device addresses, else nullptr
    const uint32_t* shards;              // [nshards] shard indices (device), or nullptr: 0 .. nshards - 1
    uint64_t nshards;
    uint32_t k, n;
    uint64_t shard_len;
    uint32_t* crcs;       // only read by a check
    uint64_t crc_pitch;
    uint32_t* first_bad;  // check only: [stripes * n], RS_VERIFY_CLEAN at launch
    // The plan (plan_crc32c).  A sector is served by a group of 2^lg_group
    // lanes, lane j taking the 16-byte words j, j + 2^lg_group, ...: `steps` of
    // them.
    uint32_t sector_len;
    uint32_t lg_group, steps;
    uint32_t nsec;               // sectors per shard
    uint32_t sec_per_block;      // a block's run of sectors
    uint32_t blocks_per_shard;
    uint32_t tail_unshift;       // x^(-8 * pad) of the last sector's pad up to sector_len (1: none)
    uint32_t term_full, term_tail;  // initial-value and final-XOR terms of a full and of the last sector
};

bool crc32c_sector_len_ok(size_t sector_len);  // a power of two in [512, 65536]
// Fills in the plan for shards of shard_len > 0 bytes; false when the grid
// would exceed 2^31 - 1 blocks.  a.nshards is set.
bool plan_crc32c(CrcArgs* a, size_t shard_len, size_t sector_len);
hipError_t launch_crc32c(const CrcArgs& a, bool check, hipStream_t stream);  // a: planned
const char* crc32c_variant_name();       // "crc32c_H16_B256"
const char* crc32c_ptrs_variant_name();  // "crc32c_H16_B256_ptrs"

}  // namespace rsmi
