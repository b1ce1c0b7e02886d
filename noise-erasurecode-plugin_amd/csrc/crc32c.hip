// crc32c.hip -- the sector-checksum kernel: CRC-32C (RFC 3720) of every
// sector of device-resident shards, stored or compared in registers.
//
// gfx950 has no carry-less multiply, so the CRC is taken as what it is, a
// GF(2)-linear map (crc32c_math.hpp), and cut for the memory system: a sector
// is served by a group of G lanes of one wave and lane j takes the 16-byte
// words j, j + G, j + 2G, ... straight from its coalesced loads (interleaved
// Horner):
//     acc <- acc * x^(128 G)  ^  f(word)
// -- four lookups for the constant multiply, sixteen (slice-by-16) for the
// word, all in LDS tables (20 KiB).  At the end lane j multiplies by its
// position weight x^(128 (G - 1 - j)) with a 32-step shift-and-XOR in
// registers and the group XORs its lanes together.  G = sector_len / 64 up to
// a whole wave (8 lanes for 512-byte sectors, 64 from 4 KiB), so the register
// multiply is paid once per 64 bytes or less often and a lane always has at
// least four loads in flight.
//
// A short last sector is computed as if padded with zero bytes to sector_len
// and the pad is taken off again by one multiplication with x^(-8 pad); the
// words past round_up(shard_len, 16) are not loaded and the bytes of the last
// word at or past shard_len are masked, so they never enter a checksum.
//
// A translation unit of its own, so that the streaming kernels' code objects
// stay as they are.
#include "crc32c.hpp"

#include "crc32c_math.hpp"

namespace rsmi {

namespace {

constexpr int kCrcBlock = 256;
constexpr uint32_t kCrcBlockBytes = 65536;  // a block's run of sectors (at least one sector per wave)

__device__ const CrcTables d_crc_tab = make_crc_tables();

// a * b mod P in registers (crc_mulmod, unrolled).
__device__ __forceinline__ uint32_t mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}

// XOR of table[i][byte i of v], i = 0..3, for four consecutive 256-entry tables.
__device__ __forceinline__ uint32_t lookup4(const uint32_t* t, uint32_t v) {
    return t[v & 0xFFu] ^ t[256 + ((v >> 8) & 0xFFu)] ^ t[512 + ((v >> 16) & 0xFFu)] ^ t[768 + (v >> 24)];
}

template <bool PTRS, bool CHECK>
__global__ __launch_bounds__(kCrcBlock) void rs_crc32c_kernel(CrcArgs a) {
    // s_slice[i * 256 + b] = slice[15 - i][b] serves byte i of a word (15 - i
    // bytes follow it): the slices are stored in reverse order, so that dword
    // q of a word reads its four tables from s_slice + 1024 q.
    __shared__ uint32_t s_slice[kCrcSlices * 256];
    __shared__ uint32_t s_stride[4 * 256];
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = blockIdx.x / a.blocks_per_shard, run = blockIdx.x % a.blocks_per_shard;
    const uint64_t shard = a.shards ? a.shards[slot] : slot;
    const uint32_t lg = a.lg_group;
    for (uint32_t i = tid; i < kCrcSlices * 256; i += kCrcBlock)
        s_slice[i] = d_crc_tab.slice[kCrcSlices - 1 - (i >> 8)][i & 0xFFu];
    // stride[lg - 3]: the multiply by x^(8 * 16 G), a group's stride of 16 G =
    // 128 << (lg - 3) bytes (G = 8 lanes: 128 bytes, table 0).
    for (uint32_t i = tid; i < 4 * 256; i += kCrcBlock) s_stride[i] = d_crc_tab.stride[lg - 3][i >> 8][i & 0xFFu];
    // The shard's base, once per block.
    const uint64_t stripe = shard / a.n;
    const uint32_t id = static_cast<uint32_t>(shard % a.n);
    const uint8_t* base;
    if (PTRS)
        base = reinterpret_cast<const uint8_t*>(a.shard_ptrs[shard]);
    else
        base = id < a.k ? a.data + stripe * a.data_ss + static_cast<uint64_t>(id) * a.pitch
                        : a.parity + stripe * a.parity_ss + static_cast<uint64_t>(id - a.k) * a.pitch;
    __syncthreads();

    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t G = 1u << lg, j = lane & (G - 1u), g = lane >> lg;
    const uint32_t per_wave = 64u >> lg;  // sectors a wave serves at a time
    const uint32_t weight = d_crc_tab.pos[G - 1u - j];
    const uint32_t first = run * a.sec_per_block;
    const uint64_t len = a.shard_len;
    for (uint32_t task = wave * per_wave; task < a.sec_per_block; task += 4u * per_wave) {
        if (first + task >= a.nsec) break;  // wave-uniform
        const uint32_t sec = first + task + g;
        // Lanes of a sector at or past nsec start at or past shard_len: they load nothing.
        const uint64_t sec_off = static_cast<uint64_t>(sec) * a.sector_len;
        uint32_t acc = 0;
        for (uint32_t t = 0; t < a.steps; t += 4) {
            uint4 w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint64_t off = sec_off + (static_cast<uint64_t>((t + u) << lg) + j) * 16u;
                w[u] = make_uint4(0, 0, 0, 0);
                if (off < len) {
                    w[u] = *reinterpret_cast<const uint4*>(base + off);
                    const uint64_t left = len - off;
                    if (left < 16) {  // the shard's last word: mask by byte
                        uint32_t* d = reinterpret_cast<uint32_t*>(&w[u]);
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int nb = static_cast<int>(left) - 4 * q;
                            d[q] = nb >= 4 ? d[q] : nb <= 0 ? 0u : d[q] & ((1u << (8 * nb)) - 1u);
                        }
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                acc = lookup4(s_stride, acc) ^ lookup4(s_slice, w[u].x) ^ lookup4(s_slice + 1024, w[u].y) ^
                      lookup4(s_slice + 2048, w[u].z) ^ lookup4(s_slice + 3072, w[u].w);
        }
        acc = mulmod(acc, weight);
        for (uint32_t d = 1; d < G; d <<= 1) acc ^= __shfl_xor(acc, d);
        if (j == 0 && sec < a.nsec) {
            const bool tail = sec == a.nsec - 1u;
            if (tail && a.tail_unshift != kCrcOne) acc = mulmod(acc, a.tail_unshift);
            const uint32_t crc = acc ^ (tail ? a.term_tail : a.term_full);
            uint32_t* const at = a.crcs + shard * a.crc_pitch + sec;
            if (CHECK) {
                if (*at != crc) atomicMin(a.first_bad + shard, sec);
            } else {
                *at = crc;
            }
        }
    }
}

}  // namespace

bool crc32c_sector_len_ok(size_t sector_len) {
    return sector_len >= 512 && sector_len <= 65536 && (sector_len & (sector_len - 1)) == 0;
}

bool plan_crc32c(CrcArgs* a, size_t shard_len, size_t sector_len) {
    if (!crc32c_sector_len_ok(sector_len) || shard_len == 0) return false;
    const uint64_t nsec = (shard_len + sector_len - 1) / sector_len;
    if (nsec > 0xFFFFFFFFull) return false;
    a->shard_len = shard_len;
    a->sector_len = static_cast<uint32_t>(sector_len);
    a->nsec = static_cast<uint32_t>(nsec);
    uint32_t lg = 3;  // G = sector_len / 64 lanes, 8 .. 64
    while ((64u << lg) < sector_len && lg < 6) ++lg;
    a->lg_group = lg;
    a->steps = static_cast<uint32_t>(sector_len >> (4 + lg));  // 4 up to 4 KiB, sector_len / 1024 beyond
    a->sec_per_block = sector_len >= kCrcBlockBytes / 4 ? 4u : kCrcBlockBytes / static_cast<uint32_t>(sector_len);
    a->blocks_per_shard = (a->nsec + a->sec_per_block - 1) / a->sec_per_block;
    const uint64_t tail = shard_len - (nsec - 1) * sector_len;
    a->tail_unshift = crc_xinv8(sector_len - tail);
    a->term_full = crc_init_term(sector_len);
    a->term_tail = crc_init_term(tail);
    return a->nshards * a->blocks_per_shard <= 0x7FFFFFFFull;
}

hipError_t launch_crc32c(const CrcArgs& a, bool check, hipStream_t stream) {
    if (a.nshards == 0) return hipSuccess;
    const dim3 grid(static_cast<uint32_t>(a.nshards * a.blocks_per_shard)), block(kCrcBlock);
    if (a.shard_ptrs) {
        if (check)
            hipLaunchKernelGGL((rs_crc32c_kernel<true, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((rs_crc32c_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (check)
            hipLaunchKernelGGL((rs_crc32c_kernel<false, true>), grid, block, 0, stream, a);
        else
            hipLaunchKernelGGL((rs_crc32c_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

const char* crc32c_variant_name() { return "crc32c_H16_B256"; }
const char* crc32c_ptrs_variant_name() { return "crc32c_H16_B256_ptrs"; }

}  // namespace rsmi
