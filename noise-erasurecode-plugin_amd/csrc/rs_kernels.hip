// rs_kernels.hip -- CDNA4 (gfx950) kernels for GF(2^8) coding-matrix x
// shard-stripe products: the parity loop of infectious (*FEC).Encode
// (reference call site main.go:262) and the inverted-submatrix loop of
// (*FEC).Rebuild (reference call site main.go:77), batched over stripes.
//
// Arithmetic (no MFMA: GF(2^8) is not an FP contraction):
//   split-table GF(2^8) multiply (gf_device.hpp): three v_perm_b32 lookups
//   per coefficient on four packed bytes at once.
//   The five table dwords per coefficient are built per block from the raw
//   coefficient bytes and staged in LDS; a lane reads a coefficient's tables
//   with broadcast ds_read_b128 and XOR-accumulates in VGPRs (v_bitop3_b32).
// Memory: each lane owns one 16-byte column of every survivor shard
// (global_load_dwordx4, fully coalesced: 64 lanes = 1 KiB contiguous per
// shard); outputs are written once with global_store_dwordx4.
#include "rs_kernels.hpp"

#include "gf_device.hpp"
#include "xcd.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace rsmi {
namespace {

constexpr int kBlock = 256;

using gfd::build_tables;
using gfd::gf_mac;
using gfd::xor3;

// Compiler fence for memory operations: keeps LDS table reads where they are
// written (LICM would otherwise hoist all k*MG*5 table dwords into VGPRs).
#define RS_MEM_FENCE() asm volatile("" ::: "memory")

constexpr int kRowsPerStep = 4;               // output rows per table sub-step
constexpr int kStepWords = kRowsPerStep * 5;  // table dwords per sub-step (5 x b128)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const u32x4 GlobalCU4;
typedef __attribute__((address_space(1))) u32x4 GlobalU4;

// Global (not flat) 16-byte load/store: flat ops would count on lgkmcnt too
// and serialise against the LDS table reads.  NT sets the non-temporal cache
// policy bit: every shard byte is touched exactly once per launch, and on
// MI355X nt loads + nt stores raise the 10-read/4-write movement ceiling from
// 5.84 to 6.26 TB/s (profiles/r01_membench_cachepolicy.log).
template <bool NT>
__device__ __forceinline__ uint4 gload16(const uint8_t* p) {
    u32x4 v;
    if constexpr (NT) v = __builtin_nontemporal_load((GlobalCU4*)(p));
    else v = *(GlobalCU4*)(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <bool NT>
__device__ __forceinline__ void gstore16(uint8_t* p, uint4 v) {
    u32x4 w = {v.x, v.y, v.z, v.w};
    if constexpr (NT) __builtin_nontemporal_store(w, (GlobalU4*)(p));
    else *(GlobalU4*)(p) = w;
}

// Wave-uniform 64-bit value into SGPRs.
__device__ __forceinline__ uint8_t* uniform_ptr(uint8_t* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return reinterpret_cast<uint8_t*>((static_cast<uint64_t>(hi) << 32) | lo);
}

__device__ __forceinline__ void load_step(const uint4* src, uint32_t (&T)[kStepWords]) {
#pragma unroll
    for (int w = 0; w < kStepWords / 4; ++w) {
        const uint4 v = src[w];
        T[4 * w + 0] = v.x;
        T[4 * w + 1] = v.y;
        T[4 * w + 2] = v.z;
        T[4 * w + 3] = v.w;
    }
}

// acc[r][w] ^= coef(row r) * x.w for the first R rows of one sub-step (R < 4
// only in the last sub-step of a row group that is not a multiple of 4).
template <int R = kRowsPerStep>
__device__ __forceinline__ void mac_step(uint32_t (&acc)[kRowsPerStep][4], const uint4& x,
                                         const uint32_t (&T)[kStepWords]) {
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t ia = xw[w] & 0x07070707u;
        const uint32_t ib = (xw[w] >> 3) & 0x07070707u;
        const uint32_t ic = (xw[w] >> 6) & 0x03030303u;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][w] = gf_mac(acc[r][w], &T[r * 5], ia, ib, ic);
    }
}

// mac_step for the first `rows` (1..4, wave-uniform) rows: one branch per
// row past the first, around all four words.
__device__ __forceinline__ void mac_step_rows(uint32_t (&acc)[kRowsPerStep][4], const uint4& x,
                                              const uint32_t (&T)[kStepWords], int rows) {
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
    uint32_t ia[4], ib[4], ic[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        ia[w] = xw[w] & 0x07070707u;
        ib[w] = (xw[w] >> 3) & 0x07070707u;
        ic[w] = (xw[w] >> 6) & 0x03030303u;
    }
#pragma unroll
    for (int r = 0; r < kRowsPerStep; ++r) {
        if (r > 0 && r >= rows) break;
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[r][w] = gf_mac(acc[r][w], &T[r * 5], ia[w], ib[w], ic[w]);
    }
}

// Step boundary: the accumulators of the finished sub-step are inputs of the
// asm, so its arithmetic completes before the boundary, and the memory
// clobber keeps the next sub-step's LDS reads after it.  At most two
// sub-steps of tables (2 x 20 dwords) are live at any time.
__device__ __forceinline__ void step_fence(uint32_t (&acc)[kRowsPerStep][4]) {
#pragma unroll
    for (int r = 0; r < kRowsPerStep; ++r)
        asm volatile("" : "+v"(acc[r][0]), "+v"(acc[r][1]), "+v"(acc[r][2]), "+v"(acc[r][3])::"memory");
}

// One block codes a chunk of 16-byte columns of one stripe for one group of
// MG output rows: logical block `blk` of `nblk` (rs_matmul_kernel: blockIdx.x
// of the grid; rs_resident_kernel: each job's blocks in turn).  LDS: [k][MG/4][20]
// table dwords | k survivor pointers.
//
// VF (verify twin, rs_verify_kernel): the block reads the stored 16-byte
// columns of its output rows instead of writing them.  They are requested
// next to the survivor loads and become the accumulators' initial value, so
// after the MACs an accumulator holds stored ^ recomputed and any set bit is
// a mismatch; nothing is stored but one atomicMin per wave that saw one.
//
// VARLEN (rs_verify_ptrs_lens, verify twin in pointer mode only): entry sv of
// the stripe list has its own column count and shard length.  The block finds
// sv by the search of lm->first_block[] that only `blk` feeds
// (combine_lens_map.hpp: scalar loads, uniform across the block), in natural
// block order, and takes every column bound -- the last column, the tail-lane
// clamp, the end of the iterations, the chunk stride, the bytes that count --
// from that entry.  a.iters is the most iterations any block runs; a.ncols16,
// a.chunks and a.xcd are unused.  The equal-length instances take none of this.
template <int K, int MG, int BT, bool NT, bool VF = false, bool VARLEN = false>
__device__ __forceinline__ void matmul_block(const MatArgs& a, uint32_t blk, uint32_t nblk, uint4* lds4,
                                             uint32_t* first_bad = nullptr, uint32_t shard_len = 0,
                                             const ScrubLensTables* lm = nullptr) {
    static_assert(!VARLEN || VF, "per-stripe lengths: the verify twin only");
    static_assert(MG % 2 == 0, "MG must be even");
    constexpr int TG = (MG + kRowsPerStep - 1) / kRowsPerStep;  // sub-steps per survivor
    constexpr int RL = MG - (TG - 1) * kRowsPerStep;            // rows in the last sub-step
    constexpr bool kRegPtrs = K > 0 && K <= 16;           // survivor bases kept in SGPRs
    // A single 4-row group (the RS(10,4), RS(4,2), RS(8,14) reconstructs)
    // codes only the stripe's e rows: one MG = 4 launch serves stripes of
    // 1..4 erasures, and coding all 4 rows for each cost 1.6x the VALU of the
    // 1..4 mix (e = 2.5 on average).
#ifdef RSMI_NO_DYNROWS  // A/B builds only
    constexpr bool kDynRows = false;
#else
    constexpr bool kDynRows = TG == 1 && RL == kRowsPerStep && kRegPtrs;
#endif
    constexpr int JB = (K == 0) ? 8 : (K <= 16 ? K : 8);  // survivor loads in flight
    const int k = K ? K : static_cast<int>(a.k);
    uint32_t* tw = reinterpret_cast<uint32_t*>(lds4);
    uint8_t** sptr = reinterpret_cast<uint8_t**>(tw + k * MG * 5);

    // VARLEN: the block's place and its stripe's bounds, from the block map.
    [[maybe_unused]] uint32_t v_grp = 0, v_chunk = 0, v_chunks = 0, v_ncols = 0, v_sv = 0;
    if constexpr (VARLEN) {
        const CombineBlock at = combine_lens_block(lm->first_block, lm->njobs, a.groups, blk);
        v_sv = __builtin_amdgcn_readfirstlane(at.job);
        v_grp = __builtin_amdgcn_readfirstlane(at.grp);
        v_chunk = __builtin_amdgcn_readfirstlane(at.chunk);
        v_chunks = __builtin_amdgcn_readfirstlane(at.chunks);
        v_ncols = __builtin_amdgcn_readfirstlane(lm->ncols[v_sv]);
        shard_len = __builtin_amdgcn_readfirstlane(lm->lens[v_sv]);
    }
    // XCD-aware order (xcd.hpp): regions of a.xcd blocks per XCD in turn.
    uint64_t b = a.xcd ? xcd_block(blk, a.xcd, nblk) : blk;
    const uint32_t grp = VARLEN ? v_grp : static_cast<uint32_t>(b % a.groups);
    b /= a.groups;
    const uint32_t chunk = VARLEN ? v_chunk : static_cast<uint32_t>(b % a.chunks);
    const uint64_t sv = VARLEN ? v_sv : b / a.chunks;
    // The equal-length instances read both from the arguments where they did.
    const uint32_t& chunks = VARLEN ? v_chunks : a.chunks;
    const uint32_t& ncols16 = VARLEN ? v_ncols : a.ncols16;
    // Stripe descriptor = {stripe, pattern id << 8 | outputs} (one dependent
    // load); without a table it is stripe sv with a.desc0 (encode: pattern 0,
    // all m parity rows) -- a single-message decode then starts its pattern
    // and survivor reads without a dependent read of host memory first.
    uint2 desc = make_uint2(static_cast<uint32_t>(sv), a.desc0 ? a.desc0 : a.m);
    if (a.stripe_desc) desc = a.stripe_desc[sv];
    else if (a.n_inline) desc = a.inl_desc[sv];
    const uint64_t s = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(desc.x));
    const uint32_t sw = __builtin_amdgcn_readfirstlane(desc.y);
    const uint32_t pat = sw >> 8;
    const int e = static_cast<int>(sw & 0xFFu);
    const int row0 = static_cast<int>(grp) * MG;
    if (row0 >= e) return;  // whole block: uniform
    const int eg = min(MG, e - row0);

    // This lane's coefficient byte for the table build is requested first, so
    // waiting for it later does not wait for the survivor loads behind it.
    const uint8_t* coef = a.coef + (static_cast<size_t>(pat) * a.m + row0) * k;
    uint32_t cbyte[(K > 0 && K * MG <= BT) ? 1 : 1];
    const bool one_coef = (K > 0 && K * MG <= BT);
    if (one_coef) {
        const int j = threadIdx.x / MG, t = threadIdx.x - j * MG;
        cbyte[0] = (static_cast<int>(threadIdx.x) < k * MG && t < eg) ? coef[t * k + j] : 0u;
    }

    auto shard = [&](uint32_t id) -> uint8_t* {
        if (a.shard_ptrs) return reinterpret_cast<uint8_t*>(a.shard_ptrs[s * (a.k + a.m) + id]);
        return id < a.k ? a.data + s * a.data_ss + static_cast<uint64_t>(id) * a.pitch
                        : a.parity + s * a.parity_ss + static_cast<uint64_t>(id - a.k) * a.pitch;
    };
    // a.src == nullptr: survivor j is shard id j (no id read before the
    // survivor loads).
    const uint32_t* srcid = a.src ? a.src + static_cast<size_t>(pat) * k : nullptr;
    const uint32_t* dstid = a.dst + static_cast<size_t>(pat) * a.dst_stride + row0;
    uint8_t* sp[kRegPtrs ? K : 1];
    if constexpr (kRegPtrs) {
        // All K survivor ids in one batch of scalar loads, then all K
        // addresses (pointer mode: one more batch): the mode branches sit
        // outside the loops.  Round 4 resolved the survivors one at a time
        // (id load, wait, mode branch, address load, wait): K dependent
        // scalar round trips before the first survivor load.
        uint32_t ids[K];
#pragma unroll
        for (int j = 0; j < K; ++j) ids[j] = static_cast<uint32_t>(j);
        if (srcid) {
#pragma unroll
            for (int j = 0; j < K; ++j) ids[j] = __builtin_amdgcn_readfirstlane(srcid[j]);
        }
        if (a.shard_ptrs) {
            const uint64_t* tp = a.shard_ptrs + s * (a.k + a.m);
#pragma unroll
            for (int j = 0; j < K; ++j) sp[j] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[ids[j]]));
        } else {
            uint8_t* dbase = a.data + s * a.data_ss;
            uint8_t* pbase = a.parity + s * a.parity_ss;
#pragma unroll
            for (int j = 0; j < K; ++j)
                sp[j] = ids[j] < static_cast<uint32_t>(K) ? dbase + static_cast<uint64_t>(ids[j]) * a.pitch
                                                         : pbase + static_cast<uint64_t>(ids[j] - K) * a.pitch;
        }
    } else {
        for (int i = threadIdx.x; i < k; i += BT) sptr[i] = shard(srcid ? srcid[i] : static_cast<uint32_t>(i));
    }
    const uint32_t last = ncols16 - 1;
    // Survivor loads of the block's first iteration are issued before the
    // table build, so the prologue (pattern lookup, tables, barrier) overlaps
    // their HBM latency; with one iteration per block (the default) this is
    // the whole data path.
    uint4 xpre[kRegPtrs ? K : 1];
    // Iteration it of block `chunk` codes column chunk (it * chunks + chunk):
    // blocks running together stay on adjacent 4 KiB pieces of the same
    // shards (DRAM row locality) whatever the iteration count.
    const uint32_t cstride = chunks * BT;
    const uint32_t col0 = chunk * BT + threadIdx.x;
    const uint32_t off0 = (col0 <= last ? col0 : last) * 16u;
    if constexpr (kRegPtrs) {
#pragma unroll
        for (int j = 0; j < K; ++j) xpre[j] = gload16<NT>(sp[j] + off0);
    }
    // Output pointers are only needed at store time.  Rows are padded to 16
    // ids, so whole 4-id groups load unconditionally (s_load_dwordx4); rows
    // past eg point at a valid shard and are never stored.
    uint8_t* dp[TG * 4];
    {
        uint32_t oid[TG * 4];
#pragma unroll
        for (int g = 0; g < TG; ++g) {
            const uint4 ids = *reinterpret_cast<const uint4*>(dstid + 4 * g);
            oid[4 * g + 0] = __builtin_amdgcn_readfirstlane(ids.x);
            oid[4 * g + 1] = __builtin_amdgcn_readfirstlane(ids.y);
            oid[4 * g + 2] = __builtin_amdgcn_readfirstlane(ids.z);
            oid[4 * g + 3] = __builtin_amdgcn_readfirstlane(ids.w);
        }
        if (a.shard_ptrs) {
            const uint64_t* tp = a.shard_ptrs + s * (a.k + a.m);
#pragma unroll
            for (int r = 0; r < TG * 4; ++r) dp[r] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[oid[r]]));
        } else {
            uint8_t* dbase = a.data + s * a.data_ss;
            uint8_t* pbase = a.parity + s * a.parity_ss;
#pragma unroll
            for (int r = 0; r < TG * 4; ++r)
                dp[r] = oid[r] < a.k ? dbase + static_cast<uint64_t>(oid[r]) * a.pitch
                                     : pbase + static_cast<uint64_t>(oid[r] - a.k) * a.pitch;
        }
    }
    uint32_t acc[TG][kRowsPerStep][4];
    // Verify: the accumulators start as the stored columns, loaded next to
    // the survivors so they ride the same latency.  Rows past eg are not
    // read and stay zero (their tables are zero too, so they never report).
    auto load_stored = [&](uint32_t at) {
#pragma unroll
        for (int g = 0; g < TG; ++g)
#pragma unroll
            for (int r = 0; r < kRowsPerStep; ++r) {
                uint4 p = make_uint4(0u, 0u, 0u, 0u);
                if (g * kRowsPerStep + r < eg) p = gload16<NT>(dp[g * kRowsPerStep + r] + at);
                acc[g][r][0] = p.x;
                acc[g][r][1] = p.y;
                acc[g][r][2] = p.z;
                acc[g][r][3] = p.w;
            }
    };
    if constexpr (VF) load_stored(off0);
    // Split tables of rows [row0, row0 + MG): sub-step (j, g) holds rows
    // 4g..4g+3 as 4 x 5 dwords.
    if (one_coef) {
        if (static_cast<int>(threadIdx.x) < k * MG) {
            const int j = threadIdx.x / MG, t = threadIdx.x - j * MG;
            build_tables(cbyte[0], &tw[(j * TG + t / kRowsPerStep) * kStepWords + (t % kRowsPerStep) * 5]);
        }
    } else {
        for (int idx = threadIdx.x; idx < k * MG; idx += BT) {
            const int j = idx / MG, t = idx - j * MG;
            const uint32_t c = (t < eg) ? coef[t * k + j] : 0u;
            build_tables(c, &tw[(j * TG + t / kRowsPerStep) * kStepWords + (t % kRowsPerStep) * 5]);
        }
    }
    __syncthreads();

    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint32_t colbase = chunk * BT + it * cstride;
        if (colbase >= ncols16) break;
        RS_MEM_FENCE();
        const uint32_t col = colbase + threadIdx.x;
        const bool ok = col <= last;
        // Tail lanes re-read the last column (always in bounds) and skip the store.
        const uint32_t off = (ok ? col : last) * 16u;
        if constexpr (!VF) {
#pragma unroll
            for (int g = 0; g < TG; ++g)
#pragma unroll
                for (int r = 0; r < kRowsPerStep; ++r)
#pragma unroll
                    for (int w = 0; w < 4; ++w) acc[g][r][w] = 0u;
        }
        // Row groups of 4 beyond the pattern's outputs are skipped (uniform).
        const int tg_used = (eg + kRowsPerStep - 1) / kRowsPerStep;

        for (int jb = 0; jb < k; jb += JB) {
            uint4 xb[kRegPtrs ? 1 : JB];
            uint4* x = kRegPtrs ? xpre : xb;
            if constexpr (!kRegPtrs) {
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (K == 0 && jb + q >= k) break;
                    x[q] = gload16<NT>(uniform_ptr(sptr[jb + q]) + off);
                }
            }
            uint32_t TA[kStepWords], TB[kStepWords];
            load_step(lds4 + static_cast<size_t>(jb * TG) * (kStepWords / 4), TA);
#pragma unroll
            for (int q = 0; q < JB; ++q) {
                if (K == 0 && jb + q >= k) break;
#pragma unroll
                for (int g = 0; g < TG; ++g) {
                    // Sub-step (jb+q, g): prefetch the next one's tables, then
                    // multiply with the current ones (TA/TB alternate; the
                    // unrolled loop turns the copy into register renaming).
                    const int step = (jb + q) * TG + g;
                    const bool more = (g + 1 < TG) || (q + 1 < JB && (K != 0 || jb + q + 1 < k));
                    if (more) load_step(lds4 + static_cast<size_t>(step + 1) * (kStepWords / 4), TB);
                    if constexpr (kDynRows) {
                        mac_step_rows(acc[g], x[q], TA, eg);
                    } else if (TG == 1 || g < tg_used) {
                        if (g == TG - 1) mac_step<RL>(acc[g], x[q], TA);
                        else mac_step(acc[g], x[q], TA);
                    }
                    step_fence(acc[g]);
#pragma unroll
                    for (int w = 0; w < kStepWords; ++w) TA[w] = TB[w];
                }
            }
        }
        if constexpr (kRegPtrs) {
            // Software pipelining: the next iteration's survivor loads go out
            // before this iteration's stores.
            const uint32_t ncol = colbase + cstride + threadIdx.x;
            if (it + 1 < a.iters && colbase + cstride < ncols16) {
                const uint32_t noff = (ncol <= last ? ncol : last) * 16u;
#pragma unroll
                for (int j = 0; j < K; ++j) xpre[j] = gload16<NT>(sp[j] + noff);
            }
        }
        if constexpr (VF) {
            // Bytes at which any row's stored column differs from the
            // recomputed one; tail lanes and bytes past shard_len do not count.
            uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int g = 0; g < TG; ++g)
#pragma unroll
                for (int r = 0; r < kRowsPerStep; ++r)
#pragma unroll
                    for (int w = 0; w < 4; ++w) d[w] |= acc[g][r][w];
            const uint32_t nb = ok ? min(16u, shard_len - col * 16u) : 0u;  // bytes of this column below shard_len
            uint32_t byte = 16u;
#pragma unroll
            for (int w = 3; w >= 0; --w) {
                const uint32_t nbw = nb > 4u * w ? min(4u, nb - 4u * w) : 0u;
                const uint32_t dw = d[w] & (nbw >= 4u ? ~0u : (1u << (8u * nbw)) - 1u);
                if (dw) byte = 4u * w + (static_cast<uint32_t>(__builtin_ctz(dw)) >> 3);
            }
            // Lanes are in column order: the first mismatching lane holds the
            // wave's lowest offset.
            const bool bad = byte < 16u;
            const uint64_t bal = __ballot(bad);
            if (bad && (bal & ((1ull << __lane_id()) - 1ull)) == 0) atomicMin(&first_bad[s], col * 16u + byte);
            if (it + 1 < a.iters && colbase + cstride < ncols16) {
                const uint32_t ncol = colbase + cstride + threadIdx.x;
                load_stored((ncol <= last ? ncol : last) * 16u);
            }
        } else {
#pragma unroll
            for (int g = 0; g < TG; ++g)
#pragma unroll
                for (int r = 0; r < kRowsPerStep; ++r) {
                    const int t = g * kRowsPerStep + r;
                    if (t >= eg) break;
                    if (ok) gstore16<NT>(dp[t] + off, make_uint4(acc[g][r][0], acc[g][r][1], acc[g][r][2], acc[g][r][3]));
                }
        }
    }
}

// Verify twin of rs_matmul_kernel: first_bad[stripe] = min(first_bad[stripe],
// lowest mismatching byte offset below shard_len); the caller presets
// first_bad to 0xFF bytes on the same stream.
template <int K, int MG, int BT, bool NT>
__global__ __launch_bounds__(BT) void rs_verify_kernel(MatArgs a, uint32_t* first_bad, uint32_t shard_len) {
    extern __shared__ uint4 lds4[];
    matmul_block<K, MG, BT, NT, true>(a, blockIdx.x, gridDim.x, lds4, first_bad, shard_len);
}

// Its per-stripe-length twin (rs_verify_ptrs_lens; matmul_block<.., VARLEN>):
// a.stripe_desc lists the stripes, lm carries their lengths and the block map.
template <int K, int MG, int BT, bool NT>
__global__ __launch_bounds__(BT) void rs_verify_lens_kernel(MatArgs a, uint32_t* first_bad, ScrubLensTables lm) {
    extern __shared__ uint4 lds4[];
    matmul_block<K, MG, BT, NT, true, true>(a, blockIdx.x, gridDim.x, lds4, first_bad, 0u, &lm);
}

// Scrub's locate step: wave i copies the n bytes of stripe pairs[i].x at byte
// offset pairs[i].y, one per shard in id order, to out[i * n .. i * n + n).
__global__ __launch_bounds__(64) void gather_columns_kernel(const uint8_t* data, const uint8_t* parity,
                                                            uint64_t data_ss, uint64_t parity_ss, uint64_t pitch,
                                                            uint32_t k, uint32_t n, const uint2* pairs, uint8_t* out) {
    const uint2 p = pairs[blockIdx.x];
    for (uint32_t id = threadIdx.x; id < n; id += 64u) {
        const uint8_t* shard = id < k ? data + p.x * data_ss + static_cast<uint64_t>(id) * pitch
                                      : parity + p.x * parity_ss + static_cast<uint64_t>(id - k) * pitch;
        out[static_cast<size_t>(blockIdx.x) * n + id] = shard[p.y];
    }
}

// The gather of the degraded scrub: pair i also has n flags, flags[i * n + id]
// non-zero = shard id is missing.  Its byte is written as 0 and no address
// into its slot is formed (scrub_locate ignores those positions).
__global__ __launch_bounds__(64) void gather_columns_masked_kernel(const uint8_t* data, const uint8_t* parity,
                                                                   uint64_t data_ss, uint64_t parity_ss,
                                                                   uint64_t pitch, uint32_t k, uint32_t n,
                                                                   const uint2* pairs, const uint8_t* flags,
                                                                   uint8_t* out) {
    const uint2 p = pairs[blockIdx.x];
    for (uint32_t id = threadIdx.x; id < n; id += 64u) {
        uint8_t v = 0;
        if (!flags[static_cast<size_t>(blockIdx.x) * n + id]) {
            const uint8_t* shard = id < k ? data + p.x * data_ss + static_cast<uint64_t>(id) * pitch
                                          : parity + p.x * parity_ss + static_cast<uint64_t>(id - k) * pitch;
            v = shard[p.y];
        }
        out[static_cast<size_t>(blockIdx.x) * n + id] = v;
    }
}

// In-place parity update (rs_kernels.hpp UpdArgs): matmul_block's block
// decomposition with the job's j changed shards as the runtime "k".  The
// accumulators start as the stored parity columns (as in the verify twin),
// the inputs are old ^ new, the coefficients single columns of the encode
// matrix, and the accumulators go back to the addresses they came from.
// LDS: [j][MG/4][20] table dwords | j old-shard pointers | j new-shard pointers.
//
// PTRS (compile-time twin, launch_update_ptrs): shard id of stripe s is at
// a.shard_ptrs[s * n + id] and the layout fields of `a` are unused.  The block
// loads the table entries of its job's changed shards -- their ids first, then
// their addresses, as the check kernel's oid[] / dp[] -- and of its group's eg
// parity rows, and no other entry of the table.  a.shard_off, the byte offset
// of the call's slice within every slot, is added once to each resolved base;
// a src holds the slice from its start.
struct UpdPtrArgs : UpdArgs {
    const uint64_t* shard_ptrs;
    uint64_t shard_off;
};
template <int MG, int BT, bool NT, bool PTRS = false>
__global__ __launch_bounds__(BT) void rs_update_kernel(std::conditional_t<PTRS, UpdPtrArgs, UpdArgs> a) {
    extern __shared__ uint4 lds4[];
    static_assert(MG % 4 == 0, "whole sub-steps");
    constexpr int TG = MG / kRowsPerStep;  // sub-steps per changed shard
    // Changed shards whose old/new loads are in flight, next to the MG parity
    // loads.  2, not matmul_block's 8: the common update changes one shard
    // of a stripe, and 4 cost 138 / 129 / 244 VGPRs (MG 4 / 8 / 16) against
    // 104 / 106 / 198.
    constexpr int JB = 2;

    uint64_t b = a.xcd ? xcd_block(blockIdx.x, a.xcd, gridDim.x) : blockIdx.x;
    const uint32_t grp = static_cast<uint32_t>(b % a.groups);
    b /= a.groups;
    const uint32_t chunk = static_cast<uint32_t>(b % a.chunks);
    const UpdateJob job = a.jobs[b / a.chunks];
    const uint64_t s = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe))) |
                       (static_cast<uint64_t>(static_cast<uint32_t>(
                            __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe >> 32))))
                        << 32);
    const UpdateEntry* ent = a.entries + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.first));
    const int j = __builtin_amdgcn_readfirstlane(job.j);
    const int row0 = static_cast<int>(grp) * MG;
    const int eg = min(MG, static_cast<int>(a.m) - row0);  // >= 1: groups = ceil(m / MG)

    uint32_t* tw = reinterpret_cast<uint32_t*>(lds4);
    uint8_t** optr = reinterpret_cast<uint8_t**>(tw + j * TG * kStepWords);
    uint8_t** nptr = optr + j;
    uint8_t* dbase = nullptr;      // strided layout: the stripe's data
    const uint64_t* tp = nullptr;  // pointer mode: the stripe's row of the shard table
    // Parity rows of this group; rows past eg are never dereferenced.
    uint8_t* pp[MG];
    // The first JB changed shards, resolved ahead of the LDS pointer arrays
    // for the loads that go out before the table build.
    uint8_t* po[JB];
    uint8_t* pn[JB];
    if constexpr (PTRS) {
        tp = a.shard_ptrs + s * (a.k + a.m);
        // Ids first, then every address the first iteration needs in one batch
        // of scalar loads: the group's parity rows and the first JB old
        // shards.  A row past eg or a shard past j takes the index of the last
        // real one -- an entry the block loads anyway, so that the batch has
        // no branches and never leaves the job's entries of the table -- and
        // is never dereferenced.
        uint32_t sh[JB];
#pragma unroll
        for (int q = 0; q < JB; ++q) {
            const UpdateEntry e = ent[min(q, j - 1)];
            sh[q] = __builtin_amdgcn_readfirstlane(e.shard);
            pn[q] = uniform_ptr(reinterpret_cast<uint8_t*>(e.src));
        }
#pragma unroll
        for (int r = 0; r < MG; ++r)
            pp[r] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[a.k + row0 + min(r, eg - 1)])) + a.shard_off;
#pragma unroll
        for (int q = 0; q < JB; ++q) po[q] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[sh[q]])) + a.shard_off;
    } else {
        dbase = a.data + s * a.data_ss;
        for (int i = threadIdx.x; i < j; i += BT) {
            const UpdateEntry e = ent[i];
            optr[i] = dbase + static_cast<uint64_t>(e.shard) * a.pitch;
            nptr[i] = reinterpret_cast<uint8_t*>(e.src);
        }
#pragma unroll
        for (int r = 0; r < MG; ++r)
            pp[r] = uniform_ptr(a.parity + s * a.parity_ss + static_cast<uint64_t>(row0 + r) * a.pitch);
    }

    const uint32_t last = a.ncols16 - 1;
    const uint32_t cstride = a.chunks * BT;
    const uint32_t col0 = chunk * BT + threadIdx.x;
    const uint32_t off0 = (col0 <= last ? col0 : last) * 16u;
    uint32_t acc[TG][kRowsPerStep][4];
    auto load_stored = [&](uint32_t at) {
#pragma unroll
        for (int g = 0; g < TG; ++g)
#pragma unroll
            for (int r = 0; r < kRowsPerStep; ++r) {
                uint4 p = make_uint4(0u, 0u, 0u, 0u);
                if (g * kRowsPerStep + r < eg) p = gload16<NT>(pp[g * kRowsPerStep + r] + at);
                acc[g][r][0] = p.x;
                acc[g][r][1] = p.y;
                acc[g][r][2] = p.z;
                acc[g][r][3] = p.w;
            }
    };
    // The first iteration's loads -- the stored parity columns and the old
    // and new columns of the first JB changed shards, their addresses taken
    // straight from the entry table -- go out before the table build; with
    // one iteration per block and j <= JB that is the whole data path.
    load_stored(off0);
    uint4 xo[JB], xn[JB];
#pragma unroll
    for (int q = 0; q < JB; ++q) {
        if (q >= j) break;
        if constexpr (PTRS) {
            xo[q] = gload16<NT>(po[q] + off0);
            xn[q] = gload16<NT>(pn[q] + off0);
        } else {
            const UpdateEntry e = ent[q];
            const uint32_t sh = __builtin_amdgcn_readfirstlane(e.shard);
            xo[q] = gload16<NT>(uniform_ptr(dbase + static_cast<uint64_t>(sh) * a.pitch) + off0);
            xn[q] = gload16<NT>(uniform_ptr(reinterpret_cast<uint8_t*>(e.src)) + off0);
        }
    }
    if constexpr (PTRS) {
        // The LDS pointer arrays (later iterations, shards past JB, the commit)
        // take two dependent vector loads per entry: behind the loads above,
        // not in front of them.
        for (int i = threadIdx.x; i < j; i += BT) {
            const UpdateEntry e = ent[i];
            optr[i] = reinterpret_cast<uint8_t*>(tp[e.shard]) + a.shard_off;
            nptr[i] = reinterpret_cast<uint8_t*>(e.src);
        }
    }
    // Split tables: sub-step (c, g) holds E[k + row0 + 4g .. + 3][shard_c].
    for (int idx = threadIdx.x; idx < j * MG; idx += BT) {
        const int c = idx / MG, t = idx - c * MG;
        const uint32_t cf = (t < eg) ? a.enc[static_cast<size_t>(a.k + row0 + t) * a.k + ent[c].shard] : 0u;
        build_tables(cf, &tw[(c * TG + t / kRowsPerStep) * kStepWords + (t % kRowsPerStep) * 5]);
    }
    __syncthreads();

    const int tg_used = (eg + kRowsPerStep - 1) / kRowsPerStep;
    bool preloaded = true;
    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint32_t colbase = chunk * BT + it * cstride;
        if (colbase >= a.ncols16) break;
        RS_MEM_FENCE();
        const uint32_t col = colbase + threadIdx.x;
        const bool ok = col <= last;
        // Tail lanes re-read the last column and store nothing: the lane that
        // owns that column may have patched it already.
        const uint32_t off = (ok ? col : last) * 16u;
        if (!preloaded) load_stored(off);
        for (int jb = 0; jb < j; jb += JB) {
            if (!preloaded) {
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (jb + q >= j) break;
                    xo[q] = gload16<NT>(uniform_ptr(optr[jb + q]) + off);
                    xn[q] = gload16<NT>(uniform_ptr(nptr[jb + q]) + off);
                }
            }
            preloaded = false;
            uint32_t TA[kStepWords], TB[kStepWords];
            load_step(lds4 + static_cast<size_t>(jb * TG) * (kStepWords / 4), TA);
#pragma unroll
            for (int q = 0; q < JB; ++q) {
                if (jb + q >= j) break;
                const uint4 x = make_uint4(xo[q].x ^ xn[q].x, xo[q].y ^ xn[q].y, xo[q].z ^ xn[q].z, xo[q].w ^ xn[q].w);
#pragma unroll
                for (int g = 0; g < TG; ++g) {
                    const int step = (jb + q) * TG + g;
                    const bool more = (g + 1 < TG) || (q + 1 < JB && jb + q + 1 < j);
                    if (more) load_step(lds4 + static_cast<size_t>(step + 1) * (kStepWords / 4), TB);
                    if (TG == 1 || g < tg_used) mac_step(acc[g], x, TA);
                    step_fence(acc[g]);
#pragma unroll
                    for (int w = 0; w < kStepWords; ++w) TA[w] = TB[w];
                }
                // Commit: the only block that reads this shard's old column
                // has consumed it.
                if (a.commit && ok) gstore16<NT>(uniform_ptr(optr[jb + q]) + off, xn[q]);
            }
        }
#pragma unroll
        for (int g = 0; g < TG; ++g)
#pragma unroll
            for (int r = 0; r < kRowsPerStep; ++r) {
                const int t = g * kRowsPerStep + r;
                if (t >= eg) break;
                if (ok) gstore16<NT>(pp[t] + off, make_uint4(acc[g][r][0], acc[g][r][1], acc[g][r][2], acc[g][r][3]));
            }
    }
}

// Caller-chosen combinations (rs_kernels.hpp CombArgs): rs_update_kernel's
// block decomposition with everything a job's own -- nsrc sources as the
// runtime "k", nout outputs cut into row groups of MG, the coefficient rows
// read from the job's slice of the coefficient table.  In accumulate mode the
// accumulators start as the stored destination columns and go back where they
// came from (as the update's parity); in overwrite mode they start at zero
// and the destinations are never read.
// LDS: [nsrc][MG/4][20] table dwords | nsrc source pointers.
//
// VARLEN (rs_combine_lens, CombLensArgs): every job has its own column count.
// The block finds its job by a search of first_block[] that only blockIdx
// feeds (combine_lens_map.hpp: scalar loads, uniform across the block), in
// natural block order, and takes every column bound -- the last column, the
// tail-lane clamp, the end of the iterations, the chunk stride -- from that
// job; a block never leaves its job.  a.iters is the most iterations any
// block runs.  The equal-length instances take none of this.
template <int MG, int BT, bool NT, bool VARLEN = false>
__global__ __launch_bounds__(BT) void rs_combine_kernel(std::conditional_t<VARLEN, CombLensArgs, CombArgs> a) {
    extern __shared__ uint4 lds4[];
    static_assert(MG % 4 == 0, "whole sub-steps");
    constexpr int TG = MG / kRowsPerStep;  // sub-steps per source
    // Sources whose loads are in flight, next to the MG stored columns of an
    // accumulating job: 4, the update kernel's depth (two shards, old and
    // new).  8 cost 138 VGPRs against 120 for MG 4 -- three waves per SIMD
    // where the update kernel runs four.
    constexpr int JB = 4;

    uint32_t grp, chunk, chunks, ncols;
    CombineJob job;
    if constexpr (VARLEN) {
        const CombineBlock at = combine_lens_block(a.first_block, a.njobs, a.groups, blockIdx.x);
        const uint32_t jb = __builtin_amdgcn_readfirstlane(at.job);
        grp = __builtin_amdgcn_readfirstlane(at.grp);
        chunk = __builtin_amdgcn_readfirstlane(at.chunk);
        chunks = __builtin_amdgcn_readfirstlane(at.chunks);
        ncols = __builtin_amdgcn_readfirstlane(a.ncols[jb]);
        job = a.jobs[jb];
    } else {
        uint64_t b = a.xcd ? xcd_block(blockIdx.x, a.xcd, gridDim.x) : blockIdx.x;
        grp = static_cast<uint32_t>(b % a.groups);
        b /= a.groups;
        chunk = static_cast<uint32_t>(b % a.chunks);
        job = a.jobs[b / a.chunks];
        chunks = a.chunks;
        ncols = a.ncols16;
    }
    const int nsrc = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.nsrc));
    const int nout = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.nout));
    const bool accumulate = __builtin_amdgcn_readfirstlane(job.accumulate) != 0;
    const int row0 = static_cast<int>(grp) * MG;
    if (row0 >= nout) return;  // whole block: uniform
    const int eg = min(MG, nout - row0);
    const uint64_t* sa = a.addrs + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.addr));
    const uint64_t* da = sa + nsrc + row0;
    const uint8_t* cf = a.coef + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.coef)) +
                        static_cast<size_t>(row0) * nsrc;

    uint32_t* tw = reinterpret_cast<uint32_t*>(lds4);
    uint8_t** sptr = reinterpret_cast<uint8_t**>(tw + nsrc * TG * kStepWords);
    for (int i = threadIdx.x; i < nsrc; i += BT) sptr[i] = reinterpret_cast<uint8_t*>(sa[i]);
    // Destinations of this group's rows; rows past eg have none.
    uint8_t* dp[MG];
#pragma unroll
    for (int r = 0; r < MG; ++r) dp[r] = r < eg ? uniform_ptr(reinterpret_cast<uint8_t*>(da[r])) : nullptr;

    const uint32_t last = ncols - 1;
    const uint32_t cstride = chunks * BT;
    const uint32_t col0 = chunk * BT + threadIdx.x;
    const uint32_t off0 = (col0 <= last ? col0 : last) * 16u;
    uint32_t acc[TG][kRowsPerStep][4];
    auto load_stored = [&](uint32_t at) {
#pragma unroll
        for (int g = 0; g < TG; ++g)
#pragma unroll
            for (int r = 0; r < kRowsPerStep; ++r) {
                uint4 p = make_uint4(0u, 0u, 0u, 0u);
                if (accumulate && g * kRowsPerStep + r < eg) p = gload16<NT>(dp[g * kRowsPerStep + r] + at);
                acc[g][r][0] = p.x;
                acc[g][r][1] = p.y;
                acc[g][r][2] = p.z;
                acc[g][r][3] = p.w;
            }
    };
    // The first iteration's loads -- the stored columns and the first JB
    // sources, their addresses taken straight from the address table -- go
    // out before the table build; with one iteration per block and nsrc <= JB
    // that is the whole data path.
    load_stored(off0);
    uint4 x[JB];
#pragma unroll
    for (int q = 0; q < JB; ++q) {
        if (q >= nsrc) break;
        x[q] = gload16<NT>(uniform_ptr(reinterpret_cast<uint8_t*>(sa[q])) + off0);
    }
    // Split tables: sub-step (c, g) holds coef[row0 + 4g .. + 3][c].
    for (int idx = threadIdx.x; idx < nsrc * MG; idx += BT) {
        const int c = idx / MG, t = idx - c * MG;
        const uint32_t v = (t < eg) ? cf[static_cast<size_t>(t) * nsrc + c] : 0u;
        build_tables(v, &tw[(c * TG + t / kRowsPerStep) * kStepWords + (t % kRowsPerStep) * 5]);
    }
    __syncthreads();

    [[maybe_unused]] const int tg_used = (eg + kRowsPerStep - 1) / kRowsPerStep;
    bool preloaded = true;
    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint32_t colbase = chunk * BT + it * cstride;
        if (colbase >= ncols) break;
        RS_MEM_FENCE();
        const uint32_t col = colbase + threadIdx.x;
        const bool ok = col <= last;
        // Tail lanes re-read the last column and store nothing: the lane that
        // owns that column may have written it already.
        const uint32_t off = (ok ? col : last) * 16u;
        if (!preloaded) load_stored(off);
        for (int jb = 0; jb < nsrc; jb += JB) {
            if (!preloaded) {
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (jb + q >= nsrc) break;
                    x[q] = gload16<NT>(uniform_ptr(sptr[jb + q]) + off);
                }
            }
            preloaded = false;
            uint32_t TA[kStepWords], TB[kStepWords];
            load_step(lds4 + static_cast<size_t>(jb * TG) * (kStepWords / 4), TA);
#pragma unroll
            for (int q = 0; q < JB; ++q) {
                if (jb + q >= nsrc) break;
#pragma unroll
                for (int g = 0; g < TG; ++g) {
                    const int step = (jb + q) * TG + g;
                    const bool more = (g + 1 < TG) || (q + 1 < JB && jb + q + 1 < nsrc);
                    if (more) load_step(lds4 + static_cast<size_t>(step + 1) * (kStepWords / 4), TB);
                    // Row groups of 4 multiply only the group's eg rows (a
                    // job of one output pays for one); wider ones whole
                    // sub-steps, as the update kernel.
                    if constexpr (TG == 1) {
                        if (eg == kRowsPerStep) mac_step(acc[g], x[q], TA);
                        else mac_step_rows(acc[g], x[q], TA, eg);
                    } else if (g < tg_used) {
                        mac_step(acc[g], x[q], TA);
                    }
                    step_fence(acc[g]);
#pragma unroll
                    for (int w = 0; w < kStepWords; ++w) TA[w] = TB[w];
                }
            }
        }
#pragma unroll
        for (int g = 0; g < TG; ++g)
#pragma unroll
            for (int r = 0; r < kRowsPerStep; ++r) {
                const int t = g * kRowsPerStep + r;
                if (t >= eg) break;
                if (ok) gstore16<NT>(dp[t] + off, make_uint4(acc[g][r][0], acc[g][r][1], acc[g][r][2], acc[g][r][3]));
            }
    }
}

// In-place parity update of stripes with missing shards (rs_kernels.hpp
// DegArgs): rs_update_kernel's block decomposition and accumulators -- the
// stored columns of the job's PRESENT parity rows, which go back where they
// came from -- over rs_combine_kernel's source loop.  A source is up to two
// loads, XORed, and an optional commit address:
//   pair form    source c = (new_c, old_c), coefficient E[k + r][c]; old_c is
//                the shard's slot, or the entry's `old` buffer;
//   decode form  sources 0 .. k - 1 are the survivors of the job's pattern,
//                k .. k + j - 1 the new buffers.  With D the pattern's decode
//                rows, old_c = sum_i D[rank_c][i] * survivor_i for an erased
//                changed shard c, so the patch of row r is
//                    sum_i (sum_{c in U_x} E[k+r][c] * D[rank_c][i]) * survivor_i
//                  ^ sum_{c' in U_p} E[k+r][c'] * survivor_c'   (a present data
//                    shard is the survivor of its own slot)
//                  ^ sum_{c in U} E[k+r][c] * new_c,
//                and the block composes those coefficients in its table build
//                (gfd::gf_mul).  No scratch, and no slot of an erased shard is
//                ever addressed: the survivors are present by construction,
//                the rows are the present ones, and only present changed
//                shards have a commit address.
// In place: in the decode form a parity survivor is a source AND an output,
// and a present changed shard is a source and is overwritten.  That is safe
// only because ONE block owns every read and write of a column of a stripe --
// hence one row group (groups == 1) -- and, lane by lane, it reads all of
// them in program order before it stores any: the accumulators and every
// survivor's column are loaded before the first commit (the new buffers
// follow the survivors in the source order) and the parity goes out last.
// Tail lanes re-read the last column and store nothing, as in the update
// kernel, and nothing is prefetched for the next iteration but other columns.
// The pair form has no such source, so it may run several row groups; then
// commit is 0 and the caller copies the new contents in behind the kernel.
// LDS: [nsrc][MG/4][20] table dwords | nsrc x {load, second load or 0, commit or 0}.
template <int MG, int BT, bool NT>
__global__ __launch_bounds__(BT) void rs_update_degraded_kernel(DegArgs a) {
    extern __shared__ uint4 lds4[];
    static_assert(MG % 4 == 0, "whole sub-steps");
    constexpr int TG = MG / kRowsPerStep;  // sub-steps per source
    // Sources whose loads are in flight, next to the MG parity loads: 4 as in
    // the combine kernel -- a pair-form job of two changed shards has all its
    // loads out at once, as in the update kernel.
    constexpr int JB = 4;

    uint64_t b = a.xcd ? xcd_block(blockIdx.x, a.xcd, gridDim.x) : blockIdx.x;
    const uint32_t grp = static_cast<uint32_t>(b % a.groups);
    b /= a.groups;
    const uint32_t chunk = static_cast<uint32_t>(b % a.chunks);
    const DegJob job = a.jobs[b / a.chunks];
    const uint64_t s = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe))) |
                       (static_cast<uint64_t>(static_cast<uint32_t>(
                            __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe >> 32))))
                        << 32);
    const DegEntry* ent = a.entries + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.first));
    const int j = __builtin_amdgcn_readfirstlane(job.j);
    const int jp = j - static_cast<int>(__builtin_amdgcn_readfirstlane(job.jx));  // present entries come first
    const int nrows = __builtin_amdgcn_readfirstlane(job.nrows);
    const uint32_t pat = __builtin_amdgcn_readfirstlane(job.pat);
    const bool decode = pat != kDegNoPattern;
    const int k = static_cast<int>(a.k);
    const int nsrc = decode ? k + j : j;
    const int row0 = static_cast<int>(grp) * MG;
    // A job with fewer present rows than the call's row groups cover leaves
    // its surplus blocks idle; the first block stays, with no rows at all if
    // need be: it commits the data.
    if (grp > 0 && row0 >= nrows) return;  // whole block: uniform
    const int eg = max(0, min(MG, nrows - row0));
    const uint32_t* rows = a.rows + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.row_first)) + row0;
    const uint32_t* srcid = decode ? a.src + static_cast<size_t>(pat) * k : nullptr;
    const uint8_t* drow = decode ? a.coef + static_cast<size_t>(pat) * a.m * k : nullptr;
    uint8_t* dbase = a.data + s * a.data_ss;
    uint8_t* pbase = a.parity + s * a.parity_ss;

    // Source i: what to load (l0, and l1 or null) and where the block commits
    // l0's column afterwards (cm or null).
    auto source = [&](int i, uint8_t*& l0, uint8_t*& l1, uint8_t*& cm) {
        l1 = nullptr;
        cm = nullptr;
        if (decode && i < k) {
            const uint32_t id = srcid[i];
            l0 = id < a.k ? dbase + static_cast<uint64_t>(id) * a.pitch
                          : pbase + static_cast<uint64_t>(id - a.k) * a.pitch;
            return;
        }
        const DegEntry e = ent[decode ? i - k : i];
        uint8_t* slot = dbase + static_cast<uint64_t>(e.shard) * a.pitch;
        l0 = reinterpret_cast<uint8_t*>(e.src);
        if (!decode) l1 = e.old ? reinterpret_cast<uint8_t*>(e.old) : slot;
        if (a.commit && e.rank == kDegPresent) cm = slot;
    };

    uint32_t* tw = reinterpret_cast<uint32_t*>(lds4);
    uint8_t** sp = reinterpret_cast<uint8_t**>(tw + nsrc * TG * kStepWords);
    for (int i = threadIdx.x; i < nsrc; i += BT) source(i, sp[3 * i], sp[3 * i + 1], sp[3 * i + 2]);
    // Present parity rows of this group; rows past eg are never dereferenced.
    uint8_t* pp[MG];
#pragma unroll
    for (int r = 0; r < MG; ++r)
        pp[r] = r < eg ? uniform_ptr(pbase + static_cast<uint64_t>(rows[r]) * a.pitch) : nullptr;

    const uint32_t last = a.ncols16 - 1;
    const uint32_t cstride = a.chunks * BT;
    const uint32_t col0 = chunk * BT + threadIdx.x;
    const uint32_t off0 = (col0 <= last ? col0 : last) * 16u;
    uint32_t acc[TG][kRowsPerStep][4];
    auto load_stored = [&](uint32_t at) {
#pragma unroll
        for (int g = 0; g < TG; ++g)
#pragma unroll
            for (int r = 0; r < kRowsPerStep; ++r) {
                uint4 p = make_uint4(0u, 0u, 0u, 0u);
                if (g * kRowsPerStep + r < eg) p = gload16<NT>(pp[g * kRowsPerStep + r] + at);
                acc[g][r][0] = p.x;
                acc[g][r][1] = p.y;
                acc[g][r][2] = p.z;
                acc[g][r][3] = p.w;
            }
    };
    // The first iteration's loads -- the stored parity columns and the first
    // JB sources, their addresses taken straight from the tables -- go out
    // before the table build, as in the update kernel.
    load_stored(off0);
    uint4 x0[JB], x1[JB];
#pragma unroll
    for (int q = 0; q < JB; ++q) {
        if (q >= nsrc) break;
        uint8_t *l0, *l1, *cm;
        source(q, l0, l1, cm);
        l1 = uniform_ptr(l1);
        x0[q] = gload16<NT>(uniform_ptr(l0) + off0);
        x1[q] = make_uint4(0u, 0u, 0u, 0u);
        if (l1) x1[q] = gload16<NT>(l1 + off0);
    }
    // Split tables: sub-step (c, g) holds source c's coefficients for rows
    // rows[4g .. 4g + 3] of the group.
    const uint8_t* gf_exp = a.enc + static_cast<size_t>(a.k + a.m) * a.k;
    const uint8_t* gf_log = gf_exp + 512;
    for (int idx = threadIdx.x; idx < nsrc * MG; idx += BT) {
        const int c = idx / MG, t = idx - c * MG;
        uint32_t cf = 0u;
        if (t < eg) {
            const uint8_t* er = a.enc + static_cast<size_t>(a.k + rows[t]) * a.k;  // E[k + r][.]
            if (!decode) {
                cf = er[ent[c].shard];
            } else if (c >= k) {
                cf = er[ent[c - k].shard];
            } else {
                for (int x = jp; x < j; ++x)
                    cf ^= gfd::gf_mul(gf_exp, gf_log, er[ent[x].shard], drow[static_cast<size_t>(ent[x].rank) * k + c]);
                // A present data shard is the survivor of its own slot: if it
                // changes, its old contents are this source.
                const uint32_t id = srcid[c];
                if (id < a.k)
                    for (int x = 0; x < jp; ++x)
                        if (ent[x].shard == id) cf ^= er[id];
            }
        }
        build_tables(cf, &tw[(c * TG + t / kRowsPerStep) * kStepWords + (t % kRowsPerStep) * 5]);
    }
    __syncthreads();

    [[maybe_unused]] const int tg_used = (eg + kRowsPerStep - 1) / kRowsPerStep;
    bool preloaded = true;
    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint32_t colbase = chunk * BT + it * cstride;
        if (colbase >= a.ncols16) break;
        RS_MEM_FENCE();
        const uint32_t col = colbase + threadIdx.x;
        const bool ok = col <= last;
        // Tail lanes re-read the last column and store nothing: the lane that
        // owns that column may have patched it already.
        const uint32_t off = (ok ? col : last) * 16u;
        if (!preloaded) load_stored(off);
        for (int jb = 0; jb < nsrc; jb += JB) {
            if (!preloaded) {
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (jb + q >= nsrc) break;
                    uint8_t* l1 = uniform_ptr(sp[3 * (jb + q) + 1]);
                    x0[q] = gload16<NT>(uniform_ptr(sp[3 * (jb + q)]) + off);
                    x1[q] = make_uint4(0u, 0u, 0u, 0u);
                    if (l1) x1[q] = gload16<NT>(l1 + off);
                }
            }
            preloaded = false;
            uint32_t TA[kStepWords], TB[kStepWords];
            load_step(lds4 + static_cast<size_t>(jb * TG) * (kStepWords / 4), TA);
#pragma unroll
            for (int q = 0; q < JB; ++q) {
                if (jb + q >= nsrc) break;
                const uint4 x = make_uint4(x0[q].x ^ x1[q].x, x0[q].y ^ x1[q].y, x0[q].z ^ x1[q].z, x0[q].w ^ x1[q].w);
#pragma unroll
                for (int g = 0; g < TG; ++g) {
                    const int step = (jb + q) * TG + g;
                    const bool more = (g + 1 < TG) || (q + 1 < JB && jb + q + 1 < nsrc);
                    if (more) load_step(lds4 + static_cast<size_t>(step + 1) * (kStepWords / 4), TB);
                    // Row groups of 4 multiply only the present rows (a stripe
                    // that has lost three of four parity shards pays for
                    // one); wider ones whole sub-steps, as the combine kernel.
                    if constexpr (TG == 1) {
                        if (eg == kRowsPerStep) mac_step(acc[g], x, TA);
                        else mac_step_rows(acc[g], x, TA, eg);
                    } else if (g < tg_used) {
                        mac_step(acc[g], x, TA);
                    }
                    step_fence(acc[g]);
#pragma unroll
                    for (int w = 0; w < kStepWords; ++w) TA[w] = TB[w];
                }
                // Commit: every load of this column that reads the shard's
                // old contents -- its own pair, or the survivors, all of them
                // ahead of the new buffers -- has been issued by this lane.
                uint8_t* cm = uniform_ptr(sp[3 * (jb + q) + 2]);
                if (cm && ok) gstore16<NT>(cm + off, x0[q]);
            }
        }
#pragma unroll
        for (int g = 0; g < TG; ++g)
#pragma unroll
            for (int r = 0; r < kRowsPerStep; ++r) {
                const int t = g * kRowsPerStep + r;
                if (t >= eg) break;
                if (ok) gstore16<NT>(pp[t] + off, make_uint4(acc[g][r][0], acc[g][r][1], acc[g][r][2], acc[g][r][3]));
            }
    }
}

// Degraded read (rs_kernels.hpp ReadArgs): the split-table matmul_block with
// the rows and the outputs taken from the job's entry table instead of the
// pattern.  Row t of the block's group is row entries[first + row0 + t].row of
// the cached pattern -- the pattern's other rows are neither multiplied nor
// stored -- and its columns go to entries[first + row0 + t].dst with the same
// 16-byte stores.  The survivors come from the strided layout through the
// pattern's src ids; nothing in the stripes is written.
// One sub-step per survivor (MG = 4) and only the group's eg wanted rows are
// multiplied (mac_step_rows) whatever K is: the common read wants one row.
// LDS: [k][20] table dwords | k survivor pointers.
//
// PTRS (compile-time twin, launch_read_ptrs): shard id of stripe s is at
// a.shard_ptrs[s * n + id] and the layout fields of `a` are unused.  The
// survivors' addresses are resolved exactly as rs_check_kernel<..., PTRS>
// resolves them: one batch of scalar loads from the table behind the batch of
// ids (K <= 16), or the LDS pointer array -- and there the first 4 survivors by
// scalar loads too, their first loads ahead of the barrier (kEarly below), which
// the check kernel's twin does not do.  a.shard_off, the byte offset of the
// call's slice within every slot, is added once to each resolved base.
// entries[..].dst stays a real destination and receives the slice from its
// start.  The table entries of erased shards are never loaded: the pattern's
// survivors are all present.
struct ReadPtrArgs : ReadArgs {
    const uint64_t* shard_ptrs;
    uint64_t shard_off;
};
template <int K, int MG, int BT, bool NT, bool PTRS = false>
__global__ __launch_bounds__(BT) void rs_read_kernel(std::conditional_t<PTRS, ReadPtrArgs, ReadArgs> a) {
    extern __shared__ uint4 lds4[];
    static_assert(MG == kRowsPerStep, "one table sub-step per survivor");
    constexpr bool kRegPtrs = K > 0 && K <= 16;           // survivor bases kept in SGPRs
    constexpr int JB = (K == 0) ? 8 : (K <= 16 ? K : 8);  // survivor loads in flight
    const int k = K ? K : static_cast<int>(a.k);
    uint32_t* tw = reinterpret_cast<uint32_t*>(lds4);
    uint8_t** sptr = reinterpret_cast<uint8_t**>(tw + k * kStepWords);

    uint64_t b = a.xcd ? xcd_block(blockIdx.x, a.xcd, gridDim.x) : blockIdx.x;
    const uint32_t grp = static_cast<uint32_t>(b % a.groups);
    b /= a.groups;
    const uint32_t chunk = static_cast<uint32_t>(b % a.chunks);
    const uint64_t ji = b / a.chunks;
    const ReadJob job = a.jobs[ji];
    const uint64_t s = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe))) |
                       (static_cast<uint64_t>(static_cast<uint32_t>(
                            __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe >> 32))))
                        << 32);
    const int j = __builtin_amdgcn_readfirstlane(job.j);
    const int row0 = static_cast<int>(grp) * MG;
    if (row0 >= j) return;  // whole block: uniform
    const int eg = min(MG, j - row0);
    const ReadEntry* ent = a.entries + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.first)) + row0;
    const uint32_t pat = __builtin_amdgcn_readfirstlane(a.pats[ji]);

    // This lane's coefficient byte for the table build is requested first, so
    // waiting for it later does not wait for the survivor loads behind it.
    const uint8_t* coef = a.coef + static_cast<size_t>(pat) * a.m * k;
    constexpr bool one_coef = (K > 0 && K * MG <= BT);
    uint32_t cbyte = 0u;
    if constexpr (one_coef) {
        const int c = threadIdx.x / MG, t = threadIdx.x - c * MG;
        if (static_cast<int>(threadIdx.x) < k * MG && t < eg) cbyte = coef[static_cast<size_t>(ent[t].row) * k + c];
    }

    const uint32_t* srcid = a.src + static_cast<size_t>(pat) * k;
    uint8_t* sp[kRegPtrs ? K : 1];
    // The twin's LDS pointer path: its fill takes two dependent vector loads
    // per survivor (id, then table entry) where the strided kernel's takes
    // one, so the first EB survivors are resolved by scalar loads as well and
    // their first-iteration loads go out ahead of the fill, the table build
    // and the barrier (below, where off0 is known).
    constexpr bool kEarly = PTRS && !kRegPtrs;
    // Early survivors: 4 of the batch's JB = 8.  All 8 cost 135 VGPRs against
    // the strided kernel's 103 -- past 128, a wave per SIMD less.
    constexpr int EB = 4;
    const uint64_t* tp = nullptr;  // pointer mode: the stripe's row of the shard table
    if constexpr (PTRS) {
        tp = a.shard_ptrs + s * (a.k + a.m);
        if constexpr (kRegPtrs) {
            uint32_t ids[K];
#pragma unroll
            for (int c = 0; c < K; ++c) ids[c] = __builtin_amdgcn_readfirstlane(srcid[c]);
#pragma unroll
            for (int c = 0; c < K; ++c) sp[c] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[ids[c]])) + a.shard_off;
        }
    } else {
        uint8_t* dbase = const_cast<uint8_t*>(a.data) + s * a.data_ss;
        uint8_t* pbase = const_cast<uint8_t*>(a.parity) + s * a.parity_ss;
        if constexpr (kRegPtrs) {
            uint32_t ids[K];
#pragma unroll
            for (int c = 0; c < K; ++c) ids[c] = __builtin_amdgcn_readfirstlane(srcid[c]);
#pragma unroll
            for (int c = 0; c < K; ++c)
                sp[c] = ids[c] < static_cast<uint32_t>(K) ? dbase + static_cast<uint64_t>(ids[c]) * a.pitch
                                                         : pbase + static_cast<uint64_t>(ids[c] - K) * a.pitch;
        } else {
            for (int i = threadIdx.x; i < k; i += BT) {
                const uint32_t id = srcid[i];
                sptr[i] = id < a.k ? dbase + static_cast<uint64_t>(id) * a.pitch
                                   : pbase + static_cast<uint64_t>(id - a.k) * a.pitch;
            }
        }
    }
    const uint32_t last = a.ncols16 - 1;
    // Survivor loads of the block's first iteration go out before the table
    // build, as in matmul_block.
    uint4 xpre[kRegPtrs ? K : 1];
    const uint32_t cstride = a.chunks * BT;
    const uint32_t col0 = chunk * BT + threadIdx.x;
    const uint32_t off0 = (col0 <= last ? col0 : last) * 16u;
    if constexpr (kRegPtrs) {
#pragma unroll
        for (int c = 0; c < K; ++c) xpre[c] = gload16<NT>(sp[c] + off0);
    }
    uint4 xe[kEarly ? EB : 1];
    if constexpr (kEarly) {
        // A survivor past k (runtime k < EB) takes the index of the last one:
        // a batch without branches that stays within the entries the block
        // loads anyway; its column is loaded and never used.
        uint32_t ids[EB];
#pragma unroll
        for (int q = 0; q < EB; ++q) ids[q] = __builtin_amdgcn_readfirstlane(srcid[min(q, k - 1)]);
        uint8_t* pe[EB];
#pragma unroll
        for (int q = 0; q < EB; ++q) pe[q] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[ids[q]])) + a.shard_off;
#pragma unroll
        for (int q = 0; q < EB; ++q) xe[q] = gload16<NT>(pe[q] + off0);
        for (int i = threadIdx.x; i < k; i += BT)
            sptr[i] = reinterpret_cast<uint8_t*>(tp[srcid[i]]) + a.shard_off;
    }
    // Destinations of the group's wanted rows; rows past eg have none.
    uint8_t* dp[MG];
#pragma unroll
    for (int t = 0; t < MG; ++t) dp[t] = t < eg ? uniform_ptr(reinterpret_cast<uint8_t*>(ent[t].dst)) : nullptr;
    // Split tables of the wanted rows: survivor c's sub-step holds 4 x 5 dwords.
    if constexpr (one_coef) {
        if (static_cast<int>(threadIdx.x) < k * MG) {
            const int c = threadIdx.x / MG, t = threadIdx.x - c * MG;
            build_tables(cbyte, &tw[c * kStepWords + t * 5]);
        }
    } else {
        for (int idx = threadIdx.x; idx < k * MG; idx += BT) {
            const int c = idx / MG, t = idx - c * MG;
            const uint32_t cf = (t < eg) ? coef[static_cast<size_t>(ent[t].row) * k + c] : 0u;
            build_tables(cf, &tw[c * kStepWords + t * 5]);
        }
    }
    __syncthreads();

    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint32_t colbase = chunk * BT + it * cstride;
        if (colbase >= a.ncols16) break;
        RS_MEM_FENCE();
        const uint32_t col = colbase + threadIdx.x;
        const bool ok = col <= last;
        // Tail lanes re-read the last column (always in bounds) and skip the store.
        const uint32_t off = (ok ? col : last) * 16u;
        uint32_t acc[kRowsPerStep][4];
#pragma unroll
        for (int r = 0; r < kRowsPerStep; ++r)
#pragma unroll
            for (int w = 0; w < 4; ++w) acc[r][w] = 0u;

        for (int jb = 0; jb < k; jb += JB) {
            uint4 xb[kRegPtrs ? 1 : JB];
            uint4* x = kRegPtrs ? xpre : xb;
            if constexpr (kEarly) {
                // The first EB columns of the block's first batch were loaded
                // ahead of the table build (off == off0 there).
                const bool early = it == 0 && jb == 0;
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (K == 0 && jb + q >= k) break;
                    if (q < EB && early) x[q] = xe[q];
                    else x[q] = gload16<NT>(uniform_ptr(sptr[jb + q]) + off);
                }
            } else if constexpr (!kRegPtrs) {
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (K == 0 && jb + q >= k) break;
                    x[q] = gload16<NT>(uniform_ptr(sptr[jb + q]) + off);
                }
            }
            uint32_t TA[kStepWords], TB[kStepWords];
            load_step(lds4 + static_cast<size_t>(jb) * (kStepWords / 4), TA);
#pragma unroll
            for (int q = 0; q < JB; ++q) {
                if (K == 0 && jb + q >= k) break;
                const bool more = q + 1 < JB && (K != 0 || jb + q + 1 < k);
                if (more) load_step(lds4 + static_cast<size_t>(jb + q + 1) * (kStepWords / 4), TB);
                mac_step_rows(acc, x[q], TA, eg);
                step_fence(acc);
#pragma unroll
                for (int w = 0; w < kStepWords; ++w) TA[w] = TB[w];
            }
        }
        if constexpr (kRegPtrs) {
            // Software pipelining: the next iteration's survivor loads go out
            // before this iteration's stores.
            const uint32_t ncol = colbase + cstride + threadIdx.x;
            if (it + 1 < a.iters && colbase + cstride < a.ncols16) {
                const uint32_t noff = (ncol <= last ? ncol : last) * 16u;
#pragma unroll
                for (int c = 0; c < K; ++c) xpre[c] = gload16<NT>(sp[c] + noff);
            }
        }
#pragma unroll
        for (int t = 0; t < kRowsPerStep; ++t) {
            if (t >= eg) break;
            if (ok) gstore16<NT>(dp[t] + off, make_uint4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]));
        }
    }
}

// Degraded check (rs_kernels.hpp launch_check): the verify twin of
// rs_read_kernel, with a body of its own.  A job's entries are the stripe's
// present shards outside the pattern's survivors; entries[..].dst is the
// address of the STORED shard and is only read.  The block loads the stored
// 16-byte columns of its group's rows behind the survivor loads and before
// the table build, into the accumulators (as matmul_block<VF>): after the
// MACs an accumulator holds stored ^ recomputed, and the first mismatching
// lane of a wave does one atomicMin on first_bad[stripe].  Nothing else is
// stored; the slots of erased shards are in neither the pattern's survivors
// nor the entries, so no address into them is ever formed.
// LDS: [k][20] table dwords | k survivor pointers.
//
// PTRS (compile-time twin, launch_check_ptrs): shard id of stripe s is at
// a.shard_ptrs[s * n + id].  The survivors' addresses are one batch of scalar
// loads from the table behind the batch of ids (K <= 16) or go to the LDS
// pointer array; entries[..].dst is the stored shard's ID and is resolved
// through the table too.  The table entries of erased shards are never loaded.
struct CheckPtrArgs : ReadArgs {
    const uint64_t* shard_ptrs;
};
// VARLEN (compile-time twin of the PTRS one, launch_check_lens): job b has
// ncols[b] 16-byte columns and lens[b] bytes and owns the blocks
// [first_block[b], first_block[b + 1]) of the grid; a.ncols16, a.chunks, a.xcd
// and the shard_len argument are unused.
struct CheckLensArgs : CheckPtrArgs {
    const uint32_t* first_block;
    const uint32_t* ncols;
    const uint32_t* lens;
};
template <int K, int MG, int BT, bool NT, bool PTRS = false, bool VARLEN = false>
__global__ __launch_bounds__(BT) void rs_check_kernel(std::conditional_t<VARLEN, CheckLensArgs, std::conditional_t<PTRS, CheckPtrArgs, ReadArgs>> a,
                                                      uint32_t* first_bad, uint32_t shard_len) {
    extern __shared__ uint4 lds4[];
    static_assert(MG == kRowsPerStep, "one table sub-step per survivor");
    constexpr bool kRegPtrs = K > 0 && K <= 16;           // survivor bases kept in SGPRs
    constexpr int JB = (K == 0) ? 8 : (K <= 16 ? K : 8);  // survivor loads in flight
    const int k = K ? K : static_cast<int>(a.k);
    uint32_t* tw = reinterpret_cast<uint32_t*>(lds4);
    uint8_t** sptr = reinterpret_cast<uint8_t**>(tw + k * kStepWords);

    static_assert(!VARLEN || PTRS, "per-stripe lengths: the pointer placement only");
    uint32_t grp, chunk, chunks, ncols16;
    uint64_t ji;
    if constexpr (VARLEN) {
        // The job's own column count and shard length (see matmul_block).
        const CombineBlock at = combine_lens_block(a.first_block, a.njobs, a.groups, blockIdx.x);
        ji = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(at.job));
        grp = __builtin_amdgcn_readfirstlane(at.grp);
        chunk = __builtin_amdgcn_readfirstlane(at.chunk);
        chunks = __builtin_amdgcn_readfirstlane(at.chunks);
        ncols16 = __builtin_amdgcn_readfirstlane(a.ncols[ji]);
        shard_len = __builtin_amdgcn_readfirstlane(a.lens[ji]);
    } else {
        uint64_t b = a.xcd ? xcd_block(blockIdx.x, a.xcd, gridDim.x) : blockIdx.x;
        grp = static_cast<uint32_t>(b % a.groups);
        b /= a.groups;
        chunk = static_cast<uint32_t>(b % a.chunks);
        ji = b / a.chunks;
        chunks = a.chunks;
        ncols16 = a.ncols16;
    }
    const ReadJob job = a.jobs[ji];
    // Stripe indices of a check fit 32 bits (plan_checks).
    const uint64_t s = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe)));
    const int j = __builtin_amdgcn_readfirstlane(job.j);
    const int row0 = static_cast<int>(grp) * MG;
    if (row0 >= j) return;  // whole block: uniform
    const int eg = min(MG, j - row0);
    const ReadEntry* ent = a.entries + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.first)) + row0;
    const uint32_t pat = __builtin_amdgcn_readfirstlane(a.pats[ji]);

    // This lane's coefficient byte for the table build is requested first, so
    // waiting for it later does not wait for the survivor loads behind it.
    const uint8_t* coef = a.coef + static_cast<size_t>(pat) * a.m * k;
    constexpr bool one_coef = (K > 0 && K * MG <= BT);
    uint32_t cbyte = 0u;
    if constexpr (one_coef) {
        const int c = threadIdx.x / MG, t = threadIdx.x - c * MG;
        if (static_cast<int>(threadIdx.x) < k * MG && t < eg) cbyte = coef[static_cast<size_t>(ent[t].row) * k + c];
    }

    const uint32_t* srcid = a.src + static_cast<size_t>(pat) * k;
    uint8_t* sp[kRegPtrs ? K : 1];
    const uint64_t* tp = nullptr;  // pointer mode: the stripe's row of the shard table
    if constexpr (PTRS) {
        tp = a.shard_ptrs + s * (a.k + a.m);
        if constexpr (kRegPtrs) {
            uint32_t ids[K];
#pragma unroll
            for (int c = 0; c < K; ++c) ids[c] = __builtin_amdgcn_readfirstlane(srcid[c]);
#pragma unroll
            for (int c = 0; c < K; ++c) sp[c] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[ids[c]]));
        } else {
            for (int i = threadIdx.x; i < k; i += BT) sptr[i] = reinterpret_cast<uint8_t*>(tp[srcid[i]]);
        }
    } else {
        uint8_t* dbase = const_cast<uint8_t*>(a.data) + s * a.data_ss;
        uint8_t* pbase = const_cast<uint8_t*>(a.parity) + s * a.parity_ss;
        if constexpr (kRegPtrs) {
            uint32_t ids[K];
#pragma unroll
            for (int c = 0; c < K; ++c) ids[c] = __builtin_amdgcn_readfirstlane(srcid[c]);
#pragma unroll
            for (int c = 0; c < K; ++c)
                sp[c] = ids[c] < static_cast<uint32_t>(K) ? dbase + static_cast<uint64_t>(ids[c]) * a.pitch
                                                         : pbase + static_cast<uint64_t>(ids[c] - K) * a.pitch;
        } else {
            for (int i = threadIdx.x; i < k; i += BT) {
                const uint32_t id = srcid[i];
                sptr[i] = id < a.k ? dbase + static_cast<uint64_t>(id) * a.pitch
                                   : pbase + static_cast<uint64_t>(id - a.k) * a.pitch;
            }
        }
    }
    const uint32_t last = ncols16 - 1;
    // Survivor loads of the block's first iteration go out before the table
    // build, as in matmul_block.
    uint4 xpre[kRegPtrs ? K : 1];
    const uint32_t cstride = chunks * BT;
    const uint32_t col0 = chunk * BT + threadIdx.x;
    const uint32_t off0 = (col0 <= last ? col0 : last) * 16u;
    if constexpr (kRegPtrs) {
#pragma unroll
        for (int c = 0; c < K; ++c) xpre[c] = gload16<NT>(sp[c] + off0);
    }
    // Stored shards of the group's rows; rows past eg have none.
    const uint8_t* dp[MG];
    if constexpr (PTRS) {
        // The entries carry shard ids: all of them first, then their addresses.
        uint32_t oid[MG];
#pragma unroll
        for (int t = 0; t < MG; ++t)
            oid[t] = t < eg ? __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(ent[t].dst)) : 0u;
#pragma unroll
        for (int t = 0; t < MG; ++t) dp[t] = t < eg ? uniform_ptr(reinterpret_cast<uint8_t*>(tp[oid[t]])) : nullptr;
    } else {
#pragma unroll
        for (int t = 0; t < MG; ++t) dp[t] = t < eg ? uniform_ptr(reinterpret_cast<uint8_t*>(ent[t].dst)) : nullptr;
    }
    // The accumulators start as the stored columns, loaded next to the
    // survivors so they ride the same latency.  Rows past eg are not read and
    // stay zero (they are not multiplied either, so they never report).
    uint32_t acc[kRowsPerStep][4];
    auto load_stored = [&](uint32_t at) {
#pragma unroll
        for (int r = 0; r < kRowsPerStep; ++r) {
            uint4 p = make_uint4(0u, 0u, 0u, 0u);
            if (r < eg) p = gload16<NT>(dp[r] + at);
            acc[r][0] = p.x;
            acc[r][1] = p.y;
            acc[r][2] = p.z;
            acc[r][3] = p.w;
        }
    };
    load_stored(off0);
    // Split tables of the group's rows: survivor c's sub-step holds 4 x 5 dwords.
    if constexpr (one_coef) {
        if (static_cast<int>(threadIdx.x) < k * MG) {
            const int c = threadIdx.x / MG, t = threadIdx.x - c * MG;
            build_tables(cbyte, &tw[c * kStepWords + t * 5]);
        }
    } else {
        for (int idx = threadIdx.x; idx < k * MG; idx += BT) {
            const int c = idx / MG, t = idx - c * MG;
            const uint32_t cf = (t < eg) ? coef[static_cast<size_t>(ent[t].row) * k + c] : 0u;
            build_tables(cf, &tw[c * kStepWords + t * 5]);
        }
    }
    __syncthreads();

    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint32_t colbase = chunk * BT + it * cstride;
        if (colbase >= ncols16) break;
        RS_MEM_FENCE();
        const uint32_t col = colbase + threadIdx.x;
        const bool ok = col <= last;  // tail lanes re-read the last column (always in bounds) and do not report

        for (int jb = 0; jb < k; jb += JB) {
            uint4 xb[kRegPtrs ? 1 : JB];
            uint4* x = kRegPtrs ? xpre : xb;
            if constexpr (!kRegPtrs) {
                const uint32_t off = (ok ? col : last) * 16u;
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (K == 0 && jb + q >= k) break;
                    x[q] = gload16<NT>(uniform_ptr(sptr[jb + q]) + off);
                }
            }
            uint32_t TA[kStepWords], TB[kStepWords];
            load_step(lds4 + static_cast<size_t>(jb) * (kStepWords / 4), TA);
#pragma unroll
            for (int q = 0; q < JB; ++q) {
                if (K == 0 && jb + q >= k) break;
                const bool more = q + 1 < JB && (K != 0 || jb + q + 1 < k);
                if (more) load_step(lds4 + static_cast<size_t>(jb + q + 1) * (kStepWords / 4), TB);
                mac_step_rows(acc, x[q], TA, eg);
                step_fence(acc);
#pragma unroll
                for (int w = 0; w < kStepWords; ++w) TA[w] = TB[w];
            }
        }
        const bool again = it + 1 < a.iters && colbase + cstride < ncols16;
        const uint32_t ncol = colbase + cstride + threadIdx.x;
        const uint32_t noff = (ncol <= last ? ncol : last) * 16u;
        if constexpr (kRegPtrs) {
            // Software pipelining: the next iteration's survivor loads go out
            // before this iteration's compare.
            if (again) {
#pragma unroll
                for (int c = 0; c < K; ++c) xpre[c] = gload16<NT>(sp[c] + noff);
            }
        }
        // Bytes at which any row's stored column differs from the recomputed
        // one; tail lanes and bytes past shard_len do not count.
        uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < kRowsPerStep; ++r)
#pragma unroll
            for (int w = 0; w < 4; ++w) d[w] |= acc[r][w];
        const uint32_t nb = ok ? min(16u, shard_len - col * 16u) : 0u;  // bytes of this column below shard_len
        uint32_t byte = 16u;
#pragma unroll
        for (int w = 3; w >= 0; --w) {
            const uint32_t nbw = nb > 4u * w ? min(4u, nb - 4u * w) : 0u;
            const uint32_t dw = d[w] & (nbw >= 4u ? ~0u : (1u << (8u * nbw)) - 1u);
            if (dw) byte = 4u * w + (static_cast<uint32_t>(__builtin_ctz(dw)) >> 3);
        }
        // Lanes are in column order: the first mismatching lane holds the
        // wave's lowest offset.
        const bool bad = byte < 16u;
        const uint64_t bal = __ballot(bad);
        if (bad && (bal & ((1ull << __lane_id()) - 1ull)) == 0) atomicMin(&first_bad[s], col * 16u + byte);
        if (again) load_stored(noff);
    }
}

// Checked repair (rs_kernels.hpp launch_repair): rs_check_kernel and
// rs_read_kernel in one pass over the survivors, a sibling of the check kernel
// with a body of its own.  A job's entries are all m ids of X' (plan_repairs),
// entry t with row t, and entries[..].pad says what becomes of the row:
//   compare  the id is a present shard outside the survivors: its stored
//            column is preloaded into the accumulator and feeds the first_bad
//            reduction, exactly as in the check kernel; nothing is stored;
//   store    the id is erased: the accumulator starts at zero, no load from
//            the slot is ever issued, and the row ends in one 16-byte store
//            per column (tail lanes, which re-read the last column, do not
//            store).
// The store bits of the group's rows are one wave-uniform mask, so every branch
// on them is scalar.  The survivors are never among the entries: a block's
// stores cannot alias anything it or another block reads.
// LDS: [k][20] table dwords | k survivor pointers.
//
// PTRS (compile-time twin, launch_repair_ptrs): as the check kernel's, and the
// table entries of erased shards are loaded too: they are the destinations.
template <int K, int MG, int BT, bool NT, bool PTRS = false, bool VARLEN = false>
__global__ __launch_bounds__(BT) void rs_repair_kernel(std::conditional_t<VARLEN, CheckLensArgs, std::conditional_t<PTRS, CheckPtrArgs, ReadArgs>> a,
                                                       uint32_t* first_bad, uint32_t shard_len) {
    extern __shared__ uint4 lds4[];
    static_assert(MG == kRowsPerStep, "one table sub-step per survivor");
    constexpr bool kRegPtrs = K > 0 && K <= 16;           // survivor bases kept in SGPRs
    constexpr int JB = (K == 0) ? 8 : (K <= 16 ? K : 8);  // survivor loads in flight
    const int k = K ? K : static_cast<int>(a.k);
    uint32_t* tw = reinterpret_cast<uint32_t*>(lds4);
    uint8_t** sptr = reinterpret_cast<uint8_t**>(tw + k * kStepWords);

    static_assert(!VARLEN || PTRS, "per-stripe lengths: the pointer placement only");
    uint32_t grp, chunk, chunks, ncols16;
    uint64_t ji;
    if constexpr (VARLEN) {
        // The job's own column count and shard length (see matmul_block).
        const CombineBlock at = combine_lens_block(a.first_block, a.njobs, a.groups, blockIdx.x);
        ji = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(at.job));
        grp = __builtin_amdgcn_readfirstlane(at.grp);
        chunk = __builtin_amdgcn_readfirstlane(at.chunk);
        chunks = __builtin_amdgcn_readfirstlane(at.chunks);
        ncols16 = __builtin_amdgcn_readfirstlane(a.ncols[ji]);
        shard_len = __builtin_amdgcn_readfirstlane(a.lens[ji]);
    } else {
        uint64_t b = a.xcd ? xcd_block(blockIdx.x, a.xcd, gridDim.x) : blockIdx.x;
        grp = static_cast<uint32_t>(b % a.groups);
        b /= a.groups;
        chunk = static_cast<uint32_t>(b % a.chunks);
        ji = b / a.chunks;
        chunks = a.chunks;
        ncols16 = a.ncols16;
    }
    const ReadJob job = a.jobs[ji];
    // Stripe indices of a repair fit 32 bits (plan_repairs).
    const uint64_t s = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(job.stripe)));
    const int j = __builtin_amdgcn_readfirstlane(job.j);
    const int row0 = static_cast<int>(grp) * MG;
    if (row0 >= j) return;  // whole block: uniform
    const int eg = min(MG, j - row0);
    const ReadEntry* ent = a.entries + static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(job.first)) + row0;
    const uint32_t pat = __builtin_amdgcn_readfirstlane(a.pats[ji]);

    // This lane's coefficient byte for the table build is requested first, so
    // waiting for it later does not wait for the survivor loads behind it.
    // Entry t of a job has row t (plan_repairs): the rows of the group are
    // row0 .. row0 + eg - 1, and the request does not wait for the entry table.
    const uint8_t* coef = a.coef + (static_cast<size_t>(pat) * a.m + row0) * k;
    constexpr bool one_coef = (K > 0 && K * MG <= BT);
    uint32_t cbyte = 0u;
    if constexpr (one_coef) {
        const int c = threadIdx.x / MG, t = threadIdx.x - c * MG;
        if (static_cast<int>(threadIdx.x) < k * MG && t < eg) cbyte = coef[t * k + c];
    }

    const uint32_t* srcid = a.src + static_cast<size_t>(pat) * k;
    uint8_t* sp[kRegPtrs ? K : 1];
    const uint64_t* tp = nullptr;  // pointer mode: the stripe's row of the shard table
    if constexpr (PTRS) {
        tp = a.shard_ptrs + s * (a.k + a.m);
        if constexpr (kRegPtrs) {
            uint32_t ids[K];
#pragma unroll
            for (int c = 0; c < K; ++c) ids[c] = __builtin_amdgcn_readfirstlane(srcid[c]);
#pragma unroll
            for (int c = 0; c < K; ++c) sp[c] = uniform_ptr(reinterpret_cast<uint8_t*>(tp[ids[c]]));
        } else {
            for (int i = threadIdx.x; i < k; i += BT) sptr[i] = reinterpret_cast<uint8_t*>(tp[srcid[i]]);
        }
    } else {
        uint8_t* dbase = const_cast<uint8_t*>(a.data) + s * a.data_ss;
        uint8_t* pbase = const_cast<uint8_t*>(a.parity) + s * a.parity_ss;
        if constexpr (kRegPtrs) {
            uint32_t ids[K];
#pragma unroll
            for (int c = 0; c < K; ++c) ids[c] = __builtin_amdgcn_readfirstlane(srcid[c]);
#pragma unroll
            for (int c = 0; c < K; ++c)
                sp[c] = ids[c] < static_cast<uint32_t>(K) ? dbase + static_cast<uint64_t>(ids[c]) * a.pitch
                                                         : pbase + static_cast<uint64_t>(ids[c] - K) * a.pitch;
        } else {
            for (int i = threadIdx.x; i < k; i += BT) {
                const uint32_t id = srcid[i];
                sptr[i] = id < a.k ? dbase + static_cast<uint64_t>(id) * a.pitch
                                   : pbase + static_cast<uint64_t>(id - a.k) * a.pitch;
            }
        }
    }
    const uint32_t last = ncols16 - 1;
    // Survivor loads of the block's first iteration go out before the table
    // build, as in matmul_block.
    uint4 xpre[kRegPtrs ? K : 1];
    const uint32_t cstride = chunks * BT;
    const uint32_t col0 = chunk * BT + threadIdx.x;
    const uint32_t off0 = (col0 <= last ? col0 : last) * 16u;
    if constexpr (kRegPtrs) {
#pragma unroll
        for (int c = 0; c < K; ++c) xpre[c] = gload16<NT>(sp[c] + off0);
    }
    // Slots of the group's rows and their store bits (bit t: row t is stored);
    // rows past eg have neither.
    uint8_t* dp[MG];
    uint32_t st = 0u;
#pragma unroll
    for (int t = 0; t < MG; ++t)
        if (t < eg) st |= (__builtin_amdgcn_readfirstlane(ent[t].pad) & 1u) << t;
    if constexpr (PTRS) {
        // The entries carry shard ids: all of them first, then their addresses.
        uint32_t oid[MG];
#pragma unroll
        for (int t = 0; t < MG; ++t)
            oid[t] = t < eg ? __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(ent[t].dst)) : 0u;
#pragma unroll
        for (int t = 0; t < MG; ++t) dp[t] = t < eg ? uniform_ptr(reinterpret_cast<uint8_t*>(tp[oid[t]])) : nullptr;
    } else {
#pragma unroll
        for (int t = 0; t < MG; ++t) dp[t] = t < eg ? uniform_ptr(reinterpret_cast<uint8_t*>(ent[t].dst)) : nullptr;
    }
    const uint32_t cmp = ~st & ((1u << eg) - 1u);  // bit t: row t is compared
    // The accumulators of compare rows start as the stored columns, loaded next
    // to the survivors so they ride the same latency; those of store rows and
    // of rows past eg start at zero, and nothing is read from their slots.
    uint32_t acc[kRowsPerStep][4];
    auto load_stored = [&](uint32_t at) {
#pragma unroll
        for (int r = 0; r < kRowsPerStep; ++r) {
            uint4 p = make_uint4(0u, 0u, 0u, 0u);
            if (cmp & (1u << r)) p = gload16<NT>(dp[r] + at);
            acc[r][0] = p.x;
            acc[r][1] = p.y;
            acc[r][2] = p.z;
            acc[r][3] = p.w;
        }
    };
    load_stored(off0);
    // Split tables of the group's rows: survivor c's sub-step holds 4 x 5 dwords.
    if constexpr (one_coef) {
        if (static_cast<int>(threadIdx.x) < k * MG) {
            const int c = threadIdx.x / MG, t = threadIdx.x - c * MG;
            build_tables(cbyte, &tw[c * kStepWords + t * 5]);
        }
    } else {
        for (int idx = threadIdx.x; idx < k * MG; idx += BT) {
            const int c = idx / MG, t = idx - c * MG;
            const uint32_t cf = (t < eg) ? coef[t * k + c] : 0u;
            build_tables(cf, &tw[c * kStepWords + t * 5]);
        }
    }
    __syncthreads();

    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint32_t colbase = chunk * BT + it * cstride;
        if (colbase >= ncols16) break;
        RS_MEM_FENCE();
        const uint32_t col = colbase + threadIdx.x;
        const bool ok = col <= last;  // tail lanes re-read the last column (always in bounds): no report, no store
        const uint32_t off = (ok ? col : last) * 16u;

        for (int jb = 0; jb < k; jb += JB) {
            uint4 xb[kRegPtrs ? 1 : JB];
            uint4* x = kRegPtrs ? xpre : xb;
            if constexpr (!kRegPtrs) {
#pragma unroll
                for (int q = 0; q < JB; ++q) {
                    if (K == 0 && jb + q >= k) break;
                    x[q] = gload16<NT>(uniform_ptr(sptr[jb + q]) + off);
                }
            }
            uint32_t TA[kStepWords], TB[kStepWords];
            load_step(lds4 + static_cast<size_t>(jb) * (kStepWords / 4), TA);
#pragma unroll
            for (int q = 0; q < JB; ++q) {
                if (K == 0 && jb + q >= k) break;
                const bool more = q + 1 < JB && (K != 0 || jb + q + 1 < k);
                if (more) load_step(lds4 + static_cast<size_t>(jb + q + 1) * (kStepWords / 4), TB);
                mac_step_rows(acc, x[q], TA, eg);
                step_fence(acc);
#pragma unroll
                for (int w = 0; w < kStepWords; ++w) TA[w] = TB[w];
            }
        }
        const bool again = it + 1 < a.iters && colbase + cstride < ncols16;
        const uint32_t ncol = colbase + cstride + threadIdx.x;
        const uint32_t noff = (ncol <= last ? ncol : last) * 16u;
        if constexpr (kRegPtrs) {
            // Software pipelining: the next iteration's survivor loads go out
            // before this iteration's stores and compare.
            if (again) {
#pragma unroll
                for (int c = 0; c < K; ++c) xpre[c] = gload16<NT>(sp[c] + noff);
            }
        }
        // Store rows: the regenerated column, once.  Compare rows: the bytes at
        // which the stored column differs from the recomputed one; tail lanes
        // and bytes past shard_len do not count.
        uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < kRowsPerStep; ++r) {
            if (st & (1u << r)) {
                if (ok) gstore16<NT>(dp[r] + off, make_uint4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]));
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w) d[w] |= acc[r][w];
            }
        }
        if (cmp) {  // uniform: a group of store rows has nothing to report
            const uint32_t nb = ok ? min(16u, shard_len - col * 16u) : 0u;  // bytes of this column below shard_len
            uint32_t byte = 16u;
#pragma unroll
            for (int w = 3; w >= 0; --w) {
                const uint32_t nbw = nb > 4u * w ? min(4u, nb - 4u * w) : 0u;
                const uint32_t dw = d[w] & (nbw >= 4u ? ~0u : (1u << (8u * nbw)) - 1u);
                if (dw) byte = 4u * w + (static_cast<uint32_t>(__builtin_ctz(dw)) >> 3);
            }
            // Lanes are in column order: the first mismatching lane holds the
            // wave's lowest offset.
            const bool bad = byte < 16u;
            const uint64_t bal = __ballot(bad);
            if (bad && (bal & ((1ull << __lane_id()) - 1ull)) == 0) atomicMin(&first_bad[s], col * 16u + byte);
        }
        if (again) load_stored(noff);
    }
}

template <int K, int MG, int BT, bool NT>
__global__ __launch_bounds__(BT) void rs_matmul_kernel(MatArgs a) {
    extern __shared__ uint4 lds4[];
    matmul_block<K, MG, BT, NT>(a, blockIdx.x, gridDim.x, lds4);
}

// ------------------------------------------------------------- mailbox --
// One grid per single-message call (rs_kernels.hpp MailboxHost), a group of
// `per_job` blocks per job: the group's blocks poll `posted` over PCIe and
// code their job as soon as it is posted -- while the groups of earlier jobs
// are still reading theirs, so the PCIe reads of consecutive chunks overlap
// instead of each chunk paying the read latency ramp again (a kernel reading
// 256 KiB / 512 KiB / 1 MiB of pinned host memory takes 11 / 17 / 30 us,
// profiles/r06n/pcie_rates.txt).  The last block of a group to finish
// writes done[j - 1].  The call's chunks then cost the host one word each
// instead of a launch and an event, and the grid's dispatch overlaps the
// staging of the first chunk (profiles/r06h/: 4.3 us to launch a chunk,
// 5 us to dispatch it, 5.4 us between two chunks' kernels).  The jobs'
// arguments ride in the kernel arguments: read from the job board in pinned
// memory they cost each group 1.6-3.5 us of PCIe round trips before its
// first survivor load (profiles/r06u/).  Every wave leaves: after its job,
// on quit, or when its job is not posted in time.
__device__ __forceinline__ uint64_t mb_clock() { return __builtin_amdgcn_s_memrealtime(); }

template <int K, int MG, int BT>
__global__ __launch_bounds__(BT) void rs_mailbox_kernel(MailboxHost* h, MailboxDev* d, uint32_t per_job,
                                                        uint64_t timeout, uint32_t stamps, MailboxJobs jobs) {
    extern __shared__ uint4 lds4[];
    __shared__ uint32_t go_s;
    const uint32_t j = blockIdx.x / per_job;  // this block's job, 0-based
    const bool stamper = stamps && threadIdx.x == 0 && blockIdx.x == j * per_job;
    if (stamps && threadIdx.x == 0 && blockIdx.x == 0) d->stamp[0] = mb_clock();
    if (threadIdx.x == 0) {
        uint32_t go = 0;
        const uint64_t since = mb_clock();
        for (;;) {
            if (__hip_atomic_load(&h->posted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) > j) {
                go = 1;
                break;
            }
            if (__hip_atomic_load(&h->quit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) || mb_clock() - since > timeout)
                break;
            __builtin_amdgcn_s_sleep(4);
        }
        go_s = go;
        if (!go)  // the waiting caller launches the job itself at once, not after its own deadline
            __hip_atomic_store(&h->gave_up, uint64_t(1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (stamper) d->stamp[1 + 3 * j] = mb_clock();
    }
    __syncthreads();
    if (go_s) {
        // Job j's inputs (and a decode's pattern table) are in host memory
        // the host wrote before posting it: nothing cached from earlier may
        // be used.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        if (stamper) d->stamp[2 + 3 * j] = mb_clock();
        const MailboxJob& job = jobs.job[j];
        const uint32_t nblk = job.blocks;
        for (uint32_t lb = blockIdx.x - j * per_job; lb < nblk; lb += per_job) {
            matmul_block<K, MG, BT, true>(job.a, lb, nblk, lds4);
            __syncthreads();  // the next logical block rebuilds the LDS tables
        }
        // This wave's outputs reach host memory before the block reports.
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __syncthreads();
        if (threadIdx.x == 0 &&
            __hip_atomic_fetch_add(&d->arrive[j], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == per_job) {
            if (stamps) d->stamp[3 + 3 * j] = mb_clock();
            __hip_atomic_store(&h->done[j], static_cast<uint64_t>(j + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    // The last block out zeroes the device counters for the next launch on
    // this stream (kernel boundaries order the two).
    if (threadIdx.x == 0 &&
        __hip_atomic_fetch_add(&d->left, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1 == gridDim.x) {
        for (int i = 0; i < kMailboxJobs; ++i)
            __hip_atomic_store(&d->arrive[i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&d->left, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct MailboxVariant {
    int K, MG;
    void (*fn)(MailboxHost*, MailboxDev*, uint32_t, uint64_t, uint32_t, MailboxJobs);  // (h, d, per_job, timeout, stamps, jobs)
};
const MailboxVariant kMailbox[] = {
    {10, 4, rs_mailbox_kernel<10, 4, 256>},  // RS(10,4): BASELINE config 1
    {4, 4, rs_mailbox_kernel<4, 4, 256>},    // RS(4,2): the plugin default (main.go:34-35)
};
const MailboxVariant* mailbox_variant(int k, int rows) {
    for (const MailboxVariant& v : kMailbox)
        if (v.K == k && rows >= 1 && rows <= v.MG) return &v;
    return nullptr;
}

__global__ __launch_bounds__(kBlock) void fill_splitmix_kernel(uint8_t* p, size_t len,
                                                               uint64_t seed) {
    const size_t nq = len / 8;
    const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
    for (size_t q = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; q <= nq; q += stride) {
        uint64_t z = seed + (q + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        if (q < nq) {
            reinterpret_cast<uint64_t*>(p)[q] = z;
        } else {
            for (size_t i = nq * 8; i < len; ++i) p[i] = static_cast<uint8_t>(z >> (8 * (i - nq * 8)));
        }
    }
}

struct Variant {
    int K, MG, BT;
    bool nt;
    const char* name;
    void (*fn)(MatArgs);
};

#define RS_VARIANT(K, MG, BT) {K, MG, BT, true, "K" #K "_MG" #MG "_B" #BT, rs_matmul_kernel<K, MG, BT, true>}
#define RS_VARIANT_T(K, MG, BT) {K, MG, BT, false, "K" #K "_MG" #MG "_B" #BT "_T", rs_matmul_kernel<K, MG, BT, false>}
// Specialised variants for the configurations the plugin and BASELINE use,
// then runtime-k fall-backs (k up to 256).
const Variant kVariants[] = {
    RS_VARIANT(10, 4, 256),   // RS(10,4): BASELINE configs 1-4
    RS_VARIANT(4, 4, 256),    // RS(4,2): plugin default (main.go:34-35)
    RS_VARIANT(8, 4, 256),    // infectious example RS(8,14): reconstructs of <= 4 erasures
    RS_VARIANT(8, 6, 256),    // ... its encode (6 rows: no padded rows' products)
    RS_VARIANT(8, 8, 256),
    RS_VARIANT(64, 4, 256),   // RS(64,16) reconstructs of <= 4 erasures (fewer VGPRs, smaller tables)
    RS_VARIANT(64, 8, 256),   // ... and <= 8
    RS_VARIANT(64, 16, 256),  // RS(64,16): BASELINE config 5
    RS_VARIANT(0, 4, 256),
    RS_VARIANT(0, 8, 256),
    // Temporal-policy twin of the headline variant, for A/B (RSMI_NT=0).
    RS_VARIANT_T(10, 4, 256),
    // 512/1024-thread blocks measured 3-13% slower for RS(10,4) on one box
    // (profiles/r01_ab_block.log); RSMI_BLOCK selects among compiled sizes.
};
#undef RS_VARIANT
#undef RS_VARIANT_T

// The variant for a launch coding up to `rows` output rows per stripe: the
// first specialised one for k whose row group holds them all (smaller row
// groups are listed first), else row groups of the runtime-k kernels.
const Variant& pick(int k, int rows) {
    static const int want_bt = [] {
        const char* e = std::getenv("RSMI_BLOCK");  // tuning knob
        return e ? std::atoi(e) : 256;
    }();
    static const bool want_nt = [] {
        const char* e = std::getenv("RSMI_NT");  // tuning knob (default 1: non-temporal)
        return e ? std::atoi(e) != 0 : true;
    }();
    for (const Variant& v : kVariants)
        if (v.K != 0 && v.K == k && rows <= v.MG && v.BT == want_bt && v.nt == want_nt) return v;
    for (const Variant& v : kVariants)
        if (v.K != 0 && v.K == k && rows <= v.MG && v.BT == want_bt) return v;
    for (const Variant& v : kVariants)
        if (v.K != 0 && v.K == k && rows <= v.MG) return v;
    for (const Variant& v : kVariants)
        if (v.K == 64 && k == 64 && v.MG == 16) return v;  // RS(64, m > 16): row groups of 16
    const int want_mg = rows <= 4 ? 4 : 8;  // runtime-k fall-backs
    for (const Variant& v : kVariants)
        if (v.K == 0 && v.MG == want_mg) return v;
    return kVariants[0];  // unreachable: both runtime-k variants are listed
}

// Verify twins of the variants that serve an encode; every other (k, m)
// goes through row groups of the runtime-k ones.
struct VerifyVariant {
    int K, MG;
    const char* name;
    void (*fn)(MatArgs, uint32_t*, uint32_t);
    const char* lens_name;  // the per-stripe-length twin (pointer mode)
    void (*lens_fn)(MatArgs, uint32_t*, ScrubLensTables);
};
#define RS_VERIFY(K, MG)                                                                                         \
    {K, MG, "verify_K" #K "_MG" #MG "_B256", rs_verify_kernel<K, MG, kBlock, true>, "verify_K" #K "_MG" #MG "_B256_lens", \
     rs_verify_lens_kernel<K, MG, kBlock, true>}
const VerifyVariant kVerify[] = {
    RS_VERIFY(10, 4), RS_VERIFY(4, 4), RS_VERIFY(8, 6), RS_VERIFY(64, 16), RS_VERIFY(0, 4), RS_VERIFY(0, 8),
};
#undef RS_VERIFY

const VerifyVariant& pick_verify(int k, int rows) {
    for (const VerifyVariant& v : kVerify)
        if (v.K != 0 && v.K == k && (rows <= v.MG || k == 64)) return v;  // RS(64, m > 16): row groups of 16
    return kVerify[rows <= 4 ? 4 : 5];
}

// Update variants: the smallest row group that holds all m rows commits the
// data in-kernel; m > 16 goes through row groups of 16.
struct UpdateVariant {
    int MG;
    const char* name;
    void (*fn)(UpdArgs);
    const char* ptrs_name;  // the pointer-mode twin
    void (*ptrs_fn)(UpdPtrArgs);
};
#define RS_UPDATE(MG)                                                                       \
    {MG, "update_MG" #MG "_B256", rs_update_kernel<MG, kBlock, true>, "update_MG" #MG "_B256_ptrs", \
     rs_update_kernel<MG, kBlock, true, true>}
const UpdateVariant kUpdate[] = {RS_UPDATE(4), RS_UPDATE(8), RS_UPDATE(16)};
#undef RS_UPDATE

constexpr size_t kUpdateLdsMax = 64 * 1024;
size_t update_lds(int mg, uint32_t max_j) {
    return static_cast<size_t>(max_j) * (mg / kRowsPerStep) * kStepWords * 4 + 2 * static_cast<size_t>(max_j) * sizeof(void*);
}

// max_j = 0: the variant named for m.  A job of more than 195 shards does not
// fit the LDS with row groups of 16; it takes row groups of 8.
const UpdateVariant& pick_update(int m, uint32_t max_j) {
    const UpdateVariant& v = kUpdate[m <= 4 ? 0 : m <= 8 ? 1 : 2];
    return update_lds(v.MG, max_j) <= kUpdateLdsMax ? v : kUpdate[1];
}

// Degraded-update variants: the update kernel's row groups over the present
// parity rows.
struct DegVariant {
    int MG;
    const char* name;
    void (*fn)(DegArgs);
};
#define RS_UPDATE_DEG(MG) {MG, "update_degraded_MG" #MG "_B256", rs_update_degraded_kernel<MG, kBlock, true>}
const DegVariant kUpdateDeg[] = {RS_UPDATE_DEG(4), RS_UPDATE_DEG(8), RS_UPDATE_DEG(16)};
#undef RS_UPDATE_DEG

// Per source: its table sub-steps and three addresses.
size_t update_degraded_lds(int mg, uint32_t max_src) {
    return static_cast<size_t>(max_src) * (mg / kRowsPerStep) * kStepWords * 4 + 3 * static_cast<size_t>(max_src) * sizeof(void*);
}

const DegVariant& pick_update_degraded(int m) { return kUpdateDeg[m <= 4 ? 0 : m <= 8 ? 1 : 2]; }

// Combine variants: the update kernel's row groups, chosen from the call's
// largest nout, so that a job of up to 16 outputs reads its sources once.
struct CombineVariant {
    int MG;
    const char* name;
    void (*fn)(CombArgs);
};
#define RS_COMBINE(MG) {MG, "combine_MG" #MG "_B256", rs_combine_kernel<MG, kBlock, true>}
const CombineVariant kCombine[] = {RS_COMBINE(4), RS_COMBINE(8), RS_COMBINE(16)};
#undef RS_COMBINE

// Their per-job-length twins (rs_combine_lens), same row groups.
struct CombineLensVariant {
    int MG;
    const char* name;
    void (*fn)(CombLensArgs);
};
#define RS_COMBINE_LENS(MG) {MG, "combine_lens_MG" #MG "_B256", rs_combine_kernel<MG, kBlock, true, true>}
const CombineLensVariant kCombineLens[] = {RS_COMBINE_LENS(4), RS_COMBINE_LENS(8), RS_COMBINE_LENS(16)};
#undef RS_COMBINE_LENS
static_assert(kCombineBlockCols == kBlock, "the block map's columns per block are the kernel's lanes");

size_t combine_lds(int mg, uint32_t max_nsrc) {
    return static_cast<size_t>(max_nsrc) * (mg / kRowsPerStep) * kStepWords * 4 + static_cast<size_t>(max_nsrc) * sizeof(void*);
}

// A job of more than 199 sources does not fit the LDS with row groups of 16
// (328 bytes per source); it takes row groups of 8.
const CombineVariant& pick_combine(uint32_t max_nsrc, uint32_t max_nout) {
    const CombineVariant& v = kCombine[max_nout <= 4 ? 0 : max_nout <= 8 ? 1 : 2];
    return combine_lds(v.MG, max_nsrc) <= kUpdateLdsMax ? v : kCombine[1];
}

// Read variants: always the split-table kernel with row groups of 4 wanted
// rows, also for the codes whose reconstruct runs the syndrome network.
struct ReadVariant {
    int K;
    const char* name;
    void (*fn)(ReadArgs);
    const char* ptrs_name;  // the pointer-mode twin
    void (*ptrs_fn)(ReadPtrArgs);
};
#define RS_READ(K)                                                                                 \
    {K, "read_K" #K "_MG4_B256", rs_read_kernel<K, 4, kBlock, true>, "read_K" #K "_MG4_B256_ptrs", \
     rs_read_kernel<K, 4, kBlock, true, true>}
const ReadVariant kRead[] = {RS_READ(10), RS_READ(4), RS_READ(8), RS_READ(64), RS_READ(0)};
#undef RS_READ
constexpr int kReadMG = 4;

const ReadVariant& pick_read(int k) {
    for (const ReadVariant& v : kRead)
        if (v.K == k) return v;
    return kRead[sizeof(kRead) / sizeof(kRead[0]) - 1];  // runtime k
}

// Check variants: the read kernel's instances, one twin each.
struct CheckVariant {
    int K;
    const char* name;
    void (*fn)(ReadArgs, uint32_t*, uint32_t);
    const char* ptrs_name;  // the pointer-mode twin
    void (*ptrs_fn)(CheckPtrArgs, uint32_t*, uint32_t);
    const char* lens_name;  // ... and its per-stripe-length twin
    void (*lens_fn)(CheckLensArgs, uint32_t*, uint32_t);
};
#define RS_CHECK(K)                                                                                    \
    {K, "check_K" #K "_MG4_B256", rs_check_kernel<K, 4, kBlock, true>, "check_K" #K "_MG4_B256_ptrs", \
     rs_check_kernel<K, 4, kBlock, true, true>, "check_K" #K "_MG4_B256_ptrs_lens",                      \
     rs_check_kernel<K, 4, kBlock, true, true, true>}
const CheckVariant kCheck[] = {RS_CHECK(10), RS_CHECK(4), RS_CHECK(8), RS_CHECK(64), RS_CHECK(0)};
#undef RS_CHECK

const CheckVariant& pick_check(int k) {
    for (const CheckVariant& v : kCheck)
        if (v.K == k) return v;
    return kCheck[sizeof(kCheck) / sizeof(kCheck[0]) - 1];  // runtime k
}

// Repair variants: the check kernel's instances, one sibling each.
struct RepairVariant {
    int K;
    const char* name;
    void (*fn)(ReadArgs, uint32_t*, uint32_t);
    const char* ptrs_name;  // the pointer-mode twin
    void (*ptrs_fn)(CheckPtrArgs, uint32_t*, uint32_t);
    const char* lens_name;  // ... and its per-stripe-length twin
    void (*lens_fn)(CheckLensArgs, uint32_t*, uint32_t);
};
#define RS_REPAIR(K)                                                                                      \
    {K, "repair_K" #K "_MG4_B256", rs_repair_kernel<K, 4, kBlock, true>, "repair_K" #K "_MG4_B256_ptrs", \
     rs_repair_kernel<K, 4, kBlock, true, true>, "repair_K" #K "_MG4_B256_ptrs_lens",                      \
     rs_repair_kernel<K, 4, kBlock, true, true, true>}
const RepairVariant kRepair[] = {RS_REPAIR(10), RS_REPAIR(4), RS_REPAIR(8), RS_REPAIR(64), RS_REPAIR(0)};
#undef RS_REPAIR

const RepairVariant& pick_repair(int k) {
    for (const RepairVariant& v : kRepair)
        if (v.K == k) return v;
    return kRepair[sizeof(kRepair) / sizeof(kRepair[0]) - 1];  // runtime k
}

}  // namespace

const char* update_variant_name(int m) { return pick_update(m, 0).name; }

const char* update_ptrs_variant_name(int m) { return pick_update(m, 0).ptrs_name; }

const char* read_variant_name(int k) { return pick_read(k).name; }

const char* read_ptrs_variant_name(int k) { return pick_read(k).ptrs_name; }

const char* check_variant_name(int k) { return pick_check(k).name; }

const char* check_ptrs_variant_name(int k) { return pick_check(k).ptrs_name; }

const char* check_lens_variant_name(int k) { return pick_check(k).lens_name; }

hipError_t launch_check_lens(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad,
                          const ScrubLensTables& t, uint32_t blocks, hipStream_t stream) {
    if (a.njobs == 0 || blocks == 0) return hipSuccess;
    if (!shard_ptrs || !t.first_block || !t.ncols || !t.lens || t.njobs != a.njobs) return hipErrorInvalidValue;
    if (a.groups == 0 || a.iters == 0 || blocks > 0x7FFFFFFFu) return hipErrorInvalidConfiguration;
    const CheckVariant& v = pick_check(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    CheckLensArgs la{};
    static_cast<ReadArgs&>(la) = a;
    la.ncols16 = 0;
    la.chunks = 0;
    la.xcd = 0;  // natural block order
    la.shard_ptrs = shard_ptrs;
    la.first_block = t.first_block;
    la.ncols = t.ncols;
    la.lens = t.lens;
    hipLaunchKernelGGL(v.lens_fn, dim3(blocks), dim3(kBlock), lds, stream, la, first_bad, 0u);
    return hipGetLastError();
}

hipError_t launch_check(const ReadArgs& a, uint32_t* first_bad, uint32_t shard_len, hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.groups == 0) return hipSuccess;
    const CheckVariant& v = pick_check(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(v.fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, a, first_bad, shard_len);
    return hipGetLastError();
}

hipError_t launch_check_ptrs(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad, uint32_t shard_len,
                             hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.groups == 0) return hipSuccess;
    if (!shard_ptrs) return hipErrorInvalidValue;
    const CheckVariant& v = pick_check(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    CheckPtrArgs pa{};
    static_cast<ReadArgs&>(pa) = a;
    pa.shard_ptrs = shard_ptrs;
    hipLaunchKernelGGL(v.ptrs_fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, pa, first_bad,
                       shard_len);
    return hipGetLastError();
}

const char* repair_variant_name(int k) { return pick_repair(k).name; }

const char* repair_ptrs_variant_name(int k) { return pick_repair(k).ptrs_name; }

const char* repair_lens_variant_name(int k) { return pick_repair(k).lens_name; }

hipError_t launch_repair_lens(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad,
                           const ScrubLensTables& t, uint32_t blocks, hipStream_t stream) {
    if (a.njobs == 0 || blocks == 0) return hipSuccess;
    if (!shard_ptrs || !t.first_block || !t.ncols || !t.lens || t.njobs != a.njobs) return hipErrorInvalidValue;
    if (a.groups == 0 || a.iters == 0 || blocks > 0x7FFFFFFFu) return hipErrorInvalidConfiguration;
    const RepairVariant& v = pick_repair(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    CheckLensArgs la{};
    static_cast<ReadArgs&>(la) = a;
    la.ncols16 = 0;
    la.chunks = 0;
    la.xcd = 0;  // natural block order
    la.shard_ptrs = shard_ptrs;
    la.first_block = t.first_block;
    la.ncols = t.ncols;
    la.lens = t.lens;
    hipLaunchKernelGGL(v.lens_fn, dim3(blocks), dim3(kBlock), lds, stream, la, first_bad, 0u);
    return hipGetLastError();
}

hipError_t launch_repair(const ReadArgs& a, uint32_t* first_bad, uint32_t shard_len, hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.groups == 0) return hipSuccess;
    const RepairVariant& v = pick_repair(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    // Unreachable behind plan_read, which refuses such a grid before the call
    // has queued anything; kept as launch_check keeps it.
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(v.fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, a, first_bad, shard_len);
    return hipGetLastError();
}

hipError_t launch_repair_ptrs(const ReadArgs& a, const uint64_t* shard_ptrs, uint32_t* first_bad, uint32_t shard_len,
                              hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.groups == 0) return hipSuccess;
    if (!shard_ptrs) return hipErrorInvalidValue;
    const RepairVariant& v = pick_repair(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    CheckPtrArgs pa{};
    static_cast<ReadArgs&>(pa) = a;
    pa.shard_ptrs = shard_ptrs;
    hipLaunchKernelGGL(v.ptrs_fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, pa, first_bad,
                       shard_len);
    return hipGetLastError();
}

bool plan_read(ReadArgs* a, uint32_t max_j) {
    const uint32_t total_it = (a->ncols16 + kBlock - 1) / kBlock;
    static const uint32_t iters_cap = [] {
        const char* e = std::getenv("RSMI_ITERS");  // tuning knob, as launch_matmul
        const int v = e ? std::atoi(e) : 1;
        return static_cast<uint32_t>(v > 0 ? v : 1);
    }();
    a->iters = std::min<uint32_t>(iters_cap, std::max<uint32_t>(total_it, 1));
    a->chunks = (total_it + a->iters - 1) / a->iters;
    a->groups = (max_j + kReadMG - 1) / kReadMG;
    const uint64_t blocks = static_cast<uint64_t>(a->njobs) * a->chunks * a->groups;
    if (blocks > 0x7FFFFFFFull) return false;
    if (a->xcd == ~0u) a->xcd = a->chunks * a->groups;  // a job per XCD region
    return true;
}

hipError_t launch_read(const ReadArgs& a, hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.groups == 0) return hipSuccess;
    const ReadVariant& v = pick_read(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(v.fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_read_ptrs(const ReadArgs& a, const uint64_t* shard_ptrs, uint64_t shard_off, hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.groups == 0) return hipSuccess;
    if (!shard_ptrs || (shard_off & 15u)) return hipErrorInvalidValue;
    const ReadVariant& v = pick_read(static_cast<int>(a.k));
    const size_t lds = static_cast<size_t>(a.k) * kStepWords * 4 + a.k * sizeof(void*);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    ReadPtrArgs pa{};
    static_cast<ReadArgs&>(pa) = a;
    pa.shard_ptrs = shard_ptrs;
    pa.shard_off = shard_off;
    hipLaunchKernelGGL(v.ptrs_fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, pa);
    return hipGetLastError();
}

bool plan_update(UpdArgs* a, uint32_t max_j) {
    const UpdateVariant& v = pick_update(static_cast<int>(a->m), max_j);
    const uint32_t total_it = (a->ncols16 + kBlock - 1) / kBlock;
    static const uint32_t iters_cap = [] {
        const char* e = std::getenv("RSMI_ITERS");  // tuning knob, as launch_matmul
        const int v = e ? std::atoi(e) : 1;
        return static_cast<uint32_t>(v > 0 ? v : 1);
    }();
    a->iters = std::min<uint32_t>(iters_cap, std::max<uint32_t>(total_it, 1));
    a->chunks = (total_it + a->iters - 1) / a->iters;
    a->mg = static_cast<uint32_t>(v.MG);
    a->groups = (a->m + a->mg - 1) / a->mg;
    a->commit = a->groups == 1;
    const uint64_t blocks = static_cast<uint64_t>(a->njobs) * a->chunks * a->groups;
    if (blocks > 0x7FFFFFFFull) return false;
    if (a->xcd == ~0u) a->xcd = a->chunks * a->groups;  // a stripe per XCD region
    return true;
}

hipError_t launch_update(const UpdArgs& a, uint32_t max_j, hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.m == 0 || max_j == 0) return hipSuccess;
    const UpdateVariant* v = nullptr;
    for (const UpdateVariant& u : kUpdate)
        if (static_cast<uint32_t>(u.MG) == a.mg) v = &u;
    const size_t lds = update_lds(static_cast<int>(a.mg), max_j);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (!v || lds > kUpdateLdsMax || blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(v->fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_update_ptrs(const UpdArgs& a, const uint64_t* shard_ptrs, uint64_t shard_off, uint32_t max_j,
                              hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.m == 0 || max_j == 0) return hipSuccess;
    if (!shard_ptrs || (shard_off & 15u)) return hipErrorInvalidValue;
    const UpdateVariant* v = nullptr;
    for (const UpdateVariant& u : kUpdate)
        if (static_cast<uint32_t>(u.MG) == a.mg) v = &u;
    const size_t lds = update_lds(static_cast<int>(a.mg), max_j);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (!v || lds > kUpdateLdsMax || blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    UpdPtrArgs pa{};
    static_cast<UpdArgs&>(pa) = a;
    pa.shard_ptrs = shard_ptrs;
    pa.shard_off = shard_off;
    hipLaunchKernelGGL(v->ptrs_fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, pa);
    return hipGetLastError();
}

const char* update_degraded_variant_name(int m) { return pick_update_degraded(m).name; }

bool update_degraded_fused(int m, uint32_t max_src) {
    return m <= 16 && update_degraded_lds(pick_update_degraded(m).MG, max_src) <= kUpdateLdsMax;
}

bool plan_update_degraded_launch(DegArgs* a, uint32_t max_src, bool fused) {
    const DegVariant* v = &pick_update_degraded(static_cast<int>(a->m));
    // Pair form only: a job too wide for the LDS with row groups of 16 takes
    // row groups of 8, as the update kernel's.
    if (!fused && update_degraded_lds(v->MG, max_src) > kUpdateLdsMax) v = &kUpdateDeg[1];
    const uint32_t total_it = (a->ncols16 + kBlock - 1) / kBlock;
    static const uint32_t iters_cap = [] {
        const char* e = std::getenv("RSMI_ITERS");  // tuning knob, as launch_matmul
        const int v = e ? std::atoi(e) : 1;
        return static_cast<uint32_t>(v > 0 ? v : 1);
    }();
    a->iters = std::min<uint32_t>(iters_cap, std::max<uint32_t>(total_it, 1));
    a->chunks = (total_it + a->iters - 1) / a->iters;
    a->mg = static_cast<uint32_t>(v->MG);
    a->groups = fused ? 1u : std::max<uint32_t>(1u, (a->m + a->mg - 1) / a->mg);
    a->commit = fused ? 1u : 0u;
    const uint64_t blocks = static_cast<uint64_t>(a->njobs) * a->chunks * a->groups;
    if (blocks > 0x7FFFFFFFull) return false;
    if (a->xcd == ~0u) a->xcd = a->chunks * a->groups;  // a stripe per XCD region
    return true;
}

hipError_t launch_update_degraded(const DegArgs& a, uint32_t max_src, hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || max_src == 0) return hipSuccess;
    const DegVariant* v = nullptr;
    for (const DegVariant& u : kUpdateDeg)
        if (static_cast<uint32_t>(u.MG) == a.mg) v = &u;
    const size_t lds = update_degraded_lds(static_cast<int>(a.mg), max_src);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (!v || lds > kUpdateLdsMax || blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (a.commit && a.groups != 1) return hipErrorInvalidConfiguration;  // in place: one block per column
    hipLaunchKernelGGL(v->fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, a);
    return hipGetLastError();
}

const char* combine_variant_name(int nsrc, int nout) {
    return pick_combine(static_cast<uint32_t>(nsrc), static_cast<uint32_t>(nout)).name;
}

bool plan_combine_launch(CombArgs* a, uint32_t max_nsrc, uint32_t max_nout) {
    const CombineVariant& v = pick_combine(max_nsrc, max_nout);
    const uint32_t total_it = (a->ncols16 + kBlock - 1) / kBlock;
    static const uint32_t iters_cap = [] {
        const char* e = std::getenv("RSMI_ITERS");  // tuning knob, as launch_matmul
        const int v = e ? std::atoi(e) : 1;
        return static_cast<uint32_t>(v > 0 ? v : 1);
    }();
    a->iters = std::min<uint32_t>(iters_cap, std::max<uint32_t>(total_it, 1));
    a->chunks = (total_it + a->iters - 1) / a->iters;
    a->mg = static_cast<uint32_t>(v.MG);
    a->groups = (max_nout + a->mg - 1) / a->mg;
    const uint64_t blocks = static_cast<uint64_t>(a->njobs) * a->chunks * a->groups;
    if (blocks > 0x7FFFFFFFull) return false;
    if (a->xcd == ~0u) a->xcd = a->chunks * a->groups;  // a job per XCD region
    return true;
}

hipError_t launch_combine(const CombArgs& a, uint32_t max_nsrc, hipStream_t stream) {
    if (a.njobs == 0 || a.ncols16 == 0 || a.groups == 0 || max_nsrc == 0) return hipSuccess;
    const CombineVariant* v = nullptr;
    for (const CombineVariant& u : kCombine)
        if (static_cast<uint32_t>(u.MG) == a.mg) v = &u;
    const size_t lds = combine_lds(static_cast<int>(a.mg), max_nsrc);
    const uint64_t blocks = static_cast<uint64_t>(a.njobs) * a.chunks * a.groups;
    if (!v || lds > kUpdateLdsMax || blocks == 0 || blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(v->fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, a);
    return hipGetLastError();
}

uint32_t combine_iters_cap() {
    static const uint32_t cap = [] {
        const char* e = std::getenv("RSMI_ITERS");  // tuning knob, as launch_matmul
        const int v = e ? std::atoi(e) : 1;
        return static_cast<uint32_t>(v > 0 ? v : 1);
    }();
    return cap;
}

const char* combine_lens_variant_name(int nsrc, int nout) {
    const int mg = pick_combine(static_cast<uint32_t>(nsrc), static_cast<uint32_t>(nout)).MG;
    for (const CombineLensVariant& u : kCombineLens)
        if (u.MG == mg) return u.name;
    return "";
}

bool plan_combine_lens_launch(CombLensArgs* a, const CombinePlan& plan) {
    // The planner's row groups (combine_row_group) are pick_combine's.
    if (plan.jobs.empty() || static_cast<int>(plan.mg) != pick_combine(plan.max_nsrc, plan.max_nout).MG) return false;
    if (plan.first_block.size() != plan.jobs.size() + 1 || plan.ncols.size() != plan.jobs.size()) return false;
    a->njobs = static_cast<uint32_t>(plan.jobs.size());
    a->ncols16 = 0;
    a->chunks = 0;
    a->xcd = 0;  // natural block order
    a->mg = plan.mg;
    a->groups = plan.groups;
    a->iters = plan.iters;
    return true;
}

hipError_t launch_combine_lens(const CombLensArgs& a, uint32_t max_nsrc, uint32_t blocks, hipStream_t stream) {
    if (a.njobs == 0 || blocks == 0 || max_nsrc == 0) return hipSuccess;
    const CombineLensVariant* v = nullptr;
    for (const CombineLensVariant& u : kCombineLens)
        if (static_cast<uint32_t>(u.MG) == a.mg) v = &u;
    const size_t lds = combine_lds(static_cast<int>(a.mg), max_nsrc);
    if (!v || lds > kUpdateLdsMax || a.groups == 0 || a.iters == 0 || blocks > 0x7FFFFFFFu) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(v->fn, dim3(blocks), dim3(kBlock), lds, stream, a);
    return hipGetLastError();
}

const char* variant_name(int k, int rows) { return pick(k, rows).name; }

const char* verify_variant_name(int k, int rows) { return pick_verify(k, rows).name; }

bool mailbox_supported(int k, int rows) { return mailbox_variant(k, rows) != nullptr; }

void plan_mailbox_job(const MatArgs& a, int max_e, MailboxJob* job) {
    const MailboxVariant* v = mailbox_variant(static_cast<int>(a.k), max_e);
    const int mg = v ? v->MG : 4;
    job->a = a;
    job->a.iters = 1;
    job->a.chunks = (a.ncols16 + kBlock - 1) / kBlock;
    job->a.groups = static_cast<uint32_t>((max_e + mg - 1) / mg);
    job->a.xcd = 0;  // the logical blocks are dealt over the grid's blocks anyway
    job->blocks = static_cast<uint32_t>(a.stripes * job->a.chunks * job->a.groups);
}

hipError_t launch_mailbox(MailboxHost* h, MailboxDev* d, const MailboxJobs& jobs, int njobs, int k, int rows,
                          uint32_t per_job, uint64_t timeout, hipStream_t stream, bool stamps) {
    const MailboxVariant* v = mailbox_variant(k, rows);
    if (!v || per_job == 0 || njobs < 1 || njobs > kMailboxJobs) return hipErrorInvalidValue;
    const size_t lds = static_cast<size_t>(k) * ((v->MG + 3) / 4) * kStepWords * 4 + k * sizeof(void*);
    hipLaunchKernelGGL(v->fn, dim3(per_job * static_cast<uint32_t>(njobs)), dim3(kBlock), lds, stream, h, d, per_job,
                       timeout, static_cast<uint32_t>(stamps), jobs);
    return hipGetLastError();
}

namespace {
// The launch plan of variant v for a (stripes, ncols16 set) coding up to max_e
// rows per stripe: fills in iters, chunks and groups; the grid's blocks.
uint64_t plan_matmul(MatArgs* a, const Variant& v, int max_e) {
    const uint32_t total_it = (a->ncols16 + v.BT - 1) / v.BT;
    static const uint32_t iters_cap = [] {
        const char* e = std::getenv("RSMI_ITERS");  // tuning knob (default 1: one 4 KiB column chunk per block)
        const int v = e ? std::atoi(e) : 1;
        return static_cast<uint32_t>(v > 0 ? v : 1);
    }();
    a->iters = std::min<uint32_t>(iters_cap, total_it);
    a->chunks = (total_it + a->iters - 1) / a->iters;
    a->groups = static_cast<uint32_t>((max_e + v.MG - 1) / v.MG);
    return a->stripes * a->chunks * a->groups;
}
}  // namespace

hipError_t launch_matmul(MatArgs a, int max_e, hipStream_t stream) {
    if (a.stripes == 0 || a.ncols16 == 0 || max_e <= 0) return hipSuccess;
    const Variant& v = pick(static_cast<int>(a.k), max_e);
    const uint64_t blocks = plan_matmul(&a, v, max_e);
    size_t lds = static_cast<size_t>(a.k) * ((v.MG + 3) / 4) * kStepWords * 4 + a.k * sizeof(void*);
    static const size_t lds_floor = [] {
        const char* e = std::getenv("RSMI_LDS_PAD_KB");  // A/B knob: LDS per block >= this (caps occupancy)
        const int kb = e ? std::atoi(e) : 0;
        return static_cast<size_t>(kb > 0 && kb <= 64 ? kb : 0) * 1024;
    }();
    lds = std::max(lds, lds_floor);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (a.xcd == ~0u) a.xcd = a.chunks * a.groups;  // a stripe per XCD region
    hipLaunchKernelGGL(v.fn, dim3(static_cast<uint32_t>(blocks)), dim3(v.BT), lds, stream, a);
    return hipGetLastError();
}

uint64_t matmul_blocks(int k, int max_e, uint32_t ncols16, uint64_t stripes) {
    if (stripes == 0 || ncols16 == 0 || max_e <= 0) return 0;
    MatArgs a{};
    a.stripes = stripes;  // < 2^32, chunks <= 2^20, groups <= 64: no overflow
    a.ncols16 = ncols16;
    return plan_matmul(&a, pick(k, max_e), max_e);
}

hipError_t launch_verify(MatArgs a, uint32_t* first_bad, uint32_t shard_len, hipStream_t stream) {
    if (a.stripes == 0 || a.ncols16 == 0 || a.m == 0) return hipSuccess;
    const VerifyVariant& v = pick_verify(static_cast<int>(a.k), static_cast<int>(a.m));
    const uint32_t total_it = (a.ncols16 + kBlock - 1) / kBlock;
    static const uint32_t iters_cap = [] {
        const char* e = std::getenv("RSMI_ITERS");  // tuning knob, as launch_matmul
        const int v = e ? std::atoi(e) : 1;
        return static_cast<uint32_t>(v > 0 ? v : 1);
    }();
    a.iters = std::min<uint32_t>(iters_cap, total_it);
    a.chunks = (total_it + a.iters - 1) / a.iters;
    a.groups = (a.m + v.MG - 1) / v.MG;
    const size_t lds = static_cast<size_t>(a.k) * ((v.MG + 3) / 4) * kStepWords * 4 + a.k * sizeof(void*);
    const uint64_t blocks = a.stripes * a.chunks * a.groups;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidConfiguration;
    if (a.xcd == ~0u) a.xcd = a.chunks * a.groups;
    hipLaunchKernelGGL(v.fn, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), lds, stream, a, first_bad, shard_len);
    return hipGetLastError();
}

uint32_t verify_row_groups(int k, int m) {
    if (m <= 0) return 0;
    const int mg = pick_verify(k, m).MG;
    return static_cast<uint32_t>((m + mg - 1) / mg);
}

const char* verify_lens_variant_name(int k, int rows) { return pick_verify(k, rows).lens_name; }

hipError_t launch_verify_lens(MatArgs a, uint32_t* first_bad, const ScrubLensTables& t, uint32_t blocks,
                              hipStream_t stream) {
    if (t.njobs == 0 || blocks == 0 || a.m == 0) return hipSuccess;
    if (!a.shard_ptrs || !a.stripe_desc || !t.first_block || !t.ncols || !t.lens) return hipErrorInvalidValue;
    if (a.iters == 0 || blocks > 0x7FFFFFFFu) return hipErrorInvalidConfiguration;
    const VerifyVariant& v = pick_verify(static_cast<int>(a.k), static_cast<int>(a.m));
    a.stripes = t.njobs;
    a.ncols16 = 0;
    a.chunks = 0;
    a.xcd = 0;  // natural block order
    a.groups = (a.m + v.MG - 1) / v.MG;
    const size_t lds = static_cast<size_t>(a.k) * ((v.MG + 3) / 4) * kStepWords * 4 + a.k * sizeof(void*);
    hipLaunchKernelGGL(v.lens_fn, dim3(blocks), dim3(kBlock), lds, stream, a, first_bad, t);
    return hipGetLastError();
}

hipError_t launch_gather_columns(const MatArgs& a, const uint2* pairs, uint32_t count, uint8_t* out,
                                 hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_columns_kernel, dim3(count), dim3(64), 0, stream, a.data, a.parity, a.data_ss,
                       a.parity_ss, a.pitch, a.k, a.k + a.m, pairs, out);
    return hipGetLastError();
}

hipError_t launch_gather_columns_masked(const MatArgs& a, const uint2* pairs, const uint8_t* flags, uint32_t count,
                                        uint8_t* out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_columns_masked_kernel, dim3(count), dim3(64), 0, stream, a.data, a.parity, a.data_ss,
                       a.parity_ss, a.pitch, a.k, a.k + a.m, pairs, flags, out);
    return hipGetLastError();
}

namespace {
// One block per (piece, 4 KiB chunk): 256 lanes x 16 bytes.
__global__ __launch_bounds__(256) void copy_pieces_kernel(const uint8_t* src, uint8_t* dst, const uint64_t* pieces,
                                                          uint32_t chunks, uint32_t cols16) {
    const uint32_t piece = blockIdx.x / chunks;
    const uint32_t col = (blockIdx.x - piece * chunks) * 256u + threadIdx.x;
    if (col >= cols16) return;
    // readfirstlane returns int: the low words go through uint32_t, or an
    // offset with bit 31 set would sign-extend over the high word.
    const uint64_t s0 = pieces[2 * piece];
    const uint64_t so = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(s0))) |
                        (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(s0 >> 32)))) << 32);
    const uint64_t d0 = pieces[2 * piece + 1];
    const uint64_t dof = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(d0))) |
                         (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(d0 >> 32)))) << 32);
    const uint4 v = gload16<true>(src + so + static_cast<uint64_t>(col) * 16u);
    gstore16<true>(dst + dof + static_cast<uint64_t>(col) * 16u, v);
}

// Its twin for the pointer placement: piece i names entry pieces[2i] of the
// shard table on one side -- the slot, at byte offset slot_off -- and the
// address pieces[2i+1] on the other.  TO_SLOT: address -> slot (the commit of
// an update), else slot -> address (the present shards of a read).  Only the
// table entries the pieces name are loaded.
template <bool TO_SLOT>
__global__ __launch_bounds__(256) void copy_table_kernel(const uint64_t* shard_ptrs, const uint64_t* pieces,
                                                         uint32_t chunks, uint32_t cols16, uint64_t slot_off) {
    const uint32_t piece = blockIdx.x / chunks;
    const uint32_t col = (blockIdx.x - piece * chunks) * 256u + threadIdx.x;
    if (col >= cols16) return;
    const uint64_t i0 = pieces[2 * piece];
    const uint64_t idx = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(i0))) |
                         (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(i0 >> 32)))) << 32);
    uint8_t* slot = uniform_ptr(reinterpret_cast<uint8_t*>(shard_ptrs[idx])) + slot_off;
    uint8_t* addr = uniform_ptr(reinterpret_cast<uint8_t*>(pieces[2 * piece + 1]));
    const uint64_t at = static_cast<uint64_t>(col) * 16u;
    if constexpr (TO_SLOT) gstore16<true>(slot + at, gload16<true>(addr + at));
    else gstore16<true>(addr + at, gload16<true>(slot + at));
}
}  // namespace

hipError_t launch_copy_table(const uint64_t* shard_ptrs, const uint64_t* pieces, uint32_t count, size_t bytes,
                             uint64_t slot_off, bool to_slot, hipStream_t stream) {
    if (count == 0 || bytes == 0) return hipSuccess;
    if (!shard_ptrs || bytes % 16 != 0 || (slot_off & 15u)) return hipErrorInvalidValue;
    const uint64_t cols16 = bytes / 16, chunks = (cols16 + 255) / 256;
    if (cols16 > 0xFFFFFFFFull || static_cast<uint64_t>(count) * chunks > 0x7FFFFFFFull)
        return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(to_slot ? copy_table_kernel<true> : copy_table_kernel<false>,
                       dim3(static_cast<uint32_t>(count * chunks)), dim3(256), 0, stream, shard_ptrs, pieces,
                       static_cast<uint32_t>(chunks), static_cast<uint32_t>(cols16), slot_off);
    return hipGetLastError();
}

hipError_t launch_copy_pieces(const uint8_t* src, uint8_t* dst, const uint64_t* pieces, uint32_t count,
                              size_t bytes, hipStream_t stream) {
    if (count == 0 || bytes == 0) return hipSuccess;
    if (bytes % 16 != 0) return hipErrorInvalidValue;
    const uint64_t cols16 = bytes / 16, chunks = (cols16 + 255) / 256;
    if (cols16 > 0xFFFFFFFFull || static_cast<uint64_t>(count) * chunks > 0x7FFFFFFFull)
        return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(copy_pieces_kernel, dim3(static_cast<uint32_t>(count * chunks)), dim3(256), 0, stream, src, dst,
                       pieces, static_cast<uint32_t>(chunks), static_cast<uint32_t>(cols16));
    return hipGetLastError();
}

hipError_t launch_fill_splitmix(void* dev, size_t len, uint64_t seed, hipStream_t stream) {
    if (len == 0) return hipSuccess;
    const size_t nq = len / 8 + 1;
    const size_t blocks = std::min<size_t>((nq + kBlock - 1) / kBlock, 8192);
    hipLaunchKernelGGL(fill_splitmix_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kBlock), 0,
                       stream, static_cast<uint8_t*>(dev), len, seed);
    return hipGetLastError();
}

}  // namespace rsmi
