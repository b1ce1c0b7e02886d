// column_correct.hip -- the per-column correction kernel of rs_correct_columns
// (column_correct.hpp).  A translation unit of its own: the streaming kernels
// of rs_kernels.hip keep their code objects.
#include "column_correct.hpp"

#include "column_decode.hpp"
#include "combine_lens_map.hpp"
#include "gf_device.hpp"

namespace rsmi {

namespace {

using gfd::build_tables;
using gfd::Fields;
using gfd::fields;
using gfd::gf_mac;

constexpr int kColBlock = 256;    // lanes of a block: a 4 KiB column chunk
constexpr int kColSources = 32;   // sources whose split tables are in the LDS at a time
constexpr int kColLoads = 4;      // source loads in flight per lane
constexpr int kColLaneWork = 148; // a lane's decoder slice: kColumnWork in an odd number of dwords (banks)
static_assert(kColLaneWork >= kColumnWork && kColLaneWork % 4 == 0 && (kColLaneWork / 4) % 2 == 1, "lane slice");
// The phases share one region: phase A's tables [kColSources][MG][5] dwords,
// then phase B's decoder slices.
constexpr int kColRegion = kColBlock * kColLaneWork;
static_assert(kColSources * kColumnMaxSyn * 5 * 4 <= kColRegion, "tables fit the shared region");

// Phase A: the block's lanes compute the d syndrome columns of their 16-byte
// columns, S_t = sum_i W[t][i] * shard_i, with the split tables of W built in
// the LDS for kColSources sources at a time (rows past d are zero tables, so
// their syndromes are zero).  Phase B: a lane whose syndromes are not all zero
// decodes each of its byte columns below shard_len that has a non-zero
// syndrome (column_decode_core, exp / log tables and the lane's state in the
// LDS), XORs the error values into the located shards' bytes and counts them.
// The counts are summed per block in the LDS and go out as one atomicAdd per
// {block, shard}: a wholly wrong shard is 4,096 corrected bytes per block on
// one counter.
// LDS: exp [512] | log [256] | ids, x, u [256] each | counts u32 [256] | the shared region.
//
// PTRS (compile-time twin, the pointer placement): shard id of the stripe is at
// a.shard_ptrs[stripe * n + id].  The block resolves the addresses of the r
// present shards once, next to the ids, into 2 KiB more of LDS indexed by the
// shard's position in the present list: phase A's loads and phase B's byte
// stores read that array, never the table, and the table entries of shards
// outside the present list are never loaded.
//
// VARLEN (compile-time twin of the PTRS twin, rs_correct_columns_ptrs_lens):
// every job has a length of its own.  A block finds its {job, chunk} by the
// search of combine_lens_map.hpp (groups = 1) over a.first_block -- job j owns
// ceil(ncols_j / 256) blocks, one 4 KiB chunk each, as above -- and takes the
// job's column count and length from a.job_ncols / a.job_lens where the others
// take a.ncols16 / a.shard_len.  All of it is uniform: scalar loads and
// compares, no LDS and no lane state beyond the PTRS twin's.

// The twin's address array; only the PTRS instantiations allocate it.
template <bool PTRS>
__device__ __forceinline__ uint64_t* column_ptr_lds() {
    if constexpr (PTRS) {
        __shared__ uint64_t s_ptr[256];
        return s_ptr;
    } else {
        return nullptr;
    }
}

template <int MG, bool PTRS = false, bool VARLEN = false>
__global__ __launch_bounds__(kColBlock) void rs_column_kernel(ColArgs a) {
    static_assert(PTRS || !VARLEN, "per-job lengths: pointer placement only");
    __shared__ uint8_t s_exp[512];
    __shared__ uint8_t s_log[256];
    __shared__ uint8_t s_ids[256];
    __shared__ uint8_t s_x[256];
    __shared__ uint8_t s_u[256];
    __shared__ uint32_t s_cnt[256];
    __shared__ uint4 s_region[kColRegion / 16];
    const int tid = static_cast<int>(threadIdx.x);
    uint32_t jb, chunk, ncols16, shard_len;
    if constexpr (VARLEN) {
        const CombineBlock cb = combine_lens_block(a.first_block, a.njobs, 1u, blockIdx.x);
        jb = cb.job;
        chunk = cb.chunk;
        ncols16 = a.job_ncols[jb];
        shard_len = a.job_lens[jb];
    } else {
        jb = blockIdx.x / a.chunks;
        chunk = blockIdx.x - jb * a.chunks;
        ncols16 = a.ncols16;
        shard_len = a.shard_len;
    }
    const uint4 job = a.jobs[jb];
    const uint64_t stripe = __builtin_amdgcn_readfirstlane(job.x);
    const int r = static_cast<int>(__builtin_amdgcn_readfirstlane(job.z));
    const int d = static_cast<int>(__builtin_amdgcn_readfirstlane(job.w));
    const uint32_t np = (a.n + 15u) & ~15u;
    const uint8_t* tab = a.tables + static_cast<size_t>(__builtin_amdgcn_readfirstlane(job.y)) * ((3u + kColumnMaxSyn) * np);
    const uint8_t* W = tab + 3u * np;

    for (int i = tid; i < 512; i += kColBlock) s_exp[i] = a.gf[i];
    s_log[tid] = a.gf[512 + tid];
    s_cnt[tid] = 0u;
    uint64_t* s_ptr = column_ptr_lds<PTRS>();
    if (tid < r) {
        const uint8_t id = tab[tid];
        s_ids[tid] = id;
        s_x[tid] = tab[np + tid];
        s_u[tid] = tab[2u * np + tid];
        if constexpr (PTRS) s_ptr[tid] = a.shard_ptrs[stripe * a.n + id];
    }

    // Shard `id`, the pos-th of the present list.
    auto slot = [&](int pos, uint32_t id) -> uint8_t* {
        if constexpr (PTRS) {
            return reinterpret_cast<uint8_t*>(s_ptr[pos]);
        } else {
            return id < a.k ? a.data + stripe * a.data_ss + static_cast<uint64_t>(id) * a.pitch
                            : a.parity + stripe * a.parity_ss + static_cast<uint64_t>(id - a.k) * a.pitch;
        }
    };
    const uint32_t col = chunk * kColBlock + static_cast<uint32_t>(tid);
    const bool ok = col < ncols16;
    const uint32_t off = col * 16u;

    uint32_t* tw = reinterpret_cast<uint32_t*>(s_region);
    uint32_t acc[MG][4];
#pragma unroll
    for (int t = 0; t < MG; ++t)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[t][w] = 0u;

    for (int i0 = 0; i0 < r; i0 += kColSources) {
        const int cnt = min(kColSources, r - i0);
        __syncthreads();  // the ids (first round); the previous round's tables are consumed
        for (int idx = tid; idx < cnt * MG; idx += kColBlock) {
            const int il = idx / MG, t = idx - il * MG;
            const uint32_t c = t < d ? W[static_cast<uint32_t>(t) * np + static_cast<uint32_t>(i0 + il)] : 0u;
            build_tables(c, &tw[idx * 5]);
        }
        __syncthreads();
        if (!ok) continue;
        for (int q0 = 0; q0 < cnt; q0 += kColLoads) {
            uint4 x[kColLoads];
#pragma unroll
            for (int q = 0; q < kColLoads; ++q) {
                if (q0 + q >= cnt) break;
                if constexpr (PTRS) {
                    // Uniform: one LDS read, the base in SGPRs.  The halves go through
                    // uint32_t: the builtin returns int, which would sign-extend the low word.
                    const uint64_t at = s_ptr[i0 + q0 + q];
                    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(at));
                    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(at >> 32));
                    const uint8_t* base = reinterpret_cast<const uint8_t*>((static_cast<uint64_t>(hi) << 32) | lo);
                    x[q] = *reinterpret_cast<const uint4*>(base + off);
                } else {
                    const uint32_t id = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(s_ids[i0 + q0 + q]));
                    x[q] = *reinterpret_cast<const uint4*>(slot(i0 + q0 + q, id) + off);
                }
            }
#pragma unroll
            for (int q = 0; q < kColLoads; ++q) {
                if (q0 + q >= cnt) break;
                const Fields f0 = fields(x[q].x), f1 = fields(x[q].y), f2 = fields(x[q].z), f3 = fields(x[q].w);
                const uint32_t* T = &tw[(q0 + q) * MG * 5];
#pragma unroll
                for (int t = 0; t < MG; ++t) {
                    uint32_t Tt[5];
#pragma unroll
                    for (int w = 0; w < 5; ++w) Tt[w] = T[t * 5 + w];
                    acc[t][0] = gf_mac(acc[t][0], Tt, f0.a, f0.b, f0.c);
                    acc[t][1] = gf_mac(acc[t][1], Tt, f1.a, f1.b, f1.c);
                    acc[t][2] = gf_mac(acc[t][2], Tt, f2.a, f2.b, f2.c);
                    acc[t][3] = gf_mac(acc[t][3], Tt, f3.a, f3.b, f3.c);
                }
            }
        }
    }
    __syncthreads();  // every lane is done with the tables: the region becomes the decoder slices

    uint32_t any = 0u;
#pragma unroll
    for (int t = 0; t < MG; ++t) any |= acc[t][0] | acc[t][1] | acc[t][2] | acc[t][3];
    uint8_t* ws = reinterpret_cast<uint8_t*>(s_region) + tid * kColLaneWork;
    const ColumnGf g{s_exp, s_log};
    for (uint32_t b = 0; b < 16u; ++b) {
        if (!ok || any == 0u) break;
        const uint32_t o = off + b;
        if (o >= shard_len) break;  // the pad to 16 is not decoded
        const uint32_t wsel = b >> 2, sh = (b & 3u) * 8u;
        uint32_t nz = 0u;
#pragma unroll
        for (int t = 0; t < MG; ++t) {
            const uint32_t word = wsel == 0u ? acc[t][0] : wsel == 1u ? acc[t][1] : wsel == 2u ? acc[t][2] : acc[t][3];
            const uint32_t s = (word >> sh) & 0xFFu;
            ws[kColumnWsS + t] = static_cast<uint8_t>(s);
            nz |= s;
        }
        if (nz == 0u) continue;
        const int nu = column_decode_core(g, s_x, s_u, r, d, ws);
        if (nu < 0) {
            a.fail[jb] = 1u;
            continue;
        }
        for (int e = 0; e < nu; ++e) {
            const int pos = ws[kColumnWsPos + e];
            const uint32_t id = s_ids[pos];
            uint8_t* p = slot(pos, id) + o;
            *p ^= ws[kColumnWsX + e];
            atomicAdd(&s_cnt[id], 1u);
        }
    }
    __syncthreads();
    if (static_cast<uint32_t>(tid) < a.n && s_cnt[tid] != 0u)
        atomicAdd(&a.counts[static_cast<size_t>(jb) * a.n + static_cast<uint32_t>(tid)], s_cnt[tid]);
}

int column_mg(int m) { return m <= 4 ? 4 : m <= 8 ? 8 : 16; }

}  // namespace

bool column_correct_supported(int m) { return m >= 1 && m <= kColumnMaxSyn; }

bool plan_column_correct(ColArgs* a) {
    a->chunks = (a->ncols16 + kColBlock - 1) / kColBlock;
    return static_cast<uint64_t>(a->njobs) * a->chunks <= 0x7FFFFFFFull;
}

hipError_t launch_column_correct(const ColArgs& a, int m, hipStream_t stream) {
    if (a.njobs == 0 || a.chunks == 0) return hipSuccess;
    if (!column_correct_supported(m)) return hipErrorInvalidValue;
    const dim3 grid(a.njobs * a.chunks), block(kColBlock);
    if (a.shard_ptrs) {
        switch (column_mg(m)) {
            case 4: hipLaunchKernelGGL((rs_column_kernel<4, true>), grid, block, 0, stream, a); break;
            case 8: hipLaunchKernelGGL((rs_column_kernel<8, true>), grid, block, 0, stream, a); break;
            default: hipLaunchKernelGGL((rs_column_kernel<16, true>), grid, block, 0, stream, a); break;
        }
        return hipGetLastError();
    }
    switch (column_mg(m)) {
        case 4: hipLaunchKernelGGL(rs_column_kernel<4>, grid, block, 0, stream, a); break;
        case 8: hipLaunchKernelGGL(rs_column_kernel<8>, grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL(rs_column_kernel<16>, grid, block, 0, stream, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_column_correct_lens(const ColArgs& a, int m, uint32_t blocks, hipStream_t stream) {
    if (a.njobs == 0 || blocks == 0) return hipSuccess;
    if (!column_correct_supported(m) || !a.shard_ptrs || !a.first_block || !a.job_ncols || !a.job_lens ||
        blocks > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    const dim3 grid(blocks), block(kColBlock);
    switch (column_mg(m)) {
        case 4: hipLaunchKernelGGL((rs_column_kernel<4, true, true>), grid, block, 0, stream, a); break;
        case 8: hipLaunchKernelGGL((rs_column_kernel<8, true, true>), grid, block, 0, stream, a); break;
        default: hipLaunchKernelGGL((rs_column_kernel<16, true, true>), grid, block, 0, stream, a); break;
    }
    return hipGetLastError();
}

const char* column_variant_name(int m) {
    if (!column_correct_supported(m)) return "none";
    switch (column_mg(m)) {
        case 4: return "columns_MG4_B256";
        case 8: return "columns_MG8_B256";
        default: return "columns_MG16_B256";
    }
}

const char* column_ptrs_variant_name(int m) {
    if (!column_correct_supported(m)) return "none";
    switch (column_mg(m)) {
        case 4: return "columns_MG4_B256_ptrs";
        case 8: return "columns_MG8_B256_ptrs";
        default: return "columns_MG16_B256_ptrs";
    }
}

const char* column_lens_variant_name(int m) {
    if (!column_correct_supported(m)) return "none";
    switch (column_mg(m)) {
        case 4: return "columns_MG4_B256_ptrs_lens";
        case 8: return "columns_MG8_B256_ptrs_lens";
        default: return "columns_MG16_B256_ptrs_lens";
    }
}

}  // namespace rsmi
