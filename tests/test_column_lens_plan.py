"""CPU: the planner of rs_correct_columns_ptrs_lens
(csrc/column_lens_plan.cpp: rsmi::plan_column_lens, rsmi::plan_column_lens_jobs),
the block map the per-job-length column kernel shares with it
(csrc/combine_lens_map.hpp, one row group) and the parts of the binding that
need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/column_lens_plan.cpp with -fsanitize=address,undefined and run directly:
the search the program runs over first_block[] is the very function the kernel
compiles."""
import ctypes
import os
import subprocess

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "column_lens_plan.hpp"
#include "combine_lens_map.hpp"

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
}

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            std::printf("FAIL %s:%d: ", #cond, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

using rsmi::ColumnLensJobs;
using rsmi::ColumnLensPlan;

static const uint32_t kClean = 0xFFFFFFFFu;
static const size_t kMaxLen = ((size_t(1) << 28) - 1) * 16;  // the longest shard served

static bool empty(const ColumnLensPlan& p) { return p.live.empty() && p.worst_blocks == 0 && p.len_all == 0 && !p.degraded; }
static void stale(ColumnLensPlan* p) {  // contents that must not survive a refusal
    p->live = {3, 4};
    p->worst_blocks = 77;
    p->len_all = 5;
    p->degraded = true;
}
static void stale(ColumnLensJobs* j) {
    j->jobs.push_back(rsmi::ColumnLensJob{9, 9, 9, 9});
    j->hopeless = {1};
    j->sets.push_back({1, 0});
    j->ncols = {5};
    j->lens = {80};
    j->first_block = {0, 3};
    j->masked = {7, 7, 7};
}

// Flags with e erasures for stripe s (e <= n).
static void erase(std::vector<uint8_t>* fl, int n, size_t s, int e) {
    while (e > 0) {
        uint8_t& f = (*fl)[s * n + rnd() % n];
        if (!f) f = static_cast<uint8_t>(1 + rnd() % 255), --e;
    }
}

static size_t draw() {
    static const size_t fixed[] = {0, 1, 16, 4096, 4097 * 16, 17, 4112, 5000, 3 * 4096 + 40, 0};
    return rnd() % 4 ? fixed[rnd() % 10] : rnd() % 9001;
}

// The brute-force model of both functions: walks the stripes one by one.
static void against_model(const char* what, int k, int n, const std::vector<uint8_t>& erased, const std::vector<size_t>& lens,
                          const std::vector<uint32_t>& fb) {
    const size_t stripes = lens.size();
    const uint8_t* er = erased.empty() ? nullptr : erased.data();
    ColumnLensPlan p;
    stale(&p);
    const int rc = rsmi::plan_column_lens(k, n, stripes, er, lens.data(), &p);
    CHECK(rc == RS_OK, "%s: status %d", what, rc);
    if (rc != RS_OK) return;
    std::vector<uint32_t> live;
    uint64_t worst = 0;
    bool same = true, degraded = false;
    for (size_t s = 0; s < stripes; ++s) {
        same = same && lens[s] == lens[0];
        for (int id = 0; id < n && er; ++id) degraded = degraded || er[s * n + id] != 0;
        if (lens[s] == 0) continue;
        live.push_back(static_cast<uint32_t>(s));
        worst += (((lens[s] + 15) / 16) + 255) / 256;
    }
    CHECK(p.live == live && p.worst_blocks == worst && p.degraded == degraded && p.len_all == (same ? lens[0] : 0),
          "%s: %zu live, %llu blocks, len_all %u", what, p.live.size(), (unsigned long long)p.worst_blocks, p.len_all);

    ColumnLensJobs j;
    stale(&j);
    rsmi::plan_column_lens_jobs(k, n, stripes, er, lens.data(), p, fb.data(), &j);
    // the model's lists
    std::vector<uint32_t> want_jobs, want_hopeless, want_first;
    std::vector<size_t> want_masked(stripes, 0);
    std::map<std::vector<uint8_t>, uint32_t> seen;
    std::vector<std::vector<uint8_t>> want_sets;
    std::vector<uint32_t> want_table, want_r;
    uint64_t at = 0;
    for (size_t s = 0; s < stripes; ++s) {
        if (lens[s] == 0 || fb[s] == kClean) continue;
        std::vector<uint8_t> fl(n, 0);
        int r = n;
        for (int id = 0; id < n && er; ++id)
            if (er[s * n + id]) fl[id] = 1, --r;
        if (r - k < 2) {
            want_hopeless.push_back(static_cast<uint32_t>(s));
            continue;
        }
        if (!seen.count(fl)) {
            seen[fl] = static_cast<uint32_t>(want_sets.size());
            want_sets.push_back(fl);
        }
        want_jobs.push_back(static_cast<uint32_t>(s));
        want_table.push_back(seen[fl]);
        want_r.push_back(static_cast<uint32_t>(r));
        want_first.push_back(static_cast<uint32_t>(at));
        at += (((lens[s] + 15) / 16) + 255) / 256;
        want_masked[s] = lens[s];
    }
    const uint32_t nj = static_cast<uint32_t>(want_jobs.size());
    CHECK(j.jobs.size() == nj && j.ncols.size() == nj && j.lens.size() == nj && j.first_block.size() == (nj ? nj + 1u : 0u),
          "%s: %zu jobs, want %u", what, j.jobs.size(), nj);
    CHECK(j.hopeless == want_hopeless && j.masked == want_masked && j.sets == want_sets, "%s: hopeless, masked or sets", what);
    CHECK(at <= p.worst_blocks && j.blocks() == at, "%s: %u blocks, want %llu of at most %llu", what, j.blocks(),
          (unsigned long long)at, (unsigned long long)p.worst_blocks);
    if (j.jobs.size() != nj || j.first_block.size() != (nj ? nj + 1u : 0u)) return;
    for (uint32_t b = 0; b < nj; ++b) {
        const size_t s = want_jobs[b];
        CHECK(j.jobs[b].stripe == s && j.jobs[b].table == want_table[b] && j.jobs[b].r == want_r[b] &&
                  j.jobs[b].d == want_r[b] - static_cast<uint32_t>(k) && j.jobs[b].d >= 2,
              "%s: job %u = {%u, %u, %u, %u}", what, b, j.jobs[b].stripe, j.jobs[b].table, j.jobs[b].r, j.jobs[b].d);
        CHECK(j.ncols[b] == (lens[s] + 15) / 16 && j.ncols[b] >= 1 && j.lens[b] == lens[s] && j.first_block[b] == want_first[b],
              "%s: job %u: %u columns, %u bytes, first block %u", what, b, j.ncols[b], j.lens[b], j.first_block[b]);
    }
    if (nj == 0 || at > 200000) return;  // the walk below is for small plans
    // Every block maps, through the kernel's search, to {job, chunk}; the
    // chunks of a job are covered exactly once and each has a column.
    std::map<std::pair<uint32_t, uint32_t>, int> covered;
    for (uint32_t b = 0; b < j.blocks(); ++b) {
        const rsmi::CombineBlock cb = rsmi::combine_lens_block(j.first_block.data(), nj, 1u, b);
        if (cb.job >= nj) {
            CHECK(false, "%s: block %u maps to job %u", what, b, cb.job);
            return;
        }
        CHECK(j.first_block[cb.job] <= b && b < j.first_block[cb.job + 1] && cb.grp == 0 && cb.chunk == b - j.first_block[cb.job] &&
                  cb.chunks == (j.ncols[cb.job] + 255) / 256 && cb.chunk * 256u < j.ncols[cb.job],
              "%s: block %u: job %u chunk %u of %u", what, b, cb.job, cb.chunk, cb.chunks);
        ++covered[{cb.job, cb.chunk}];
    }
    uint64_t cells = 0;
    for (uint32_t b = 0; b < nj; ++b)
        for (uint32_t q = 0; q < (j.ncols[b] + 255) / 256; ++q, ++cells) {
            const auto f = covered.find({b, q});
            CHECK(f != covered.end() && f->second == 1, "%s: job %u chunk %u covered %d times", what, b, q,
                  f == covered.end() ? 0 : f->second);
        }
    CHECK(covered.size() == cells, "%s: %zu chunks covered, %llu exist", what, covered.size(), (unsigned long long)cells);
}

int main() {
    static const int codes[][2] = {{4, 6}, {10, 14}, {8, 14}, {3, 19}, {64, 80}, {240, 256}, {4, 5}, {4, 4}};
    for (const auto& kn : codes)
        for (size_t count : {size_t(1), size_t(2), size_t(3), size_t(37), size_t(400)})
            for (int rep = 0; rep < (count >= 37 ? 3 : 8); ++rep) {
                const int k = kn[0], n = kn[1], m = n - k;
                std::vector<size_t> lens(count);
                for (size_t& l : lens) l = draw();
                if (count == 400) {  // runs of zero-length stripes at the front, in the middle and at the end
                    for (size_t b = 0; b < 9; ++b) lens[b] = lens[200 + b] = lens[count - 1 - b] = 0;
                    lens[9] = 3 * 4096 + 40, lens[count - 10] = 1;
                }
                if (count == 37 && rep == 0) lens[5] = kMaxLen;  // the longest shard, counted only
                std::vector<uint8_t> erased(count * n, 0);
                for (size_t s = 0; s < count; ++s) erase(&erased, n, s, static_cast<int>(rnd() % (m + 1)));
                // verdicts: clean, dirty at some offset; zero-length stripes get both too (never a job)
                std::vector<uint32_t> fb(count);
                for (uint32_t& v : fb) v = rnd() % 3 ? (rep == 1 ? 0u : rnd() % 4096) : kClean;
                if (rep == 2) std::fill(fb.begin(), fb.end(), kClean);
                against_model("drawn", k, n, erased, lens, fb);
                if (rep < 2) against_model("no flags", k, n, {}, lens, fb);
            }
    // equal lengths: len_all names the length; a zero-length stripe among them does not
    {
        ColumnLensPlan p;
        const std::vector<size_t> eq(5, 5000);
        std::vector<size_t> ne = eq;
        ne[2] = 0;
        CHECK(rsmi::plan_column_lens(10, 14, 5, nullptr, eq.data(), &p) == RS_OK && p.len_all == 5000 && p.live.size() == 5,
              "equal lengths");
        CHECK(rsmi::plan_column_lens(10, 14, 5, nullptr, ne.data(), &p) == RS_OK && p.len_all == 0 && p.live.size() == 4,
              "equal lengths and an empty stripe");
    }
    // nothing to do
    {
        ColumnLensPlan p;
        stale(&p);
        CHECK(rsmi::plan_column_lens(10, 14, 0, nullptr, nullptr, &p) == RS_OK && empty(p), "stripes == 0");
        const std::vector<size_t> zero(3, 0);
        std::vector<uint8_t> fl(3 * 14, 0);
        fl[14 + 3] = 1;
        stale(&p);
        CHECK(rsmi::plan_column_lens(10, 14, 3, fl.data(), zero.data(), &p) == RS_OK && p.live.empty() && p.worst_blocks == 0 &&
                  p.degraded && p.len_all == 0,
              "all lengths 0");
        ColumnLensJobs j;
        stale(&j);
        const std::vector<uint32_t> fb = {0, 0, 0};
        rsmi::plan_column_lens_jobs(10, 14, 3, fl.data(), zero.data(), p, fb.data(), &j);
        CHECK(j.jobs.empty() && j.hopeless.empty() && j.sets.empty() && j.first_block.empty() && j.blocks() == 0 &&
                  j.masked == std::vector<size_t>(3, 0),
              "all lengths 0: no jobs");
    }
    // refusals, each leaving the plan empty
    {
        ColumnLensPlan p;
        const std::vector<size_t> lens = {1000, 0, 16};
        std::vector<uint8_t> fl(3 * 14, 0);
        auto refused = [&](const char* what, int want, int rc) {
            CHECK(rc == want, "%s: status %d, want %d", what, rc, want);
            CHECK(empty(p), "%s: plan not empty", what);
            stale(&p);
        };
        stale(&p);
        refused("NULL lens", RS_EINVAL, rsmi::plan_column_lens(10, 14, 3, fl.data(), nullptr, &p));
        refused("k < 1", RS_EINVAL, rsmi::plan_column_lens(0, 4, 3, nullptr, lens.data(), &p));
        refused("n < k", RS_EINVAL, rsmi::plan_column_lens(10, 9, 3, nullptr, lens.data(), &p));
        refused("n > 256", RS_EINVAL, rsmi::plan_column_lens(250, 257, 3, nullptr, lens.data(), &p));
        refused("m > 16", RS_EINVAL, rsmi::plan_column_lens(10, 27, 3, nullptr, lens.data(), &p));
        CHECK(rsmi::plan_column_lens(10, 26, 3, nullptr, lens.data(), &p) == RS_OK, "m == 16");
        stale(&p);
        refused("stripes == 2^32", RS_EINVAL, rsmi::plan_column_lens(10, 14, size_t(1) << 32, fl.data(), lens.data(), &p));
        CHECK(rsmi::plan_column_lens(10, 14, 3, fl.data(), lens.data(), nullptr) == RS_EINVAL, "NULL plan");
        // 2^28 or more 16-byte columns, with or without flags
        for (size_t bad : {kMaxLen + 1, kMaxLen + 16, size_t(1) << 40, ~size_t(0), ~size_t(0) - 14}) {
            const std::vector<size_t> l2 = {1000, bad, 16};
            refused("a length of 2^28 columns", RS_EINVAL, rsmi::plan_column_lens(10, 14, 3, fl.data(), l2.data(), &p));
            refused("a length of 2^28 columns, no flags", RS_EINVAL, rsmi::plan_column_lens(10, 14, 3, nullptr, l2.data(), &p));
        }
        // more than m erasures: in a stripe with bytes, and in a zero-length one
        for (size_t s : {size_t(0), size_t(1)}) {
            std::vector<uint8_t> f5(3 * 14, 0);
            for (int id = 0; id < 5; ++id) f5[s * 14 + 2 * id] = 1;
            refused("five erasures", RS_ENOT_ENOUGH, rsmi::plan_column_lens(10, 14, 3, f5.data(), lens.data(), &p));
            // a bad length is judged before the flags
            const std::vector<size_t> l2 = {1000, 0, kMaxLen + 1};
            refused("five erasures and a bad length", RS_EINVAL, rsmi::plan_column_lens(10, 14, 3, f5.data(), l2.data(), &p));
        }
        {
            std::vector<uint8_t> f1(3 * 4, 0);
            f1[4 + 1] = 1;  // m == 0: any erasure is one too many, also in the zero-length stripe
            refused("m == 0 with an erasure", RS_ENOT_ENOUGH, rsmi::plan_column_lens(4, 4, 3, f1.data(), lens.data(), &p));
        }
        // more than 2^31 - 1 blocks in the worst-case column launch: the longest
        // shard has 2^20 chunks, 2,048 of them 2^31; one chunk fewer is served.
        {
            std::vector<size_t> big(2048, kMaxLen);
            refused("2^31 blocks", RS_EINVAL, rsmi::plan_column_lens(10, 14, 2048, nullptr, big.data(), &p));
            std::vector<uint8_t> f5(2048 * 14, 0);
            for (int id = 0; id < 5; ++id) f5[7 * 14 + id] = 1;
            refused("2^31 blocks and five erasures", RS_ENOT_ENOUGH, rsmi::plan_column_lens(10, 14, 2048, f5.data(), big.data(), &p));
            big[7] = kMaxLen - 4096;
            CHECK(rsmi::plan_column_lens(10, 14, 2048, nullptr, big.data(), &p) == RS_OK && p.worst_blocks == 0x7FFFFFFFull,
                  "2^31 - 1 blocks");
            // every stripe dirty: the launch is the worst case, and its prefix still fits 32 bits
            ColumnLensJobs j;
            const std::vector<uint32_t> fb(2048, 0);
            rsmi::plan_column_lens_jobs(10, 14, 2048, nullptr, big.data(), p, fb.data(), &j);
            CHECK(j.jobs.size() == 2048 && j.blocks() == 0x7FFFFFFFu && j.first_block[2047] == 0x7FFFFFFFu - (1u << 20),
                  "the worst case as a launch");
            big[7] = 0;  // a zero-length stripe owns no block
            CHECK(rsmi::plan_column_lens(10, 14, 2048, nullptr, big.data(), &p) == RS_OK &&
                      p.worst_blocks == 0x80000000ull - (1u << 20) && p.live.size() == 2047,
                  "2^31 - 2^20 blocks");
        }
    }
    std::printf("plan_column_lens: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_column_lens_standalone_sanitized(tmp_path):
    src = tmp_path / "column_lens_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "column_lens_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "column_lens_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_column_lens: 0 failures" in run.stdout


def test_column_lens_entry_point_is_exported():
    import rsmi
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    assert "rs_correct_columns_ptrs_lens" in rsmi.EXPORTS and hasattr(lib, "rs_correct_columns_ptrs_lens")
    fn = rsmi.load().rs_correct_columns_ptrs_lens
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    assert fn.restype is ctypes.c_int32
    assert list(fn.argtypes) == [vp, vp, ctypes.POINTER(sz), sz, vp, ctypes.POINTER(ctypes.c_int32), vp, vp]
    assert rsmi.FEC.STAT_COLUMN_LENS_LAUNCHES == 28
    assert rsmi.FEC.STAT_SCRUB_LENS_LAUNCHES == 27
    assert callable(rsmi.FEC.correct_columns_ptrs_lens)


def test_null_context_is_rejected_without_a_device():
    """The call refuses a NULL context with RS_EINVAL before touching HIP;
    callable on a CPU-only machine."""
    import rsmi
    fn = rsmi.load().rs_correct_columns_ptrs_lens
    lens = (ctypes.c_size_t * 2)(16, 4096)
    flags = ctypes.create_string_buffer(2 * 14)
    status = (ctypes.c_int32 * 2)(7, 7)
    assert fn(None, 4096, lens, 2, ctypes.cast(flags, ctypes.c_void_p), status, None, None) == rsmi.RS_EINVAL
    assert fn(None, None, None, 0, None, None, None, None) == rsmi.RS_EINVAL
    assert fn(None, 4096, None, 2, None, None, None, None) == rsmi.RS_EINVAL
    assert list(status) == [7, 7]
