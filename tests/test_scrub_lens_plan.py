"""CPU: the planner of rs_verify_ptrs_lens / rs_reconstruct_checked_ptrs_lens
(csrc/scrub_lens_plan.cpp, rsmi::plan_scrub_lens), the block map the three
per-stripe-length kernels share with it (csrc/combine_lens_map.hpp) and the
parts of the binding that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/scrub_lens_plan.cpp and csrc/check_plan.cpp with
-fsanitize=address,undefined and run directly: the search the program runs
over first_block[] is the very function the kernels compile."""
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
#include <tuple>
#include <vector>

#include "combine_lens_map.hpp"
#include "scrub_lens_plan.hpp"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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

using rsmi::ScrubLensList;
using rsmi::ScrubLensPlan;

static bool empty(const ScrubLensList& l) {
    return l.ncols.empty() && l.lens.empty() && l.first_block.empty() && l.groups == 0 && l.blocks() == 0;
}
static bool empty(const ScrubLensPlan& p) {
    return p.checks.intact.empty() && p.checks.jobs.empty() && p.checks.entries.empty() && p.checks.flags.empty() &&
           p.checks.saturated == 0 && p.checks.max_j == 0 && empty(p.intact) && empty(p.jobs) && p.iters == 1 && p.live == 0 &&
           p.len_all == 0;
}
static void stale(ScrubLensPlan* p) {  // contents that must not survive a refusal
    p->checks.intact.push_back(3);
    p->checks.jobs.push_back(rsmi::ReadJob{1, 0, 2});
    p->checks.entries.push_back(rsmi::ReadEntry{5, 1, 0});
    p->checks.flags.push_back(1);
    p->checks.saturated = 4;
    p->checks.max_j = 2;
    for (ScrubLensList* l : {&p->intact, &p->jobs}) {
        l->ncols.push_back(7);
        l->lens.push_back(100);
        l->first_block = {0, 5};
        l->groups = 2;
    }
    p->iters = 9;
    p->live = 5;
    p->len_all = 77;
}

static const size_t kMaxLen = ((size_t(1) << 28) - 1) * 16;  // the longest shard served

// The brute-force model: walks the stripes, keeps those with bytes, and lists
// for each launch {stripe, columns, length, blocks}.
struct ModelEntry {
    uint32_t stripe, ncols, len;
    uint64_t blocks;
};
struct Model {
    std::vector<ModelEntry> intact, jobs;
    uint32_t max_j = 0, job_groups = 0;
    size_t live = 0;
};
static uint64_t model_chunks(uint32_t ncols, uint32_t iters) {
    // 256-column pieces dealt over blocks that run at most `iters` of them
    const uint64_t pieces = (static_cast<uint64_t>(ncols) + 255) / 256;
    const uint64_t it = std::min<uint64_t>(pieces, iters);
    return it ? (pieces + it - 1) / it : 0;
}
static Model model(int k, int n, const std::vector<uint8_t>& erased, const std::vector<size_t>& lens, bool repair,
                   uint32_t intact_groups, uint32_t iters) {
    Model mo;
    const int m = n - k;
    std::vector<std::pair<uint32_t, int>> job_e;
    for (size_t s = 0; s < lens.size(); ++s) {
        int e = 0;
        for (int id = 0; id < n && !erased.empty(); ++id) e += erased[s * n + id] != 0;
        if (lens[s] == 0) continue;
        ++mo.live;
        const uint32_t ncols = static_cast<uint32_t>((lens[s] + 15) / 16);
        ModelEntry en{static_cast<uint32_t>(s), ncols, static_cast<uint32_t>(lens[s]), 0};
        if (e == 0) {
            en.blocks = model_chunks(ncols, iters) * intact_groups;
            mo.intact.push_back(en);
        } else if (repair || e < m) {
            mo.max_j = std::max<uint32_t>(mo.max_j, repair ? m : m - e);
            mo.jobs.push_back(en);
        }
    }
    mo.job_groups = (mo.max_j + 3) / 4;
    for (ModelEntry& en : mo.jobs) en.blocks = model_chunks(en.ncols, iters) * mo.job_groups;
    return mo;
}

static void same_list(const char* what, const char* which, const ScrubLensList& l, const std::vector<ModelEntry>& want,
                      uint32_t groups, uint32_t iters) {
    const uint32_t nj = static_cast<uint32_t>(want.size());
    if (nj == 0) {
        CHECK(empty(l), "%s: %s: no entries, list not empty", what, which);
        return;
    }
    CHECK(l.ncols.size() == nj && l.lens.size() == nj && l.first_block.size() == nj + 1u && l.groups == groups,
          "%s: %s: table sizes, %u groups", what, which, l.groups);
    if (l.ncols.size() != nj || l.lens.size() != nj || l.first_block.size() != nj + 1u) return;
    uint64_t at = 0;
    for (uint32_t b = 0; b < nj; ++b) {
        CHECK(l.ncols[b] == want[b].ncols && l.lens[b] == want[b].len && l.ncols[b] >= 1, "%s: %s: entry %u: %u columns, %u bytes",
              what, which, b, l.ncols[b], l.lens[b]);
        CHECK(l.first_block[b] == at, "%s: %s: first_block[%u] = %u, want %llu", what, which, b, l.first_block[b],
              (unsigned long long)at);
        at += want[b].blocks;
    }
    CHECK(l.first_block[nj] == at && l.blocks() == at, "%s: %s: %u blocks, want %llu", what, which, l.blocks(),
          (unsigned long long)at);
    if (groups == 0 || at > 200000) return;  // the walk below is for small plans
    // Every block maps, through the kernels' search, to the {entry, chunk,
    // group} of the model, and the iterations the kernels then run cover every
    // (256-column piece, row group) of every entry exactly once.
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, int> covered;
    for (uint32_t b = 0; b < l.blocks(); ++b) {
        const rsmi::CombineBlock cb = rsmi::combine_lens_block(l.first_block.data(), nj, groups, b);
        if (cb.job >= nj) {
            CHECK(false, "%s: %s: block %u maps to entry %u", what, which, b, cb.job);
            return;
        }
        CHECK(l.first_block[cb.job] <= b && b < l.first_block[cb.job + 1], "%s: %s: block %u outside entry %u", what, which, b,
              cb.job);
        const uint32_t r = b - l.first_block[cb.job];
        CHECK(cb.grp == r % groups && cb.chunk == r / groups && cb.chunks == model_chunks(want[cb.job].ncols, iters) &&
                  cb.chunk < cb.chunks,
              "%s: %s: block %u: group %u, chunk %u of %u", what, which, b, cb.grp, cb.chunk, cb.chunks);
        bool first = true;
        for (uint32_t it = 0; it < iters; ++it) {
            const uint64_t colbase = (static_cast<uint64_t>(cb.chunk) + static_cast<uint64_t>(it) * cb.chunks) * 256;
            if (colbase >= want[cb.job].ncols) break;
            first = false;
            ++covered[std::make_tuple(cb.job, static_cast<uint32_t>(colbase / 256), cb.grp)];
        }
        CHECK(!first, "%s: %s: block %u has no column", what, which, b);
    }
    uint64_t cells = 0;
    for (uint32_t b = 0; b < nj; ++b)
        for (uint32_t q = 0; q < (want[b].ncols + 255) / 256; ++q)
            for (uint32_t g = 0; g < groups; ++g, ++cells) {
                const auto f = covered.find(std::make_tuple(b, q, g));
                CHECK(f != covered.end() && f->second == 1, "%s: %s: entry %u piece %u group %u covered %d times", what, which, b, q,
                      g, f == covered.end() ? 0 : f->second);
            }
    CHECK(covered.size() == cells, "%s: %s: %zu cells covered, %llu exist", what, which, covered.size(), (unsigned long long)cells);
}

// Flags with e erasures for stripe s (e <= n).
static void erase(std::vector<uint8_t>* fl, int n, size_t s, int e) {
    while (e > 0) {
        uint8_t& f = (*fl)[s * n + rnd() % n];
        if (!f) f = static_cast<uint8_t>(1 + rnd() % 255), --e;
    }
}

static void against_model(const char* what, int k, int n, const std::vector<uint8_t>& erased, const std::vector<size_t>& lens,
                          bool repair, uint32_t intact_groups, uint32_t iters) {
    ScrubLensPlan p;
    stale(&p);
    const int rc = rsmi::plan_scrub_lens(k, n, lens.size(), erased.empty() ? nullptr : erased.data(), lens.data(), repair,
                                         intact_groups, iters, &p);
    CHECK(rc == RS_OK, "%s: status %d", what, rc);
    if (rc != RS_OK) return;
    const Model mo = model(k, n, erased, lens, repair, intact_groups, iters);
    CHECK(p.live == mo.live && p.iters == iters, "%s: %zu live, %u iters", what, p.live, p.iters);
    bool same = !lens.empty();
    for (size_t l : lens) same = same && l == lens[0];
    CHECK(p.len_all == (same ? lens[0] : 0), "%s: len_all %u", what, p.len_all);
    if (mo.live == 0) {
        CHECK(empty(p.intact) && empty(p.jobs) && p.checks.intact.empty() && p.checks.jobs.empty(), "%s: no bytes, lists not empty",
              what);
        return;
    }
    CHECK(p.checks.intact.size() == mo.intact.size() && p.checks.jobs.size() == mo.jobs.size() && p.checks.max_j == mo.max_j,
          "%s: %zu intact, %zu jobs, max_j %u", what, p.checks.intact.size(), p.checks.jobs.size(), p.checks.max_j);
    if (p.checks.intact.size() != mo.intact.size() || p.checks.jobs.size() != mo.jobs.size()) return;
    for (size_t b = 0; b < mo.intact.size(); ++b)
        CHECK(p.checks.intact[b] == mo.intact[b].stripe, "%s: intact %zu is stripe %u", what, b, p.checks.intact[b]);
    for (size_t b = 0; b < mo.jobs.size(); ++b)
        CHECK(p.checks.jobs[b].stripe == mo.jobs[b].stripe, "%s: job %zu is stripe %llu", what, b,
              (unsigned long long)p.checks.jobs[b].stripe);
    CHECK(p.checks.flags.size() == mo.jobs.size() * n, "%s: flags", what);
    // the jobs themselves are the equal-length planners' over the stripes with bytes
    if (!erased.empty()) {
        std::vector<uint32_t> list;
        for (size_t s = 0; s < lens.size(); ++s)
            if (lens[s]) list.push_back(static_cast<uint32_t>(s));
        rsmi::CheckPlan q;
        const int qc = repair ? rsmi::plan_repairs_ptrs(k, n, lens.size(), erased.data(), list.data(), list.size(), &q)
                              : rsmi::plan_checks_ptrs(k, n, lens.size(), erased.data(), list.data(), list.size(), &q);
        bool eq = qc == RS_OK && q.intact == p.checks.intact && q.flags == p.checks.flags && q.saturated == p.checks.saturated &&
                  q.jobs.size() == p.checks.jobs.size() && q.entries.size() == p.checks.entries.size();
        for (size_t b = 0; eq && b < q.jobs.size(); ++b)
            eq = q.jobs[b].stripe == p.checks.jobs[b].stripe && q.jobs[b].first == p.checks.jobs[b].first && q.jobs[b].j == p.checks.jobs[b].j;
        for (size_t b = 0; eq && b < q.entries.size(); ++b)
            eq = q.entries[b].dst == p.checks.entries[b].dst && q.entries[b].row == p.checks.entries[b].row &&
                 q.entries[b].pad == p.checks.entries[b].pad;
        CHECK(eq, "%s: not the equal-length planner's jobs", what);
    }
    same_list(what, "intact", p.intact, mo.intact, intact_groups, iters);
    same_list(what, "jobs", p.jobs, mo.jobs, mo.job_groups, iters);
}

static size_t draw() {
    static const size_t fixed[] = {0, 1, 16, 4096, 4097 * 16, 17, 4112, 5000, 3 * 4096 + 40, 0};
    return rnd() % 4 ? fixed[rnd() % 10] : rnd() % 9001;
}

int main() {
    static const int codes[][2] = {{4, 6}, {10, 14}, {8, 14}, {3, 19}, {64, 80}, {4, 4}};
    // prefix tables against the model: random flags and lengths
    for (uint32_t iters : {1u, 2u, 3u})
        for (const auto& kn : codes)
            for (int repair = 0; repair < 2; ++repair)
                for (size_t count : {size_t(1), size_t(2), size_t(3), size_t(37), size_t(400)})
                    for (int rep = 0; rep < (count >= 37 ? 2 : 6); ++rep) {
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
                        const uint32_t ig = m == 0 ? 0u : static_cast<uint32_t>((m + (m > 8 ? 15 : 3)) / (m > 8 ? 16 : 4));
                        against_model("drawn", k, n, erased, lens, repair != 0, ig, iters);
                        if (!repair && rep == 0) against_model("no flags", k, n, {}, lens, false, ig, iters);
                    }
    // every listed length next to zero-length stripes
    for (uint32_t iters : {1u, 2u, 3u})
        for (size_t l : {size_t(1), size_t(16), size_t(4096), size_t(4097) * 16, kMaxLen}) {
            const int k = 10, n = 14;
            for (const std::vector<size_t>& lens :
                 std::vector<std::vector<size_t>>{{l}, {0, l}, {l, 0}, {0, l, 0}, {l, 0, l}, {0, 0, l, 16, 0, 0, l, 0, 0}}) {
                std::vector<uint8_t> erased(lens.size() * n, 0);
                against_model("intact", k, n, erased, lens, false, 1, iters);
                for (size_t s = 0; s < lens.size(); ++s) erase(&erased, n, s, 1 + static_cast<int>(s % 4));
                against_model("degraded", k, n, erased, lens, false, 1, iters);
                against_model("repair", k, n, erased, lens, true, 1, iters);
            }
        }
    // equal lengths: len_all names the length; a zero-length stripe among them does not
    {
        ScrubLensPlan p;
        const std::vector<size_t> eq(5, 5000);
        std::vector<size_t> ne = eq;
        ne[2] = 0;
        CHECK(rsmi::plan_scrub_lens(10, 14, 5, nullptr, eq.data(), false, 1, 1, &p) == RS_OK && p.len_all == 5000 && p.live == 5,
              "equal lengths");
        CHECK(rsmi::plan_scrub_lens(10, 14, 5, nullptr, ne.data(), false, 1, 1, &p) == RS_OK && p.len_all == 0 && p.live == 4,
              "equal lengths and an empty stripe");
    }
    // nothing to do
    {
        ScrubLensPlan p;
        stale(&p);
        CHECK(rsmi::plan_scrub_lens(10, 14, 0, nullptr, nullptr, true, 1, 1, &p) == RS_OK && empty(p), "stripes == 0");
        const std::vector<size_t> zero(3, 0);
        std::vector<uint8_t> fl(3 * 14, 0);
        fl[14 + 3] = 1;
        stale(&p);
        CHECK(rsmi::plan_scrub_lens(10, 14, 3, fl.data(), zero.data(), true, 1, 1, &p) == RS_OK && p.live == 0 && empty(p.intact) &&
                  empty(p.jobs) && p.checks.jobs.empty() && p.checks.intact.empty(),
              "all lengths 0");
    }
    // refusals, each leaving the plan empty
    {
        ScrubLensPlan p;
        const std::vector<size_t> lens = {1000, 0, 16};
        std::vector<uint8_t> fl(3 * 14, 0);
        auto refused = [&](const char* what, int want, int rc) {
            CHECK(rc == want, "%s: status %d, want %d", what, rc, want);
            CHECK(empty(p), "%s: plan not empty", what);
            stale(&p);
        };
        stale(&p);
        refused("NULL lens", RS_EINVAL, rsmi::plan_scrub_lens(10, 14, 3, fl.data(), nullptr, false, 1, 1, &p));
        refused("NULL erased for a repair", RS_EINVAL, rsmi::plan_scrub_lens(10, 14, 3, nullptr, lens.data(), true, 1, 1, &p));
        refused("iters == 0", RS_EINVAL, rsmi::plan_scrub_lens(10, 14, 3, fl.data(), lens.data(), false, 1, 0, &p));
        refused("n > 256", RS_EINVAL, rsmi::plan_scrub_lens(10, 257, 3, fl.data(), lens.data(), false, 1, 1, &p));
        refused("stripes == 2^32", RS_EINVAL, rsmi::plan_scrub_lens(10, 14, size_t(1) << 32, fl.data(), lens.data(), false, 1, 1, &p));
        CHECK(rsmi::plan_scrub_lens(10, 14, 3, fl.data(), lens.data(), false, 1, 1, nullptr) == RS_EINVAL, "NULL plan");
        // 2^28 or more 16-byte columns, with or without flags
        for (size_t bad : {kMaxLen + 1, kMaxLen + 16, size_t(1) << 40, ~size_t(0), ~size_t(0) - 14}) {
            const std::vector<size_t> l2 = {1000, bad, 16};
            refused("a length of 2^28 columns", RS_EINVAL, rsmi::plan_scrub_lens(10, 14, 3, fl.data(), l2.data(), false, 1, 1, &p));
            refused("a length of 2^28 columns, no flags", RS_EINVAL, rsmi::plan_scrub_lens(10, 14, 3, nullptr, l2.data(), false, 1, 1, &p));
        }
        // more than m erasures: in a stripe with bytes, and in a zero-length one
        for (size_t s : {size_t(0), size_t(1)}) {
            std::vector<uint8_t> f5(3 * 14, 0);
            for (int id = 0; id < 5; ++id) f5[s * 14 + 2 * id] = 1;
            refused("five erasures, verify", RS_ENOT_ENOUGH, rsmi::plan_scrub_lens(10, 14, 3, f5.data(), lens.data(), false, 1, 1, &p));
            refused("five erasures, repair", RS_ENOT_ENOUGH, rsmi::plan_scrub_lens(10, 14, 3, f5.data(), lens.data(), true, 1, 1, &p));
        }
        {
            std::vector<uint8_t> f1(3 * 4, 0);
            f1[4 + 1] = 1;  // m == 0: any erasure is one too many, also in the zero-length stripe
            refused("m == 0 with an erasure", RS_ENOT_ENOUGH, rsmi::plan_scrub_lens(4, 4, 3, f1.data(), lens.data(), false, 0, 1, &p));
        }
        // more than 2^31 - 1 blocks in all: the longest shard has 2^20 pieces.
        // Intact: 1,024 stripes x 2^20 x 2 groups = 2^31 blocks; one piece fewer is served.
        {
            std::vector<size_t> big(1024, kMaxLen);
            std::vector<uint8_t> none(1024 * 14, 0);
            refused("2^31 blocks, intact", RS_EINVAL, rsmi::plan_scrub_lens(10, 14, 1024, none.data(), big.data(), false, 2, 1, &p));
            big[7] = kMaxLen - 4096;
            CHECK(rsmi::plan_scrub_lens(10, 14, 1024, none.data(), big.data(), false, 2, 1, &p) == RS_OK &&
                      uint64_t(p.intact.blocks()) + p.jobs.blocks() == 0x7FFFFFFEull,
                  "2^31 - 2 blocks, intact");
            big[7] = kMaxLen;
            CHECK(rsmi::plan_scrub_lens(10, 14, 1024, none.data(), big.data(), false, 2, 2, &p) == RS_OK && p.intact.blocks() == (1u << 30),
                  "two iterations halve the blocks");
            // the two launches together: 1,024 intact + 1,024 degraded (one row group each)
            std::vector<size_t> both(2048, kMaxLen);
            std::vector<uint8_t> half(2048 * 14, 0);
            for (size_t s = 1024; s < 2048; ++s) half[s * 14 + 3] = 1;
            stale(&p);
            refused("2^31 blocks over both launches", RS_EINVAL,
                    rsmi::plan_scrub_lens(10, 14, 2048, half.data(), both.data(), false, 1, 1, &p));
            both[2047] = 0;
            CHECK(rsmi::plan_scrub_lens(10, 14, 2048, half.data(), both.data(), false, 1, 1, &p) == RS_OK &&
                      p.intact.blocks() == (1u << 30) && p.jobs.blocks() == (1u << 30) - (1u << 20),
                  "2^31 - 2^20 blocks over both launches");
        }
    }
    std::printf("plan_scrub_lens: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_scrub_lens_standalone_sanitized(tmp_path):
    src = tmp_path / "scrub_lens_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "scrub_lens_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "scrub_lens_plan.cpp"),
                    os.path.join(CSRC, "check_plan.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_scrub_lens: 0 failures" in run.stdout


def test_scrub_lens_entry_points_are_exported():
    import rsmi
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    for name in ("rs_verify_ptrs_lens", "rs_reconstruct_checked_ptrs_lens"):
        assert name in rsmi.EXPORTS and hasattr(lib, name)
    assert rsmi.FEC.STAT_SCRUB_LENS_LAUNCHES == 27
    for name in ("verify_ptrs_lens", "reconstruct_checked_ptrs_lens"):
        assert callable(getattr(rsmi.FEC, name))


def test_null_context_is_rejected_without_a_device():
    """Both calls refuse a NULL context with RS_EINVAL before touching HIP;
    callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    lens = (ctypes.c_size_t * 2)(16, 4096)
    flags = ctypes.create_string_buffer(2 * 14)
    for fn in (lib.rs_verify_ptrs_lens, lib.rs_reconstruct_checked_ptrs_lens):
        assert fn(None, 4096, lens, 2, ctypes.cast(flags, ctypes.c_void_p), 8192, None) == rsmi.RS_EINVAL
        assert fn(None, None, None, 0, None, None, None) == rsmi.RS_EINVAL
        assert fn(None, 4096, None, 2, None, 8192, None) == rsmi.RS_EINVAL
