"""CPU: the planner of rs_combine_lens (csrc/combine_plan.cpp,
rsmi::plan_combine_lens), the block map its kernel shares with it
(csrc/combine_lens_map.hpp) and the parts of the binding that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/combine_plan.cpp and the shared header with -fsanitize=address,undefined
and run directly: the search the program runs over first_block[] is the very
function the kernel compiles."""
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
#include "combine_plan.hpp"

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

// A job that owns its host arrays.
struct Job {
    std::vector<uint64_t> src, dst;
    std::vector<uint8_t> coef;
    uint32_t accumulate = 0, reserved = 0;
};
static Job job(std::vector<uint64_t> src, std::vector<uint64_t> dst, uint32_t accumulate = 0) {
    Job j;
    j.src = std::move(src);
    j.dst = std::move(dst);
    j.coef.resize(j.src.size() * j.dst.size());
    for (uint8_t& c : j.coef) c = static_cast<uint8_t>(rnd());
    j.accumulate = accumulate;
    return j;
}
static std::vector<rs_combine_job> view(const std::vector<Job>& jobs) {
    std::vector<rs_combine_job> v;
    for (const Job& j : jobs) {
        rs_combine_job c{};
        c.src = j.src.data();
        c.dst = j.dst.data();
        c.coef = j.coef.data();
        c.nsrc = static_cast<uint32_t>(j.src.size());
        c.nout = static_cast<uint32_t>(j.dst.size());
        c.accumulate = j.accumulate;
        c.reserved = j.reserved;
        v.push_back(c);
    }
    return v;
}

static bool empty(const rsmi::CombinePlan& p) {
    return p.jobs.empty() && p.addrs.empty() && p.coef.empty() && p.max_nsrc == 0 && p.max_nout == 0 && p.rows == 0 &&
           p.ncols.empty() && p.first_block.empty() && p.mg == 0 && p.groups == 0 && p.iters == 0 && p.ncols_all == 0 &&
           p.live == 0 && p.first_live == 0;
}
static void stale(rsmi::CombinePlan* p) {  // contents that must not survive a refusal
    p->jobs.push_back(rsmi::CombineJob{0, 0, 1, 1, 0});
    p->addrs.push_back(16);
    p->coef.push_back(1);
    p->max_nsrc = p->max_nout = 9;
    p->rows = 3;
    p->ncols.push_back(7);
    p->first_block.push_back(5);
    p->mg = p->groups = p->iters = p->ncols_all = p->live = p->first_live = 2;
}

static int plan_of(const std::vector<Job>& jobs, const std::vector<size_t>& lens, rsmi::CombinePlan* p, uint32_t iters = 1) {
    const std::vector<rs_combine_job> v = view(jobs);
    stale(p);
    return rsmi::plan_combine_lens(v.data(), v.size(), lens.data(), p, iters);
}
static void accepted(const char* what, const std::vector<Job>& jobs, const std::vector<size_t>& lens) {
    rsmi::CombinePlan p;
    const int rc = plan_of(jobs, lens, &p);
    CHECK(rc == RS_OK, "%s: status %d", what, rc);
}
static void refused(const char* what, const std::vector<Job>& jobs, const std::vector<size_t>& lens) {
    rsmi::CombinePlan p;
    const int rc = plan_of(jobs, lens, &p);
    CHECK(rc == RS_EINVAL, "%s: status %d, want %d", what, rc, RS_EINVAL);
    CHECK(empty(p), "%s: plan not empty", what);
}

static size_t r16(size_t x) { return (x + 15) / 16 * 16; }

// `lens.size()` jobs of mixed shapes whose destinations are carved, one after
// another and each as long as its own job's span, from one region, and whose
// sources come from another.
static std::vector<Job> carve(const std::vector<size_t>& lens) {
    static const uint32_t shapes[][2] = {{1, 1}, {4, 2}, {10, 4}, {10, 5}, {3, 17}, {64, 16}, {200, 9}};
    const uint64_t A = 0x100000, D = 0x40000000;
    std::vector<Job> jobs;
    uint64_t at = D;
    for (size_t b = 0; b < lens.size(); ++b) {
        const uint32_t* sh = shapes[lens.size() > 100 ? 1 : rnd() % 7];
        std::vector<uint64_t> src, dst;
        for (uint32_t i = 0; i < sh[0]; ++i) src.push_back(A + 16ull * (rnd() % 4096));
        for (uint32_t i = 0; i < sh[1]; ++i) dst.push_back(at), at += std::max<size_t>(r16(lens[b]), 16);
        jobs.push_back(job(src, dst, rnd() & 1));
    }
    return jobs;
}

// Every block id maps, through the kernel's search, to a {job, chunk, group}
// such that the iterations the kernel then runs cover every (256-column
// chunk, row group) of every job that has columns exactly once, and nothing
// else.
static void partition(const char* what, const std::vector<size_t>& lens, uint32_t iters) {
    const std::vector<Job> jobs = carve(lens);
    rsmi::CombinePlan p;
    const int rc = plan_of(jobs, lens, &p, iters);
    CHECK(rc == RS_OK, "%s: status %d", what, rc);
    if (rc != RS_OK) return;
    bool any = false;
    for (size_t l : lens) any |= l != 0;
    if (!any) {
        CHECK(empty(p), "%s: all lengths 0, plan not empty", what);
        return;
    }
    const uint32_t njobs = static_cast<uint32_t>(lens.size());
    CHECK(p.jobs.size() == njobs && p.ncols.size() == njobs && p.first_block.size() == njobs + 1u, "%s: table sizes", what);
    if (p.jobs.size() != njobs || p.ncols.size() != njobs || p.first_block.size() != njobs + 1u) return;
    uint32_t max_nsrc = 0, max_nout = 0, live = 0, first_live = njobs;
    uint64_t rows = 0;
    for (uint32_t b = 0; b < njobs; ++b) {
        CHECK(p.ncols[b] == (lens[b] + 15) / 16, "%s: job %u has %u columns", what, b, p.ncols[b]);
        if (lens[b] == 0) continue;
        max_nsrc = std::max<uint32_t>(max_nsrc, jobs[b].src.size());
        max_nout = std::max<uint32_t>(max_nout, jobs[b].dst.size());
        rows += jobs[b].dst.size();
        if (live++ == 0) first_live = b;
    }
    CHECK(p.max_nsrc == max_nsrc && p.max_nout == max_nout && p.rows == rows && p.live == live && p.first_live == first_live,
          "%s: the jobs with bytes: %u x %u, %llu rows, %u live from %u", what, p.max_nout, p.max_nsrc,
          (unsigned long long)p.rows, p.live, p.first_live);
    const uint32_t mg = max_nout <= 4 ? 4 : max_nout <= 8 ? 8 : (max_nsrc > 199 ? 8 : 16);
    CHECK(p.mg == mg && p.groups == (max_nout + mg - 1) / mg && p.iters == iters, "%s: row groups of %u, %u of them", what, p.mg,
          p.groups);
    CHECK(p.first_block[0] == 0, "%s: first_block[0]", what);
    for (uint32_t b = 0; b < njobs; ++b) {
        CHECK(p.first_block[b] <= p.first_block[b + 1], "%s: prefix sum falls at %u", what, b);
        CHECK((p.first_block[b] == p.first_block[b + 1]) == (lens[b] == 0), "%s: job %u blocks", what, b);
    }
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, int> covered;  // {job, 256-column chunk, row group}
    const uint32_t blocks = p.first_block[njobs];
    for (uint32_t b = 0; b < blocks; ++b) {
        const rsmi::CombineBlock at = rsmi::combine_lens_block(p.first_block.data(), njobs, p.groups, b);
        if (at.job >= njobs) {
            CHECK(false, "%s: block %u maps to job %u", what, b, at.job);
            return;
        }
        CHECK(p.first_block[at.job] <= b && b < p.first_block[at.job + 1], "%s: block %u outside job %u", what, b, at.job);
        const uint32_t ncols = p.ncols[at.job];
        CHECK(ncols > 0, "%s: block %u maps to the empty job %u", what, b, at.job);
        CHECK(at.grp < p.groups && at.chunks == rsmi::combine_lens_chunks(ncols, iters) && at.chunk < at.chunks,
              "%s: block %u: group %u, chunk %u of %u", what, b, at.grp, at.chunk, at.chunks);
        // the kernel's loop: iteration `it` starts at column chunk * 256 + it * chunks * 256
        bool first = true;
        for (uint32_t it = 0; it < iters; ++it) {
            const uint64_t colbase = (static_cast<uint64_t>(at.chunk) + static_cast<uint64_t>(it) * at.chunks) * 256;
            if (colbase >= ncols) break;
            first = false;
            ++covered[std::make_tuple(at.job, static_cast<uint32_t>(colbase / 256), at.grp)];
        }
        CHECK(!first, "%s: block %u has no column", what, b);
    }
    uint64_t want = 0;
    for (uint32_t b = 0; b < njobs; ++b)
        for (uint32_t q = 0; q < (p.ncols[b] + 255) / 256; ++q)
            for (uint32_t g = 0; g < p.groups; ++g, ++want) {
                const auto f = covered.find(std::make_tuple(b, q, g));
                CHECK(f != covered.end() && f->second == 1, "%s: job %u chunk %u group %u covered %d times", what, b, q, g,
                      f == covered.end() ? 0 : f->second);
            }
    CHECK(covered.size() == want, "%s: %zu cells covered, %llu exist", what, covered.size(), (unsigned long long)want);
}

static size_t draw() {
    static const size_t fixed[] = {0, 1, 15, 16, 17, 4080, 4095, 4096, 4097, 4112, 8192, 12289};
    return rnd() % 3 ? fixed[rnd() % 12] : rnd() % 9001;
}

int main() {
    const uint64_t A = 0x100000, B = 0x200000, D = 0x800000;

    // the block map is a partition
    for (uint32_t iters : {1u, 3u}) {
        for (size_t count : {size_t(1), size_t(2), size_t(3), size_t(1500)})
            for (int rep = 0; rep < (count == 1500 ? 2 : 40); ++rep) {
                std::vector<size_t> lens(count);
                for (size_t& l : lens) l = draw();
                if (count == 1500) {  // runs of empty jobs at the start, in the middle and at the end
                    for (size_t b = 0; b < 7; ++b) lens[b] = lens[700 + b] = lens[count - 1 - b] = 0;
                    lens[7] = 12289, lens[count - 8] = 1;
                }
                partition("drawn", lens, iters);
            }
        // every fixed length next to an empty job, in either order and between two
        for (size_t l : {1, 15, 16, 17, 4080, 4095, 4096, 4097, 4112, 8192, 12289}) {
            partition("alone", {l}, iters);
            partition("empty first", {0, l}, iters);
            partition("empty last", {l, 0}, iters);
            partition("empty around", {0, l, 0}, iters);
            partition("empty between", {l, 0, l + 1}, iters);
        }
        partition("all empty", {0, 0, 0}, iters);
    }

    // equal lengths: plan_combine's plan, and one column count for all
    for (size_t len : {1, 16, 1000, 4096, 4097, 12289}) {
        const std::vector<Job> jobs = carve(std::vector<size_t>(9, len));
        const std::vector<rs_combine_job> v = view(jobs);
        rsmi::CombinePlan p, q;
        CHECK(rsmi::plan_combine(v.data(), v.size(), len, &q) == RS_OK, "plan_combine of %zu", len);
        CHECK(plan_of(jobs, std::vector<size_t>(9, len), &p) == RS_OK, "plan_combine_lens of %zu", len);
        bool same = p.jobs.size() == q.jobs.size() && p.addrs == q.addrs && p.coef == q.coef && p.max_nsrc == q.max_nsrc &&
                    p.max_nout == q.max_nout && p.rows == q.rows;
        for (size_t b = 0; same && b < p.jobs.size(); ++b)
            same = p.jobs[b].addr == q.jobs[b].addr && p.jobs[b].coef == q.jobs[b].coef && p.jobs[b].nsrc == q.jobs[b].nsrc &&
                   p.jobs[b].nout == q.jobs[b].nout && p.jobs[b].accumulate == q.jobs[b].accumulate;
        CHECK(same, "equal lengths of %zu: not plan_combine's plan", len);
        CHECK(p.ncols_all == (len + 15) / 16 && p.live == 9 && p.first_live == 0, "equal lengths of %zu: %u columns for all", len,
              p.ncols_all);
        CHECK(q.ncols.empty() && q.first_block.empty() && q.ncols_all == 0, "plan_combine fills no block map");
        // ... and lengths that differ are told apart, also when only an empty job differs
        std::vector<size_t> lens(9, len);
        lens[4] = len + 16;
        CHECK(plan_of(carve(lens), lens, &p) == RS_OK && p.ncols_all == 0, "one longer job");
        lens[4] = 0;
        CHECK(plan_of(carve(lens), lens, &p) == RS_OK && p.ncols_all == (len + 15) / 16 && p.live == 8, "one empty job");
    }

    // nothing to do
    {
        rsmi::CombinePlan p;
        stale(&p);
        CHECK(rsmi::plan_combine_lens(nullptr, 0, nullptr, &p) == RS_OK && empty(p), "count == 0");
        const std::vector<Job> jobs = {job({A}, {D}), job({A}, {D})};  // one dst twice: no ranges, no overlap
        CHECK(plan_of(jobs, {0, 0}, &p) == RS_OK && empty(p), "all lengths 0");
    }

    // refusals, each leaving the plan empty
    {
        const std::vector<Job> good = {job({A, B}, {D})};
        const std::vector<rs_combine_job> v = view(good);
        rsmi::CombinePlan p;
        stale(&p);
        CHECK(rsmi::plan_combine_lens(v.data(), 1, nullptr, &p) == RS_EINVAL && empty(p), "NULL lens");
        const size_t one = 1000;
        stale(&p);
        CHECK(rsmi::plan_combine_lens(nullptr, 1, &one, &p) == RS_EINVAL && empty(p), "NULL jobs");
        // 2^28 or more 16-byte columns (buffers 2^40 apart: no overlap at that length)
        const std::vector<Job> far = {job({16}, {1ull << 40}), job({32}, {1ull << 41})};
        refused("a length of 2^28 columns", far, {1000, size_t(1) << 32});
        refused("a length of 2^28 columns, less 15", far, {(size_t(1) << 32) - 15, 16});
        accepted("a length of 2^28 - 1 columns", far, {1000, (size_t(1) << 32) - 16});
        // more than 2^31 - 1 blocks in all: 4,096 jobs of 2^19 blocks each; one job fewer is served
        {
            std::vector<Job> big;
            for (uint64_t i = 0; i < 4096; ++i) big.push_back(job({16}, {(i + 1) << 32}));
            std::vector<size_t> lens(4096, size_t(1) << 31);
            refused("2^31 blocks", big, lens);
            lens[0] = 0;
            accepted("2^31 - 2^19 blocks", big, lens);
            lens[0] = (size_t(1) << 31) - 4096;
            accepted("2^31 - 1 blocks", big, lens);
        }
        // an empty job is validated like any other
        std::vector<Job> bad = {job({A}, {D}), job({A + 8}, {D + 4096})};
        refused("misaligned source of an empty job", bad, {1000, 0});
        bad[1] = job({A}, {D + 4096});
        bad[1].reserved = 1;
        refused("reserved of an empty job", bad, {1000, 0});
        bad[1] = job({A}, {D + 4096}, 2);
        refused("accumulate == 2 of an empty job", bad, {1000, 0});
        rs_combine_job two[2] = {v[0], v[0]};
        const size_t lens2[2] = {1000, 0};
        two[1].src = nullptr;
        stale(&p);
        CHECK(rsmi::plan_combine_lens(two, 2, lens2, &p) == RS_EINVAL && empty(p), "NULL src of an empty job");
        two[1] = v[0], two[1].nout = 257;
        stale(&p);
        CHECK(rsmi::plan_combine_lens(two, 2, lens2, &p) == RS_EINVAL && empty(p), "nout == 257 of an empty job");
    }

    // the overlap rule with a span per job
    {
        const size_t L = 100000, S = 1000;  // spans 100,000 and 1,008
        // ranges that touch are served; one column closer they are not
        accepted("short dst behind long dst", {job({A}, {D}), job({B}, {D + L})}, {L, S});
        refused("short dst in the long dst's last column", {job({A}, {D}), job({B}, {D + L - 16})}, {L, S});
        accepted("long dst behind short dst", {job({A}, {D}), job({B}, {D + 1008})}, {S, L});
        refused("long dst in the short dst's padding", {job({A}, {D}), job({B}, {D + 992})}, {S, L});
        // a dst of the long job meets a src of the short one far beyond the short one's span ...
        refused("short src deep inside the long dst", {job({A}, {D}), job({D + 50000}, {B})}, {L, S});
        refused("short src in the long dst's last column", {job({A}, {D}), job({D + L - 16}, {B})}, {L, S});
        accepted("short src right behind the long dst", {job({A}, {D}), job({D + L}, {B})}, {L, S});
        // ... the reverse is none: the same addresses with the lengths swapped
        accepted("long src far behind the short dst", {job({A}, {D}), job({D + 50000}, {B})}, {S, L});
        accepted("long src right behind the short dst", {job({A}, {D}), job({D + 1008}, {B})}, {S, L});
        refused("long src in the short dst's padding", {job({A}, {D}), job({D + 992}, {B})}, {S, L});
        // a long src that starts below a short dst and runs over it; a short one that ends before it
        refused("long src runs over the short dst", {job({A}, {D}), job({D - 50000}, {B})}, {S, L});
        accepted("short src ends before the long dst", {job({A}, {D}), job({D - 1008}, {B})}, {L, S});
        refused("short src ends in the long dst", {job({A}, {D}), job({D - 992}, {B})}, {L, S});
        accepted("long src ends at the short dst", {job({A}, {D}), job({D - L}, {B})}, {S, L});
        // within one job, and the destination list out of address order
        refused("src is dst", {job({D}, {D})}, {S});
        refused("unsorted dsts meet", {job({A}, {D + 2 * L}), job({A}, {D + L}), job({B}, {D + L + 1008 - 16})}, {S, S, L});
        accepted("unsorted dsts touch", {job({A}, {D + 2 * L + 1008}), job({A}, {D + L}), job({B}, {D + L + 1008})}, {S, S, L});
        // a long dst swallows a short one that starts behind another dst
        refused("long dst swallows a later short dst", {job({A}, {D}), job({A}, {D + 50000}), job({A}, {D + 20000})}, {L, S, S});
        // empty jobs contribute no ranges: what would overlap at any length is served
        accepted("empty job: src is dst", {job({A}, {D}), job({D + 16}, {D + 16})}, {L, 0});
        accepted("empty job: dst inside a dst", {job({A}, {D}), job({B}, {D + 32})}, {L, 0});
        accepted("empty job: dst is a src", {job({A}, {D}), job({B}, {A})}, {L, 0});
        accepted("empty job names the long one's dst", {job({A}, {D}), job({B}, {D})}, {0, L});
        refused("the same with a byte in it", {job({A}, {D}), job({B}, {D})}, {1, L});
    }
    std::printf("plan_combine_lens: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_combine_lens_standalone_sanitized(tmp_path):
    src = tmp_path / "combine_lens_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "combine_lens_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "combine_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_combine_lens: 0 failures" in run.stdout


def test_lens_entry_points_are_exported():
    import rsmi
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    for name in ("rs_combine_lens", "rs_encode_batch_lens", "rs_decode_batch_lens"):
        assert name in rsmi.EXPORTS and hasattr(lib, name)
    assert (rsmi.FEC.STAT_BATCH_LENS_PASSES, rsmi.FEC.STAT_COMBINE_LENS_LAUNCHES) == (24, 25)
    for name in ("combine_lens", "EncodeBatchLens", "DecodeBatchLens"):
        assert callable(getattr(rsmi.FEC, name))


def test_null_context_is_rejected_without_a_device():
    """rs_combine_lens, rs_encode_batch_lens and rs_decode_batch_lens refuse a
    NULL context with RS_EINVAL before touching HIP; callable on a CPU-only
    machine."""
    import rsmi
    lib = rsmi.load()
    arr = rsmi.combine_jobs([([16], [32], b"\x01", 0)])
    lens = (ctypes.c_size_t * 1)(16)
    assert lib.rs_combine_lens(None, arr, 1, lens, None) == rsmi.RS_EINVAL
    assert lib.rs_combine_lens(None, None, 0, None, None) == rsmi.RS_EINVAL
    assert lib.rs_combine_lens(None, arr, 1, None, None) == rsmi.RS_EINVAL
    st = (ctypes.c_int * 1)()
    ptrs = (ctypes.c_void_p * 1)(None)
    nums = (ctypes.c_int * 1)(0)
    assert lib.rs_encode_batch_lens(None, 1, ptrs, lens, ptrs, st) == rsmi.RS_EINVAL
    assert lib.rs_encode_batch_lens(None, 0, None, None, None, None) == rsmi.RS_EINVAL
    assert lib.rs_decode_batch_lens(None, 1, nums, nums, ptrs, lens, ptrs, st) == rsmi.RS_EINVAL
    assert lib.rs_decode_batch_lens(None, 0, None, None, None, None, None, None) == rsmi.RS_EINVAL
