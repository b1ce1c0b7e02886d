"""CPU: the per-column decoder of rs_correct_columns (csrc/column_decode.hpp,
the core the kernel shares with the host) against the engine's Berlekamp-Welch
(rsmi::bw_column, infectious Correct): the same corrected column, or both fail.

The checks run in a stand-alone C++ program (its own main) built from
csrc/column_decode.cpp + csrc/gf256.cpp with -fsanitize=address,undefined and
run directly."""
import ctypes
import os
import subprocess

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "column_decode.hpp"
#include "gf256.hpp"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
}

static int failures = 0;
static long columns = 0, both_failed = 0, shard0 = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 40) {                       \
                std::printf("FAIL %s:%d: ", #cond, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

// A random codeword on the share numbers nums: P(x_i), deg P < k.
static std::vector<uint8_t> codeword(int k, const std::vector<int>& nums) {
    std::vector<uint8_t> p(k), y(nums.size());
    for (auto& c : p) c = static_cast<uint8_t>(rnd());
    for (size_t i = 0; i < nums.size(); ++i) {
        const uint8_t x = rsmi::eval_point(nums[i]);
        uint8_t v = 0;
        for (int d = k - 1; d >= 0; --d) v = rsmi::gmul(v, x) ^ p[d];
        y[i] = v;
    }
    return y;
}

// One received column: the core (through its host twin) against bw_column.
static void one(const char* what, int k, int n, const std::vector<int>& nums, const std::vector<uint8_t>& sent,
                const std::vector<int>& where, int radius) {
    const int r = static_cast<int>(nums.size());
    std::vector<uint8_t> ys = sent;
    for (int w : where) ys[w] ^= static_cast<uint8_t>(1 + rnd() % 255);
    for (int w : where) shard0 += nums[w] == 0;
    std::vector<uint8_t> out(n), mine = ys;
    const int ref = rsmi::bw_column(k, n, nums.data(), ys.data(), r, out.data());
    const int got = rsmi::column_correct(k, n, nums.data(), mine.data(), r);
    ++columns;
    const int weight = static_cast<int>(where.size());
    if (weight <= radius) {
        CHECK(got == weight, "%s weight %d: corrected %d", what, weight, got);
        CHECK(mine == sent, "%s weight %d: not the sent codeword", what, weight);
    }
    if (ref < 0) {
        ++both_failed;
        CHECK(got < 0, "%s weight %d: bw_column fails, the core corrects %d", what, weight, got);
        CHECK(mine == ys, "%s weight %d: a failed column was written", what, weight);
        return;
    }
    CHECK(got == ref, "%s weight %d: bw_column changes %d, the core %d", what, weight, ref, got);
    for (int i = 0; i < r; ++i)
        if (mine[i] != out[nums[i]]) {
            CHECK(false, "%s weight %d: share %d is %u, bw_column has %u", what, weight, nums[i], mine[i], out[nums[i]]);
            break;
        }
}

static std::vector<int> present(int n, const std::vector<int>& gone) {
    std::vector<int> nums;
    for (int i = 0; i < n; ++i)
        if (std::find(gone.begin(), gone.end(), i) == gone.end()) nums.push_back(i);
    return nums;
}

// Every error position set of every weight 0 .. r - k, `tuples` value tuples each.
static void exhaustive(const char* what, int k, int n, const std::vector<int>& gone, int tuples) {
    const std::vector<int> nums = present(n, gone);
    const int r = static_cast<int>(nums.size()), d = r - k;
    for (uint32_t mask = 0; mask < (1u << r); ++mask) {
        if (__builtin_popcount(mask) > d) continue;
        std::vector<int> where;
        for (int i = 0; i < r; ++i)
            if (mask >> i & 1u) where.push_back(i);
        for (int v = 0; v < tuples; ++v) one(what, k, n, nums, codeword(k, nums), where, d / 2);
    }
}

// `reps` seeded columns of every weight 0 .. radius + 2; the first of each
// weight > 0 has an error on shard 0 when that shard is present.
static void sampled(const char* what, int k, int n, const std::vector<int>& gone, int reps) {
    const std::vector<int> nums = present(n, gone);
    const int r = static_cast<int>(nums.size()), d = r - k;
    for (int weight = 0; weight <= d / 2 + 2 && weight <= r; ++weight)
        for (int rep = 0; rep < reps; ++rep) {
            std::vector<int> where;
            if (weight > 0 && rep == 0 && nums[0] == 0) where.push_back(0);
            while (static_cast<int>(where.size()) < weight) {
                const int w = static_cast<int>(rnd() % r);
                if (std::find(where.begin(), where.end(), w) == where.end()) where.push_back(w);
            }
            one(what, k, n, nums, codeword(k, nums), where, d / 2);
        }
}

// Seeded erasure sets of 1 .. m - 2 shards.  Of each size: a plain one, one
// that holds shard 0, one that holds shard n - 1 and one that holds both --
// or, for the wide codes (every_kind false), one of the four in turn.  sizes:
// the sizes to take (empty: every size).
static std::vector<std::vector<int>> erasure_sets(int n, int m, bool every_kind, const std::vector<int>& sizes = {}) {
    std::vector<std::vector<int>> sets;
    for (int e = 1; e <= m - 2; ++e)
        for (int kind = 0; kind < 4; ++kind) {
            if (!every_kind && kind != e % 4) continue;
            if (!sizes.empty() && std::find(sizes.begin(), sizes.end(), e) == sizes.end()) continue;
            std::vector<int> gone;
            if (kind == 1 || kind == 3) gone.push_back(0);
            if ((kind == 2 || kind == 3) && static_cast<int>(gone.size()) < e) gone.push_back(n - 1);
            while (static_cast<int>(gone.size()) < e) {
                const int id = static_cast<int>(rnd() % n);
                if (std::find(gone.begin(), gone.end(), id) == gone.end()) gone.push_back(id);
            }
            sets.push_back(gone);
        }
    return sets;
}

int main() {
    // the tables: u_i is the dual multiplier, W[t][i] = u_i x_i^t, zero past r and d
    {
        const int n = 14;
        std::vector<uint8_t> er(n, 0), tab(rsmi::column_table_bytes(n));
        er[0] = er[7] = 1;
        const int r = rsmi::column_tables(n, er.data(), tab.data());
        const size_t np = rsmi::column_table_pitch(n);
        CHECK(r == 12 && np == 16, "tables: r %d, pitch %zu", r, np);
        const std::vector<int> nums = present(n, {0, 7});
        for (int i = 0; i < r; ++i) {
            CHECK(tab[i] == nums[i] && tab[np + i] == rsmi::eval_point(nums[i]), "tables: id / point %d", i);
            uint8_t prod = 1;
            for (int j = 0; j < r; ++j)
                if (j != i) prod = rsmi::gmul(prod, tab[np + i] ^ tab[np + j]);
            CHECK(rsmi::gmul(prod, tab[2 * np + i]) == 1, "tables: u_%d", i);
            uint8_t p = tab[2 * np + i];
            for (int t = 0; t < rsmi::kColumnMaxSyn; ++t) {
                CHECK(tab[(3 + t) * np + i] == p, "tables: W[%d][%d]", t, i);
                p = rsmi::gmul(p, tab[np + i]);
            }
        }
        for (size_t row = 0; row < 3 + rsmi::kColumnMaxSyn; ++row)
            for (size_t i = r; i < np; ++i) CHECK(tab[row * np + i] == 0, "tables: pad of row %zu", row);
        // every codeword of the punctured code has zero syndromes
        const std::vector<uint8_t> y = codeword(10, nums);
        for (int t = 0; t < r - 10; ++t) {
            uint8_t s = 0;
            for (int i = 0; i < r; ++i) s ^= rsmi::gmul(tab[(3 + t) * np + i], y[i]);
            CHECK(s == 0, "tables: syndrome %d of a codeword is %u", t, s);
        }
    }
    // trivial cases of the twin
    {
        const int nums[5] = {0, 1, 2, 3, 4};
        uint8_t ys[5] = {9, 8, 7, 6, 5};
        CHECK(rsmi::column_correct(5, 5, nums, ys, 5) == 0, "r == k");
        std::vector<int> n5 = {0, 1, 2, 3, 4};
        std::vector<uint8_t> cw = codeword(4, n5);
        CHECK(rsmi::column_correct(4, 5, nums, cw.data(), 5) == 0, "r - k == 1, a codeword");
        cw[2] ^= 1;
        const std::vector<uint8_t> before = cw;
        CHECK(rsmi::column_correct(4, 5, nums, cw.data(), 5) == -1 && cw == before, "r - k == 1, inconsistent");
    }
    exhaustive("RS(4,6)", 4, 6, {}, 64);
    exhaustive("RS(3,9)", 3, 9, {}, 64);
    for (const auto& gone : erasure_sets(9, 6, true)) exhaustive("RS(3,9) degraded", 3, 9, gone, 64);
    struct Code {
        const char* name;
        int k, n, reps, reps_degraded;
    };
    const Code codes[] = {{"RS(10,14)", 10, 14, 200, 50}, {"RS(64,80)", 64, 80, 4, 1},
                          {"RS(3,19)", 3, 19, 200, 20}, {"RS(240,256)", 240, 256, 1, 1}};
    for (const Code& c : codes) {
        sampled(c.name, c.k, c.n, {}, c.reps);
        // RS(240,256), whose bw_column solves 256 x 257 systems: sets of 1 (shard 0), 2 (shard 255), 7 (both)
        // and m - 2 = 14 (shard 255) shards
        const std::vector<int> sizes = c.n == 256 ? std::vector<int>{1, 2, 7, 14} : std::vector<int>{};
        for (const auto& gone : erasure_sets(c.n, c.n - c.k, c.n < 80, sizes)) sampled(c.name, c.k, c.n, gone, c.reps_degraded);
    }
    CHECK(both_failed > 1000, "only %ld columns beyond the radius failed in both", both_failed);
    CHECK(shard0 > 1000, "only %ld errors on shard 0", shard0);
    std::printf("column_decode: %ld columns, %ld failed in both, %d failures\n", columns, both_failed, failures);
    return failures ? 1 : 0;
}
"""


def test_decoder_core_matches_bw_column_standalone_sanitized(tmp_path):
    src = tmp_path / "column_decode_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "column_decode_test"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "column_decode.cpp"),
                    os.path.join(CSRC, "gf256.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout


def test_column_entry_point_is_exported():
    import rsmi
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    assert "rs_correct_columns" in rsmi.EXPORTS
    assert hasattr(lib, "rs_correct_columns")
    assert (rsmi.FEC.STAT_COLUMN_STRIPES, rsmi.FEC.STAT_COLUMN_BYTES) == (22, 23)
    assert hasattr(rsmi.FEC, "correct_columns")


def test_null_context_is_rejected_without_a_device():
    """A NULL context is RS_EINVAL before HIP is touched; callable on a
    CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    st = (ctypes.c_int * 1)()
    assert lib.rs_correct_columns(None, None, 0, None, 0, 16, 16, 1, None, st, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_columns(None, None, 0, None, 0, 16, 16, 0, None, None, None, None) == rsmi.RS_EINVAL
