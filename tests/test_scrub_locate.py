"""CPU: the scrub's locate step (csrc/scrub.cpp, rsmi::scrub_locate) and the
argument handling of rs_verify_stripes / rs_correct_stripes that needs no GPU.

The locate checks run in a stand-alone C++ program (its own main) built from
csrc/scrub.cpp and csrc/gf256.cpp with -fsanitize=address,undefined and run
directly: codewords come from systematic_matrix, errors and erasures from a
fixed-seed generator."""
import ctypes
import os
import subprocess

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gf256.hpp"
#include "scrub.hpp"

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

// One random codeword column of RS(k, n).
static std::vector<uint8_t> codeword(const std::vector<uint8_t>& enc, int k, int n) {
    std::vector<uint8_t> d(k), cw(n, 0);
    for (int j = 0; j < k; ++j) d[j] = static_cast<uint8_t>(rnd());
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) cw[i] ^= rsmi::gmul(enc[static_cast<size_t>(i) * k + j], d[j]);
    return cw;
}

// `count` distinct shard ids not flagged in used[]; flags them.
static std::vector<int> pick(int n, int count, std::vector<uint8_t>& used) {
    std::vector<int> ids;
    while (static_cast<int>(ids.size()) < count) {
        const int i = static_cast<int>(rnd() % n);
        if (used[i]) continue;
        used[i] = 1;
        ids.push_back(i);
    }
    return ids;
}

static void run_code(int k, int n) {
    const int m = n - k;
    const std::vector<uint8_t> enc = rsmi::systematic_matrix(k, n);
    // a clean column, nothing known: locates nothing
    {
        std::vector<uint8_t> ys = codeword(enc, k, n), known(n, 0);
        const int got = rsmi::scrub_locate(k, n, known.data(), ys.data());
        CHECK(got == 0, "RS(%d,%d) clean column: %d", k, n, got);
        for (int i = 0; i < n; ++i) CHECK(known[i] == 0, "clean column flagged shard %d", i);
    }
    // f errors and l erasures holding garbage, 2f + l <= m (l = 0: errors only)
    for (int l = 0; l <= m; ++l)
        for (int f = 0; 2 * f + l <= m; ++f) {
            if (m - l < 2) continue;  // radius 0 (reported as -1, checked below)
            for (int rep = 0; rep < 3; ++rep) {
                std::vector<uint8_t> ys = codeword(enc, k, n), used(n, 0), known(n, 0);
                const std::vector<int> er = pick(n, l, used), bad = pick(n, f, used);
                for (int i : er) {
                    known[i] = 1;
                    ys[i] = static_cast<uint8_t>(rnd());  // garbage: never read
                }
                for (int i : bad) ys[i] ^= static_cast<uint8_t>(1 + rnd() % 255);
                const int got = rsmi::scrub_locate(k, n, known.data(), ys.data());
                CHECK(got == f, "RS(%d,%d) l=%d f=%d: located %d", k, n, l, f, got);
                std::vector<uint8_t> want(n, 0);
                for (int i : er) want[i] = 1;
                for (int i : bad) want[i] = 1;
                for (int i = 0; i < n; ++i)
                    CHECK((known[i] != 0) == (want[i] != 0), "RS(%d,%d) l=%d f=%d: shard %d flag %d", k, n, l, f, i,
                          known[i]);
            }
        }
    // erasures that leave radius 0: -1, known unchanged
    if (m >= 1) {
        std::vector<uint8_t> ys = codeword(enc, k, n), used(n, 0), known(n, 0);
        for (int i : pick(n, m - 1, used)) known[i] = 1;
        const std::vector<uint8_t> before = known;
        ys[pick(n, 1, used)[0]] ^= 0x5A;
        CHECK(rsmi::scrub_locate(k, n, known.data(), ys.data()) == -1, "RS(%d,%d) radius 0 with erasures", k, n);
        CHECK(known == before, "known changed on failure");
    }
}

int main() {
    run_code(4, 6);
    run_code(10, 14);
    run_code(64, 80);
    // RS(4,5): radius 0, one error -> -1
    {
        const std::vector<uint8_t> enc = rsmi::systematic_matrix(4, 5);
        std::vector<uint8_t> ys = codeword(enc, 4, 5), known(5, 0);
        ys[2] ^= 0x01;
        CHECK(rsmi::scrub_locate(4, 5, known.data(), ys.data()) == -1, "RS(4,5) one error");
        for (int i = 0; i < 5; ++i) CHECK(known[i] == 0, "RS(4,5) flagged shard %d", i);
    }
    // more errors than the radius: never reports success with the true set
    {
        const std::vector<uint8_t> enc = rsmi::systematic_matrix(10, 14);
        int rejected = 0;
        for (int rep = 0; rep < 20; ++rep) {
            std::vector<uint8_t> ys = codeword(enc, 10, 14), used(14, 0), known(14, 0);
            for (int i : pick(14, 3, used)) ys[i] ^= static_cast<uint8_t>(1 + rnd() % 255);
            const int got = rsmi::scrub_locate(10, 14, known.data(), ys.data());
            CHECK(got == -1 || (got >= 1 && got <= 2), "RS(10,14) 3 errors: %d", got);
            rejected += got == -1;
        }
        CHECK(rejected > 0, "3 errors were never rejected");
    }
    std::printf("scrub_locate: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_scrub_locate_standalone_sanitized(tmp_path):
    src = tmp_path / "scrub_locate_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "scrub_locate_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "scrub.cpp"),
                    os.path.join(CSRC, "gf256.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "scrub_locate: 0 failures" in run.stdout


def test_scrub_entry_points_are_exported():
    import rsmi
    assert "rs_verify_stripes" in rsmi.EXPORTS
    assert "rs_correct_stripes" in rsmi.EXPORTS
    assert rsmi.RS_VERIFY_CLEAN == 0xFFFFFFFF
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    assert hasattr(lib, "rs_verify_stripes") and hasattr(lib, "rs_correct_stripes")


def test_null_context_is_rejected_without_a_device():
    """Both scrub entry points refuse a NULL context with RS_EINVAL before
    touching HIP; callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    st = (ctypes.c_int * 1)()
    assert lib.rs_verify_stripes(None, None, 0, None, 0, 16, 16, 1, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_stripes(None, None, 0, None, 0, 16, 16, 1, st, None, None) == rsmi.RS_EINVAL
