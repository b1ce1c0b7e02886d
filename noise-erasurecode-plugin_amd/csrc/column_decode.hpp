// column_decode.hpp -- the per-column decoder of rs_correct_columns: bounded-
// distance decoding of one byte column of a stripe from its syndromes.
//
// The core (column_decode_core) is shared by the host twin (column_decode.cpp)
// and the kernel (column_correct.hip): RSMI_HD is __host__ __device__ under
// hipcc and empty under g++.
//
// The code on the present set P (r shares, points x_i = eval_point(id_i)) is
// a generalised Reed-Solomon code of dimension k; with the dual multipliers
//     u_i = 1 / prod_{j in P, j != i} (x_i ^ x_j)
// the d = r - k syndromes of a received column y are
//     S_t = sum_{i in P} u_i x_i^t y_i,   t = 0 .. d - 1   (0^0 = 1),
// all zero exactly for codewords.  An error e_a at point X_a adds
// Y_a X_a^t to S_t with Y_a = u_a e_a, so S is a sum of nu geometric
// sequences, and its shortest linear recurrence has the characteristic
// polynomial Lambda(x) = prod (x - X_a) -- in root form, because shard 0 sits
// at x = 0 and an error there shows in S_0 only.  The core finds that
// recurrence by Berlekamp-Massey, requires length nu <= d / 2 and nu distinct
// roots among the present points, solves the nu x nu Vandermonde system for
// the Y_a, requires them non-zero and that they explain all d syndromes (one
// error is found in closed form ahead of all that: X = S_1 / S_0).  A
// codeword within d / 2 of y is unique, so the result is that of any exact
// bounded-distance decoder (gf256.cpp bw_column): the same errors, or failure.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RSMI_HD __host__ __device__
#else
#define RSMI_HD
#endif

namespace rsmi {

constexpr int kColumnMaxSyn = 16;  // d = r - k served: codes with m <= 16
constexpr int kColumnMaxErr = 8;   // nu <= d / 2
// Bytes of workspace column_decode_core needs (one slice per lane in LDS, or
// the host's stack): S [16] | C [9] | B [9] | T [9] | pos [8] | X [8] | A [8][9].
constexpr int kColumnWork = 144;
constexpr int kColumnWsS = 0, kColumnWsC = 16, kColumnWsB = 25, kColumnWsT = 34, kColumnWsPos = 43,
              kColumnWsX = 51, kColumnWsA = 59;
static_assert(kColumnWsA + kColumnMaxErr * (kColumnMaxErr + 1) <= kColumnWork, "workspace layout");

// exp[512] (so the sum of two logs needs no reduction) and log[256].
struct ColumnGf {
    const uint8_t* exp;
    const uint8_t* log;
};

RSMI_HD inline uint32_t cg_mul(const ColumnGf& g, uint32_t a, uint32_t b) {
    if (a == 0u || b == 0u) return 0u;
    return g.exp[static_cast<uint32_t>(g.log[a]) + g.log[b]];
}
RSMI_HD inline uint32_t cg_div(const ColumnGf& g, uint32_t a, uint32_t b) {  // b != 0
    if (a == 0u) return 0u;
    return g.exp[static_cast<uint32_t>(g.log[a]) + 255u - g.log[b]];
}

// Decodes the column whose d syndromes are ws[kColumnWsS ..] (2 <= d <= 16;
// untouched).  x[r] / u[r]: the points and dual multipliers of the present
// shares.  Returns the number of errors nu (0 for a codeword), with their
// indices into the present list at ws[kColumnWsPos ..] and their values e_a
// (received ^ e_a is the codeword's byte) at ws[kColumnWsX ..], or -1 when no
// codeword lies within d / 2.
RSMI_HD inline int column_decode_core(const ColumnGf& g, const uint8_t* x, const uint8_t* u, int r, int d,
                                      uint8_t* ws) {
    const uint8_t* S = ws + kColumnWsS;
    uint8_t* C = ws + kColumnWsC;
    uint8_t* B = ws + kColumnWsB;
    uint8_t* T = ws + kColumnWsT;
    uint8_t* pos = ws + kColumnWsPos;
    uint8_t* X = ws + kColumnWsX;
    uint8_t* A = ws + kColumnWsA;
    const int radius = d / 2;
    uint32_t any = 0;
    for (int t = 0; t < d; ++t) any |= S[t];
    if (any == 0u) return 0;

    // One error -- the common case -- in closed form: S_t = Y X^t with Y = S_0
    // (non-zero) and X = S_1 / S_0.  The recurrence below would find the same
    // length-1 locator, so an X that is no present point is a failure here too.
    if (d >= 2 && S[0] != 0) {
        const uint32_t x1 = cg_div(g, S[1], S[0]);
        uint32_t p = S[0];
        bool one = true;
        for (int t = 1; t < d && one; ++t) {
            p = cg_mul(g, p, x1);
            one = p == S[t];
        }
        if (one) {
            for (int i = 0; i < r; ++i)
                if (x[i] == x1) {
                    pos[0] = static_cast<uint8_t>(i);
                    X[0] = static_cast<uint8_t>(cg_div(g, S[0], u[i]));
                    return 1;
                }
            return -1;
        }
    }

    // Berlekamp-Massey: C(z) = 1 + c_1 z + .. + c_L z^L with
    // sum_{j <= L} c_j S_{i-j} = 0 for L <= i < d.  A length beyond the radius
    // is a failure, so the coefficients past it are never kept.
    for (int j = 0; j <= kColumnMaxErr; ++j) C[j] = B[j] = 0;
    C[0] = B[0] = 1;
    int L = 0, gap = 1;
    uint32_t b = 1;
    for (int i = 0; i < d; ++i) {
        uint32_t delta = S[i];
        for (int j = 1; j <= L; ++j) delta ^= cg_mul(g, C[j], S[i - j]);
        if (delta == 0u) {
            ++gap;
            continue;
        }
        const uint32_t f = cg_div(g, delta, b);
        if (2 * L <= i) {
            const int nl = i + 1 - L;
            if (nl > radius) return -1;  // L only grows
            for (int j = 0; j <= kColumnMaxErr; ++j) T[j] = C[j];
            for (int j = 0; j + gap <= kColumnMaxErr; ++j) C[j + gap] ^= cg_mul(g, f, B[j]);
            for (int j = 0; j <= kColumnMaxErr; ++j) B[j] = T[j];
            L = nl;
            b = delta;
            gap = 1;
        } else {
            for (int j = 0; j + gap <= kColumnMaxErr; ++j) C[j + gap] ^= cg_mul(g, f, B[j]);
            ++gap;
        }
    }
    if (L == 0 || L > radius) return -1;

    // Roots of Lambda(x) = x^L + c_1 x^(L-1) + .. + c_L among the present
    // points: exactly L of them.
    int nu = 0;
    for (int i = 0; i < r; ++i) {
        const uint32_t xi = x[i];
        uint32_t v = 1;
        for (int j = 1; j <= L; ++j) v = cg_mul(g, v, xi) ^ C[j];
        if (v != 0u) continue;
        if (nu == L) return -1;
        pos[nu] = static_cast<uint8_t>(i);
        X[nu] = static_cast<uint8_t>(xi);
        ++nu;
    }
    if (nu != L) return -1;

    // sum_a Y_a X_a^t = S_t for t < nu: Gauss-Jordan on the augmented
    // Vandermonde matrix (the X_a are distinct, so it is regular).
    const int w = kColumnMaxErr + 1;
    for (int a = 0; a < nu; ++a) {
        uint32_t p = 1;
        for (int t = 0; t < nu; ++t) {
            A[t * w + a] = static_cast<uint8_t>(p);
            p = cg_mul(g, p, X[a]);
        }
    }
    for (int t = 0; t < nu; ++t) A[t * w + nu] = S[t];
    for (int col = 0; col < nu; ++col) {
        int pr = col;
        while (pr < nu && A[pr * w + col] == 0) ++pr;
        if (pr == nu) return -1;
        if (pr != col)
            for (int j = 0; j <= nu; ++j) {
                const uint8_t tmp = A[pr * w + j];
                A[pr * w + j] = A[col * w + j];
                A[col * w + j] = tmp;
            }
        const uint32_t pv = A[col * w + col];
        for (int j = 0; j <= nu; ++j) A[col * w + j] = static_cast<uint8_t>(cg_div(g, A[col * w + j], pv));
        for (int i = 0; i < nu; ++i) {
            const uint32_t fac = A[i * w + col];
            if (i == col || fac == 0u) continue;
            for (int j = 0; j <= nu; ++j) A[i * w + j] ^= static_cast<uint8_t>(cg_mul(g, fac, A[col * w + j]));
        }
    }
    // Every Y_a non-zero, and together they explain all d syndromes.
    for (int a = 0; a < nu; ++a)
        if (A[a * w + nu] == 0) return -1;
    for (int a = 0; a < nu; ++a) T[a] = A[a * w + nu];  // Y_a X_a^t, t running
    for (int t = 0; t < d; ++t) {
        uint32_t s = 0;
        for (int a = 0; a < nu; ++a) {
            s ^= T[a];
            T[a] = static_cast<uint8_t>(cg_mul(g, T[a], X[a]));
        }
        if (s != S[t]) return -1;
    }
    // e_a = Y_a / u_a (u_a is never zero).
    for (int a = 0; a < nu; ++a) X[a] = static_cast<uint8_t>(cg_div(g, A[a * w + nu], u[pos[a]]));
    return nu;
}

// ------------------------------------------------------------ host twin ----
// The tables of one erasure set, as the kernel reads them: np = n rounded up
// to 16 bytes per row,
//     ids [np] | x [np] | u [np] | W [kColumnMaxSyn][np],   W[t][i] = u_i x_i^t,
// over the r present shards in id order (entries past r, and rows past d, are
// zero).
inline size_t column_table_pitch(int n) { return (static_cast<size_t>(n) + 15) / 16 * 16; }
inline size_t column_table_bytes(int n) { return (3 + kColumnMaxSyn) * column_table_pitch(n); }
// Fills out[column_table_bytes(n)] for the erasure flags erased[n] (nullptr:
// none) and returns r, the number of present shards.
int column_tables(int n, const uint8_t* erased, uint8_t* out);

// Host twin of the kernel on one column: nums[r] distinct share numbers below
// n with received bytes ys[r], corrected in place.  Returns the number of
// bytes changed, or -1 (ys untouched) when no codeword lies within
// (r - k) / 2 -- always, for an inconsistent column, when r - k < 2.  Serves
// r - k <= kColumnMaxSyn.
int column_correct(int k, int n, const int* nums, uint8_t* ys, int r);

}  // namespace rsmi
