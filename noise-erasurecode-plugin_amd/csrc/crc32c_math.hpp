// crc32c_math.hpp -- CRC-32C (Castagnoli, RFC 3720) as arithmetic in
// GF(2)[x] / P, shared by the host reference (crc32c_host.cpp) and the device
// kernel (crc32c.hip).  Everything is in the reflected representation the CRC
// is defined in: bit 31 of a word is the coefficient of x^0, bit 0 that of
// x^31, and P is 0x82F63B78.  Pure constexpr: no HIP, no state.
//
// With f(M) the register after the bytes of M from a zero register and no
// final XOR, and shift(s, L) = s * x^(8L) mod P (the register after L zero
// bytes from s):
//     f(A || B) = shift(f(A), |B|) ^ f(B)
//     crc32c(M) = f(M) ^ shift(0xFFFFFFFF, |M|) ^ 0xFFFFFFFF
// so a message is cut into pieces whose f are computed independently and
// combined by multiplications with constants.
#pragma once

#include <cstdint>

namespace rsmi {

constexpr uint32_t kCrcPoly = 0x82F63B78u;
constexpr uint32_t kCrcOne = 0x80000000u;  // the polynomial 1

// a * b mod P.
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
    }
    return p;
}

constexpr uint32_t crc_powmod(uint32_t base, uint64_t e) {
    uint32_t r = kCrcOne;
    while (e) {
        if (e & 1u) r = crc_mulmod(r, base);
        base = crc_mulmod(base, base);
        e >>= 1;
    }
    return r;
}

// x^(8 * nbytes) mod P: shift(s, nbytes) = crc_mulmod(s, crc_xpow8(nbytes)).
constexpr uint32_t crc_xpow8(uint64_t nbytes) { return crc_powmod(kCrcOne >> 8, nbytes); }

// x^(-8 * nbytes) mod P.  P has a constant term, so x is a unit: x^-1 is
// (P - 1) / x, the step of crc_mulmod run backwards on 1.
constexpr uint32_t crc_xinv8(uint64_t nbytes) {
    constexpr uint32_t xinv = ((kCrcOne ^ kCrcPoly) << 1) | 1u;
    return crc_powmod(crc_powmod(xinv, 8), nbytes);
}

// The term of the initial value and the final XOR for a message of nbytes.
constexpr uint32_t crc_init_term(uint64_t nbytes) { return crc_mulmod(0xFFFFFFFFu, crc_xpow8(nbytes)) ^ 0xFFFFFFFFu; }

constexpr int kCrcSlices = 16;   // slice-by-16 on the device, the first 8 on the host
constexpr int kCrcStrides = 4;   // lane-group strides of 128, 256, 512 and 1024 bytes
constexpr int kCrcLanes = 64;

struct CrcTables {
    // slice[j][b] = f(b followed by j zero bytes): f of a 16-byte word is the
    // XOR of slice[15 - i][byte i].
    uint32_t slice[kCrcSlices][256];
    // stride[s][i][b] = (b << 8i) * x^(8 * (128 << s)): four lookups multiply a
    // register by the constant of a lane group's stride.
    uint32_t stride[kCrcStrides][4][256];
    // pos[i] = x^(128 i): the weight of a lane that sits i 16-byte words before
    // the end of its group.
    uint32_t pos[kCrcLanes];
};

constexpr CrcTables make_crc_tables() {
    CrcTables t{};
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t c = b;
        for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
        t.slice[0][b] = c;
    }
    for (int j = 1; j < kCrcSlices; ++j)
        for (uint32_t b = 0; b < 256; ++b)
            t.slice[j][b] = (t.slice[j - 1][b] >> 8) ^ t.slice[0][t.slice[j - 1][b] & 0xFFu];
    for (int s = 0; s < kCrcStrides; ++s) {
        const uint32_t c = crc_xpow8(uint64_t(128) << s);
        for (int i = 0; i < 4; ++i) {
            // linear in b: the eight one-bit values, then XORs
            for (uint32_t b = 1; b < 256; ++b) {
                const uint32_t low = b & (0u - b);
                t.stride[s][i][b] = low == b ? crc_mulmod(b << (8 * i), c) : t.stride[s][i][b ^ low] ^ t.stride[s][i][low];
            }
        }
    }
    const uint32_t w = crc_xpow8(16);
    t.pos[0] = kCrcOne;
    for (int i = 1; i < kCrcLanes; ++i) t.pos[i] = crc_mulmod(t.pos[i - 1], w);
    return t;
}

}  // namespace rsmi
