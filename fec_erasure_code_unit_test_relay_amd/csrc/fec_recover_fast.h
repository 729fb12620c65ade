// fec_recover_fast.h -- index arithmetic and the packed GF(2^8) tables of the specialised recovery
// kernel (fec_recover_fast.hip), host and device: the kernel computes its spans, source offsets and
// tables through these functions, and the host exports them (fec_recover_fast_items,
// fec_recover_fast_mul) so that the bounds and the products are checked on the CPU.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fec {

constexpr int kRecFastStageChunks = 12;  // 16-byte pieces per lane of a staged span
constexpr int kRecFastStageMax = kRecFastStageChunks * 64 * 16;  // staging limit: 12 KB per wave
constexpr int kRecFastWaveRows = 16;     // one wave per this many output rows of the call ...
constexpr int kRecFastMaxWaves = 4096;   // ... up to this many (one workgroup = one wave)

// Bytes of the span a recovered packet may touch, at its widest (k+n-1 rows, the 16-byte round-down
// in front and the round-up behind): the kernel applies when this fits the staging limit.
__host__ __device__ inline int rec_fast_span_max(int k, int n, int CW) { return (k + n - 1) * CW + 32; }

__host__ __device__ inline int rec_fast_waves(int64_t Pout) {
    const int64_t w = (Pout + kRecFastWaveRows - 1) / kRecFastWaveRows;
    return static_cast<int>(w < 1 ? 1 : (w > kRecFastMaxWaves ? kRecFastMaxWaves : w));
}

// Packet x's diagonals touch codeword rows x-k+1 .. x+n-1; inside [0, P) these are rows
// [rlo, rhi), bytes [s0, s1) of the codeword buffer.  The wave stages the 16-byte pieces
// a0 + 16 c, c < nb, of the buffer (a0 = s0 rounded down to 16; the last piece is cut at the
// buffer's end P * CW): byte o of the buffer lands at LDS offset o - a0.
struct RecFastSpan {
    int rlo, rhi;
    int64_t s0, s1, a0;
    int nb;
};
__host__ __device__ inline RecFastSpan rec_fast_span(int64_t x, int k, int n, int CW, int64_t P) {
    RecFastSpan sp;
    sp.rlo = static_cast<int>(x - k + 1 > 0 ? x - k + 1 : 0);
    sp.rhi = static_cast<int>(x + n < P ? x + n : P);
    sp.s0 = static_cast<int64_t>(sp.rlo) * CW;
    sp.s1 = static_cast<int64_t>(sp.rhi) * CW;
    sp.a0 = sp.s0 & ~int64_t(15);
    sp.nb = static_cast<int>((sp.s1 - sp.a0 + 15) >> 4);
    return sp;
}

// Item `it` = g * k + i of packet x: position i, sub-streams 4g .. 4g+ne-1 (ne < 4 in the last
// group when S % 4).  Output byte e is h = (4g+e) * k + i of [len_hi, len_lo, payload] (written
// when h < L + 2).  Term q is present for q in [qlo, qhi) (row x-i+q inside [0, P)); its source
// byte e sits at staged offset base + q * (CW + 1) + e * n.
struct RecFastItem {
    int i, g, ne, qlo, qhi, base;
};
__host__ __device__ inline RecFastItem rec_fast_item(const RecFastSpan& sp, int64_t x, int it, int k, int n, int S,
                                                     int CW, int64_t P) {
    RecFastItem m;
    m.g = it / k;
    m.i = it - m.g * k;
    m.ne = S - 4 * m.g < 4 ? S - 4 * m.g : 4;
    m.qlo = static_cast<int>(m.i - x > 0 ? m.i - x : 0);
    const int64_t qh = P - x + m.i;
    m.qhi = static_cast<int>(qh < n ? (qh > 0 ? qh : 0) : n);
    m.base = static_cast<int>((x - m.i - sp.rlo) * CW + (sp.s0 - sp.a0)) + 4 * m.g * n;
    return m;
}

// ---- packed product --------------------------------------------------------------------------
// x -> 2x in GF(2^8) (poly 0x11d) on four packed bytes.
__host__ __device__ inline uint32_t gf_double4(uint32_t v) {
    const uint32_t hi = (v >> 7) & 0x01010101u;
    return ((v & 0x7f7f7f7fu) << 1) ^ (hi * 0x1du);
}
__host__ __device__ inline uint32_t splat_byte1(uint32_t v) {  // byte 1 of v in all four bytes
    const uint32_t b = (v >> 8) & 0xffu;
    const uint32_t h = b | (b << 8);
    return h | (h << 16);
}
// The five registers of gf_mul4x (fec_device.h) for the constant c, by packed doubling:
// tab[0..1] = c*{0..7}, tab[2..3] = c*({0..7}<<3), tab[4] = c*({0..3}<<6).
__host__ __device__ inline void gf_mul4x_tables(uint32_t c, uint32_t tab[5]) {
    c &= 0xffu;
    const uint32_t c2 = gf_double4(c);
    const uint32_t t0 = (c << 8) | (c2 << 16) | ((c ^ c2) << 24);  // c * {0, 1, 2, 3}
    const uint32_t t4 = gf_double4(gf_double4(t0));                 // c * {0, 4, 8, 12}
    const uint32_t t8 = gf_double4(t4);                             // c * {0, 8, 16, 24}
    const uint32_t t32 = gf_double4(gf_double4(t8));                // c * {0, 32, 64, 96}
    const uint32_t t64 = gf_double4(t32);                           // c * {0, 64, 128, 192}
    tab[0] = t0;
    tab[1] = t0 ^ splat_byte1(t4);
    tab[2] = t8;
    tab[3] = t8 ^ splat_byte1(t32);
    tab[4] = t64;
}
// gf_mul4x without v_perm_b32: the same three lookups per byte (host mirror for the CPU check).
__host__ __device__ inline uint32_t gf_mul4x_portable(const uint32_t tab[5], uint32_t x) {
    uint32_t r = 0;
    for (int e = 0; e < 4; ++e) {
        const uint32_t b = (x >> (8 * e)) & 0xffu;
        const uint32_t g0 = b & 7u, g1 = (b >> 3) & 7u, g2 = b >> 6;
        const uint32_t p = ((tab[g0 >> 2] >> (8 * (g0 & 3))) ^ (tab[2 + (g1 >> 2)] >> (8 * (g1 & 3))) ^
                            (tab[4] >> (8 * g2))) & 0xffu;
        r |= p << (8 * e);
    }
    return r;
}

}  // namespace fec
