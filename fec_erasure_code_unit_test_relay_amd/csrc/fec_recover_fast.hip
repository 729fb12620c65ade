// fec_recover_fast.hip -- recovery of erased packets, specialised at compile time on k and n-k.
//
// Byte h = s * k + i of a recovered packet's [len_hi, len_lo, payload] is
// XOR_q coef[i][q] * cw[x-i+q][s*n+q] (fec_kernels.hip, step 4).  One wave per packet, one
// workgroup per wave; nothing is set up before the first packet and nothing is shared between
// waves:
//   * the list entry is loaded together with the count of recovered packets (a wave whose first
//     index is at or past the count returns at once), then the packet's k x n coefficients and the
//     span of codeword rows its diagonals touch are loaded together: two memory round trips;
//   * each coefficient's five gf_mul4x registers are built by one lane with packed doubling
//     (gf_mul4x_tables) and kept in LDS, (tab[0..3]) as one 16-byte entry and (tab[4]) as a dword;
//   * item (i, g) = position i of sub-streams 4g .. 4g+3: per term q the four source bytes, n
//     apart in row x-i+q of the staged span, become one dword and one packed product multiplies
//     all four (3 v_perm_b32 + XORs): no exp / log table and no data-dependent LDS address;
//   * the four result bytes go to the row assembled in LDS; the row leaves in dwords (bytes at
//     its ends when the row's address or L is off dword alignment), zero at and past the length.
// Per term: 4 ds_read_u8 + 1 ds_read_b128 + 1 ds_read_b32, 3 pack + 1 select + 5 mask/shift +
// 3 v_perm + 3 XOR VALU.  (A bit-sliced product -- mask of bit b of every byte, AND with a splat
// of c * 2^b -- takes 8 x (shift-and, multiply by 0xff, AND, XOR) = 32 VALU per term and 8
// registers per constant against 14 and 5 here, so the v_perm form was taken.)
#include "fec_device.h"
#include "fec_kernels.h"
#include "fec_recover_fast.h"

namespace fec {

template <int K, int NP>
__global__ __launch_bounds__(64) void fec_recover_fast_kernel(RecArgs a) {
    constexpr int n = K + NP;
    constexpr int KN = K * n;
    constexpr int kCf = (KN + 63) / 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t fsm[];
    uint4* t4 = reinterpret_cast<uint4*>(fsm);                    // [KN] tab[0..3] of coefficient (i, q)
    uint32_t* t1 = reinterpret_cast<uint32_t*>(fsm + 16 * KN);    // [KN] tab[4]
    uint8_t* rows = fsm + ((20 * KN + 15) & ~15);                 // the staged span (a.stage_bytes)
    uint8_t* obuf = rows + a.stage_bytes;  // [2 unused, len_hi, len_lo, payload]: payload on a dword
    const int lane = threadIdx.x;
    const int L = a.L, S = a.S, CW = a.CW;
    const int NS4 = (S + 3) >> 2;
    const int waves = gridDim.x;
    const int64_t cw_total = a.P * CW;
    phase_stamp(a.stamps, blockIdx.x, 0);
    int r = blockIdx.x;
    // the count and the wave's first list entry in one round trip (entries < Pout exist in memory)
    int nrec = a.counters[2];
    int x = 0, xr = 0;
    if (r < a.Pout) {
        x = a.rec_list[2 * r];
        xr = a.rec_list[2 * r + 1];
    }
    phase_stamp(a.stamps, blockIdx.x, 1);
    while (r < nrec) {
        const int rn = r + waves;  // the next entry travels with this packet's loads
        int xn = 0, xrn = 0;
        if (rn < nrec) {
            xn = a.rec_list[2 * rn];
            xrn = a.rec_list[2 * rn + 1];
        }
        if (x >= a.row_off) {  // else: before the caller's first output row (wave-uniform)
            uint8_t* orow = a.out + static_cast<int64_t>(x - a.row_off) * L;
            const RecFastSpan sp = rec_fast_span(x, K, n, CW, a.P);
            uint4 piece[kRecFastStageChunks];
#pragma unroll
            for (int j = 0; j < kRecFastStageChunks; ++j) {
                const int c = lane + 64 * j;
                const int64_t o = sp.a0 + 16 * c;
                piece[j] = make_uint4(0u, 0u, 0u, 0u);
                if (c < sp.nb && o + 16 <= cw_total) piece[j] = *reinterpret_cast<const uint4*>(a.cw + o);
            }
            // the buffer's last piece, when the buffer ends inside it: byte by byte
            const int ctail = static_cast<int>((cw_total - sp.a0) >> 4);
            const bool tail = ctail < sp.nb;
            uint32_t tbyte = 0;
            if (tail && sp.a0 + 16 * ctail + lane < cw_total && lane < 16) tbyte = a.cw[sp.a0 + 16 * ctail + lane];
            uint32_t cf[kCf];
            const uint8_t* cfp = a.coef + static_cast<int64_t>(xr) * KN;
#pragma unroll
            for (int j = 0; j < kCf; ++j) cf[j] = lane + 64 * j < KN ? cfp[lane + 64 * j] : 0u;
#pragma unroll
            for (int j = 0; j < kRecFastStageChunks; ++j)
                if (lane + 64 * j < sp.nb) *reinterpret_cast<uint4*>(rows + 16 * (lane + 64 * j)) = piece[j];
            if (tail && lane < 16) rows[16 * ctail + lane] = static_cast<uint8_t>(tbyte);
#pragma unroll
            for (int j = 0; j < kCf; ++j) {
                if (lane + 64 * j < KN) {
                    uint32_t tab[5];
                    gf_mul4x_tables(cf[j], tab);
                    t4[lane + 64 * j] = make_uint4(tab[0], tab[1], tab[2], tab[3]);
                    t1[lane + 64 * j] = tab[4];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int it = lane; it < K * NS4; it += 64) {
                const RecFastItem m = rec_fast_item(sp, x, it, K, n, S, CW, a.P);
                // a sub-stream past S re-reads sub-stream 4g (its byte is not written)
                const int o1 = m.ne > 1 ? n : 0, o2 = m.ne > 2 ? 2 * n : 0, o3 = m.ne > 3 ? 3 * n : 0;
                uint32_t acc = 0;
#pragma unroll
                for (int q = 0; q < n; ++q) {
                    const bool use = q >= m.qlo && q < m.qhi;
                    const uint8_t* p = rows + (use ? m.base + q * (CW + 1) : 0);
                    const uint32_t v = static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[o1]) << 8) |
                                       (static_cast<uint32_t>(p[o2]) << 16) | (static_cast<uint32_t>(p[o3]) << 24);
                    const uint4 ta = t4[m.i * n + q];
                    const uint32_t tab[5] = {ta.x, ta.y, ta.z, ta.w, t1[m.i * n + q]};
                    acc ^= gf_mul4x(tab, use ? v : 0u);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int h = (4 * m.g + e) * K + m.i;
                    if (e < m.ne && h < L + 2) obuf[2 + h] = static_cast<uint8_t>(acc >> (8 * e));
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // recovered length (Decoder.cpp:141-149): bytes 0, 1, clamped to L
            const int ln = min(static_cast<int>(obuf[2]) * 256 + static_cast<int>(obuf[3]), L);
            const uint8_t* pl = obuf + 4;  // payload byte b, on a dword
            const int head = min(L, static_cast<int>((4 - (reinterpret_cast<uintptr_t>(orow) & 3)) & 3));
            const int nd = (L - head) >> 2;
            const int tail0 = head + 4 * nd;
            for (int w = lane; w < nd; w += 64) {
                const int b = head + 4 * w;
                const uint32_t lo = *reinterpret_cast<const uint32_t*>(pl + (b & ~3));
                const uint32_t hi = *reinterpret_cast<const uint32_t*>(pl + (b & ~3) + 4);
                *reinterpret_cast<uint32_t*>(orow + b) = __builtin_amdgcn_alignbyte(hi, lo, head) & keep_bytes(ln - b);
            }
            if (lane < head) orow[lane] = lane < ln ? pl[lane] : 0;
            if (lane < L - tail0) orow[tail0 + lane] = tail0 + lane < ln ? pl[tail0 + lane] : 0;
            if (lane == 0) a.out_len[x - a.row_off] = ln;
            __builtin_amdgcn_wave_barrier();  // tables, span and row are rewritten by the next packet
        }
        r = rn;
        x = xn;
        xr = xrn;
    }
    phase_stamp(a.stamps, blockIdx.x, 2);
}

// Every pair of the specialised copy's list; whether a codec's span fits the staging limit (it
// does not for the long codewords of k = 1, 2 at L = 300) is decided per codec on the host.
#define FEC_RECOVER_FAST_INST(K, NP) template __global__ void fec_recover_fast_kernel<K, NP>(RecArgs);
FEC_COPY_FAST_LIST(FEC_RECOVER_FAST_INST)

const void* fec_recover_fast_kernel_for(int k, int np) {
#define FEC_RECOVER_FAST_CASE(K, NP) \
    if (k == K && np == NP) return reinterpret_cast<const void*>(&fec_recover_fast_kernel<K, NP>);
    FEC_COPY_FAST_LIST(FEC_RECOVER_FAST_CASE)
#undef FEC_RECOVER_FAST_CASE
    return nullptr;
}

}  // namespace fec
