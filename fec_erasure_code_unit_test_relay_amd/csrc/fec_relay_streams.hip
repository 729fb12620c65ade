// fec_relay_streams.hip -- the symbol-wise decode-and-forward relay (RELAYING_TYPE 2) and its
// destination for many independent relay streams of one (max_payload, T1, N1, T2, N2), one packet or
// a burst of each named stream per call, in one launch.
//
// Reference: one Decoder_Symbol_Wise per stream and side (src/Decoder_Symbol_Wise.cpp), fed one
// packet per call by Variable_Rate_FEC_Decoder (relay :950-1601, destination :1603-1879):
// push_current_codeword / rotate_pointers_and_insert_zero_word (:119-176), then
// symbol_wise_encode_1 (:547-619) at the relay or symbol_wise_decode_1 + extract_data (:621-665) at
// the destination.  The arithmetic, the frame layout and the undefined behaviour defined away are
// those of fec_swdf.hip (its head comment), whose batched calls run a fresh chain over seqs 0..P-1;
// here a group keeps every stream's chain between calls.
//
// What a seq needs.  With the decode done in place on the received rows (the data symbol (j, m) of
// row r belongs to the diagonal of packet r+n-1-m alone), the relay's frame symbol (j, p) of seq t
// reads the decoded hop-1 row t-p-n1+k; the symbols it reads there are decoded by the packets
// t-n2+1 .. t, whose windows reach back to row t-n1-n2+2.  The destination's row for seq t reads
// the decoded frames t-n2+1 .. t.
//
// State in HBM, per stream (zero at create: the slots before a stream's first packet are zero and
// not erased):
//   * relay side: a ring of the last H1 = n1+n2-2 hop-1 codewords (rows of S*n1 bytes, zero for an
//     erased packet), slot seq % H1.  The forwarded rows Y are recomputed from it, not kept: a ring
//     of Y would have to be written with the burst's last n2-1 forwarded rows, which another
//     workgroup (the burst's last chunk) computes, while the codewords of any chunk are in the
//     call's own rows; and in the window without erasure Y is a permutation of the codewords, so
//     recomputing it costs no arithmetic;
//   * destination side: a ring of the symbol parts (S*n2 bytes from frame byte 4) of the last
//     H2 = n2-1 frames, slot seq % H2.
// State on the host, per stream and side: the seq counter and the flags of the last 64 seqs as a
// shift register (bit 63 = the newest); the window mask of a row is its top n bits.
//
// A call's bursts are cut into chunks of at most TP packets, one workgroup each.  A chunk stages the
// H rows in front of it and its own rows in LDS.  A burst's first chunk takes the rows in front from
// the stream's ring; every later chunk lies at least H rows into the burst (TP >= H whenever a burst
// has more than one chunk) and takes them from the call's own rows.  The first chunk's workgroup
// alone writes the ring, after the barrier behind its staging, with the burst's last min(total, H)
// rows (from the call's rows, zero for an erased one).  So no workgroup reads a ring row that
// another workgroup of the launch writes, and a burst longer than the ring writes no slot twice
// (min(total, H) consecutive seqs, H slots).
//
// A mixed group (fec_relay_streams_create_mixed) gives every stream its own (T1, N1, T2, N2).  Each
// side has one chunk body (rs_chunk) and two kernels that differ only in where the chunk's geometry
// comes from: a one-code group's kernel has it in its arguments, a mixed group's takes it from a
// per-code table in device memory, indexed by the unit's code.  What ties a chunk to a code is only
// that geometry and the pointers rules, gf and tab: every decision is the window-n rule of a row's
// mask.  A group's rows and slots have one stride for all its codes: input rows of the largest
// S*n1 (frames: the largest F), output rows of the largest F (S*k), of which a stream uses the
// first bytes of its own code (the rest is written zero, and never read), and a ring slot of the
// largest H*RB per stream, in which a stream uses its own H and RB.  A code's chunks hold
// min(the call's longest burst, the code's tpmax) packets, as a one-code group's.
// A stream that changes code (fec_relay_streams_set_code) starts again at seq 0 in the same slot with
// nothing cleared: a chunk reads a ring row only for a seq >= 0 of the stream's current life (the
// `u.seq0 + p >= 0` test), and every such row was written in this life.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "fec_amd.h"
#include "fec_device.h"
#include "fec_group.h"
#include "fec_host.h"
#include "fec_kernels.h"
#include "fec_status.h"

namespace fec {
namespace {

constexpr int kRsThreads = 256;
constexpr int kRsTP = 32;             // packets per chunk, LDS permitting
constexpr int kRsMaxD = 64;           // decoded packets of a chunk: n2-1 + TP <= 16 + 32; rows: H + TP <= 64
constexpr int kRsMaxCodes = 64;       // tuples of a mixed group
constexpr int kRsRuleU16 = 16 + 16 * 17;  // a wave's rule: sel[k], log col[k][n]
// fixed part of the LDS: exp (1040), log16 (512), masks, row states, the four waves' rules
constexpr int kRsOffMask = 1552, kRsOffRow = kRsOffMask + 4 * kRsMaxD, kRsOffRule = kRsOffRow + kRsMaxD;
constexpr int kRsOffTab = kRsOffRule + 4 * 2 * kRsRuleU16;
static_assert(kRsOffTab % 16 == 0, "LDS carve-up");

struct RsUnit {      // one chunk = one workgroup
    int64_t row0;    // its first row in the call's row arrays
    int64_t seq0;    // that row's sequence number in its stream
    int32_t id;
    int32_t cnt;     // rows of the chunk (<= TP)
    int32_t lead;    // rows of the burst in front of the chunk (0: the first chunk)
    int32_t total;   // rows of the burst
    uint32_t hist;   // first chunk: flags of the H seqs in front of the burst (bit i = seq0 - H + i)
    int32_t code;    // index in the mixed kernels' table (0 in a one-code group)
};

// One side of one code: everything a chunk needs but the call's rows and its own size.  A one-code
// group's kernels take it in their arguments, a mixed group's from a table in device memory.
struct RsGeom {
    const uint8_t* rules;   // window-n rule table (raw coefficients)
    const uint8_t* gf;      // exp[512], log[256]
    const uint32_t* tab;    // relay: gf_mul4x tables of G2[k-1-m][p], [(p-k)*k + m][5]
    int k, n, n2, S, S4, blocks, ES;
    int H;                  // rows staged in front of a chunk
    int D0;                 // packets decoded in front of a chunk (relay: n2-1, destination: 0)
    int RB, RS;             // row bytes S*n; LDS row stride
    int in_off;             // symbol (row, j, m) at in_off + j*n + m of an input row
    int out_row;            // relay: the frame, F bytes; destination: S*k
    int off_raw;            // LDS carve-up after the tables
    int tpmax;              // packets per chunk of a burst cut into several chunks (0: not even the smallest fits)
    int pad;
};

struct RsRows {             // a call's row arrays (R rows) and the group's state
    const uint8_t* in;      // rows of in_stride bytes (rows of erased packets are not read)
    int64_t in_stride;
    const RsUnit* units;
    const uint32_t* masks;  // R window masks (bit m = flag of seq t-n+1+m)
    uint8_t* ring;          // a slot per stream: [H][RB] of its code
    uint8_t* out;           // rows of the group's output stride
    uint8_t* flag;          // R bytes (may be null)
};

struct RsArgs {             // one-code group: the geometry in the arguments
    RsRows r;
    RsGeom g;
    int off_ct;             // the carve-up at this call's chunk size
};
struct RsMixedArgs {        // mixed group: the geometry from codes[unit.code]
    RsRows r;
    const RsGeom* codes;
    int64_t slot;           // bytes of a stream's ring slot
    int out_stride;         // the group's output row stride
    int cap;                // the call's longest burst: a code's chunks hold min(cap, tpmax) packets
};

// LDS offset of CT for chunks of at most tp packets: behind the rows, with slack behind the last one
// for the CT build's reads past a row's last block; or behind the chunk's output rows at any byte phase.
__host__ __device__ inline int64_t rs_off_ct(const RsGeom& g, int tp) {
    const int64_t rows = static_cast<int64_t>(g.H) + tp;
    const int64_t a = rows * g.RS + 4 * g.n + 16, b = static_cast<int64_t>(tp) * g.out_row + 4;
    return (g.off_raw + (a > b ? a : b) + 15) & ~int64_t(15);
}

// One workgroup's chunk u.  ringb: the stream's ring slot; OS: the output row stride (a one-code
// kernel passes g.out_row itself, and the zero fill at the end folds away).
// LDS: GF tables; the masks of the decoded packets; per staged row its state; the rows as in memory
// (later the chunk's output rows); CT[row][m][g] = the data symbols m < k of the row as words of four
// blocks 4g..4g+3 (zero for an erased row, a row before seq 0 and the blocks past `blocks`).  Local
// row l is seq seq0 - H + l; decoded packet d is seq seq0 - D0 + d and its diagonal's position c sits
// in local row d + c (H - D0 = n - 1 on both sides).
template <bool RELAY>
__device__ __forceinline__ void rs_chunk(const RsGeom& g, int off_ct, const RsUnit& u, const RsRows& a, uint8_t* ringb,
                                         int OS) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // exp[0..509] then zeros to 1039; log16[x] = log x, 512 for x = 0: exp[log16 a + log16 b] = a*b
    uint8_t* gexp = smem;
    uint16_t* glog16 = reinterpret_cast<uint16_t*>(smem + 1040);
    uint32_t* pm = reinterpret_cast<uint32_t*>(smem + kRsOffMask);
    uint8_t* rst = smem + kRsOffRow;  // 0: a zero row (erased / before seq 0); else 1 + the staged row's byte phase
    uint32_t* tb = reinterpret_cast<uint32_t*>(smem + kRsOffTab);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint16_t* rl = reinterpret_cast<uint16_t*>(smem + kRsOffRule) + wave * kRsRuleU16;
    const int k = g.k, n = g.n, S = g.S, S4 = g.S4, G = S4 >> 2, H = g.H, D0 = g.D0, RB = g.RB, RS = g.RS;
    const int rows = H + u.cnt, nd = D0 + u.cnt, ctrow = k * S4, blocks = g.blocks;
    const int off_raw = g.off_raw, in_off = g.in_off;
    const bool first = u.lead == 0;  // the rows in front come from the ring
    // the tables are device memory: said here, because a pointer read from the mixed kernels' table is
    // generic to the compiler, which then loads through it with flat instructions
    const auto* grules = (const __attribute__((address_space(1))) uint8_t*)g.rules;
    const auto* ggf = (const __attribute__((address_space(1))) uint8_t*)g.gf;
    for (int i = tid; i < 1040; i += kRsThreads) gexp[i] = i < 510 ? ggf[i] : 0;
    for (int i = tid; i < 256; i += kRsThreads) glog16[i] = i ? ggf[512 + i] : 512;
    if constexpr (RELAY) {
        const auto* gtab = (const __attribute__((address_space(1))) uint32_t*)g.tab;
        for (int i = tid; i < (g.n2 - k) * k * 5; i += kRsThreads) tb[i] = gtab[i];
    }
    auto row_src = [&](int l) -> const uint8_t* {  // local row l < H of a first chunk: the ring's
        const int p = l - H;
        return (p >= 0 || !first) ? a.in + (u.row0 + p) * a.in_stride + in_off
                                  : ringb + ((u.seq0 + p) % H) * RB;
    };
    for (int l = tid; l < rows; l += kRsThreads) {
        const int p = l - H;
        bool live;
        if (p >= 0 || !first)
            live = !((a.masks[u.row0 + p] >> (n - 1)) & 1u);  // a row's own flag is its mask's top bit
        else
            live = u.seq0 + p >= 0;  // of the stream's current life (an erased packet's ring row is zero)
        rst[l] = live ? 1 + static_cast<int>(reinterpret_cast<uintptr_t>(row_src(l)) & 3) : 0;
    }
    const uint32_t nbits = n >= 32 ? ~0u : (1u << n) - 1u;
    for (int d = tid; d < nd; d += kRsThreads) {
        const int p = d - D0;
        const uint32_t m = (p >= 0 || !first) ? a.masks[u.row0 + p] : (static_cast<uint32_t>(u.hist >> d) & nbits);
        pm[d] = m;
        if (p >= 0 && a.flag) a.flag[u.row0 + p] = __popc(m) >= n - k + 1 ? 1 : 0;
    }
    __syncthreads();
    // 1. the rows into LDS, a wave per row (rows of erased packets are never read)
    for (int l = wave; l < rows; l += kRsThreads / 64)
        if (rst[l]) burst_stage(smem, off_raw + l * RS, row_src(l), RB, lane, 64);
    __syncthreads();
    // 2. CT, a wave per row
    for (int l = wave; l < rows; l += kRsThreads / 64) {
        const int st = rst[l];
        const uint32_t rowp = off_raw + l * RS + (st - 1);
        for (int it = lane; it < k * G; it += 64) {
            const int m = it / G, gq = it - m * G;
            uint32_t w = 0;
            if (st) {
                const uint32_t src = rowp + m + 4 * gq * n;  // (blocks past S: bytes of the slack, masked off)
                w = (uint32_t(smem[src]) | uint32_t(smem[src + n]) << 8 | uint32_t(smem[src + 2 * n]) << 16 |
                     uint32_t(smem[src + 3 * n]) << 24) & keep_bytes(blocks - 4 * gq);
            }
            *reinterpret_cast<uint32_t*>(smem + off_ct + l * ctrow + m * S4 + 4 * gq) = w;
        }
    }
    __syncthreads();
    // 3. decodeBlock(T = n-1, t = 0) of every packet whose window holds 0 < erasures < n-k+1, through
    // the window-n rule of its mask, in place: a wave per packet, a lane per word of four blocks.  A
    // recovered symbol m lands in CT[d + m][m], which no other packet and no later symbol reads
    // (position m is erased).
    for (int d = wave; d < nd; d += kRsThreads / 64) {
        const uint32_t mask = pm[d];
        const int cnt = __popc(mask);
        if (cnt == 0 || cnt >= n - k + 1) continue;
        const auto* e = grules + static_cast<int64_t>(mask) * g.ES;
        for (int i = lane; i < k + k * n; i += 64) rl[i] = i < k ? e[i] : glog16[e[i]];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int m = 0; m < k; ++m) {
            if (!((mask >> m) & 1u) || rl[m] == 0xFF) continue;
            for (int gq = lane; gq < G; gq += 64) {
                uint32_t acc = 0;
                for (int c = 0; c < n; ++c) {
                    const int st = rst[d + c];
                    if (((mask >> c) & 1u) || !st) continue;  // an erased symbol is zero
                    uint32_t x;
                    if (c < k) {
                        x = *reinterpret_cast<const uint32_t*>(smem + off_ct + (d + c) * ctrow + c * S4 + 4 * gq);
                    } else {
                        const uint32_t src = off_raw + (d + c) * RS + (st - 1) + c + 4 * gq * n;
                        x = (uint32_t(smem[src]) | uint32_t(smem[src + n]) << 8 | uint32_t(smem[src + 2 * n]) << 16 |
                             uint32_t(smem[src + 3 * n]) << 24) & keep_bytes(blocks - 4 * gq);
                    }
                    const int lc = rl[k + m * n + c];
                    acc ^= uint32_t(gexp[lc + glog16[x & 255]]) | uint32_t(gexp[lc + glog16[(x >> 8) & 255]]) << 8 |
                           uint32_t(gexp[lc + glog16[(x >> 16) & 255]]) << 16 | uint32_t(gexp[lc + glog16[x >> 24]]) << 24;
                }
                *reinterpret_cast<uint32_t*>(smem + off_ct + (d + m) * ctrow + m * S4 + 4 * gq) = acc;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the rule slot is reused by the wave's next packet
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    __syncthreads();
    // 4. the chunk's output rows into LDS, packed at the code's own row size, over the staged rows
    // (all reads of them are done), from the byte phase of the chunk's first row in memory: with
    // OS == orow every row then sits at the phase of its own place; with a wider stride most rows do
    // not, and burst_flush gathers their dwords from bytes (a dword-aligned LDS stride per row, each row
    // at its own phase, was tried: correct, and measured no faster).  Words of four blocks, scattered to
    // the blocks' bytes
    const int orow = g.out_row;
    uint8_t* gout = a.out + u.row0 * OS;
    const int ao = off_raw + static_cast<int>(reinterpret_cast<uintptr_t>(gout) & 3);
    if constexpr (RELAY) {
        // frame = [size BE16][0, 0][S blocks of n2][n2-2 zeros]; symbol (j, p) = XOR_m G2[k-1-m][p] *
        // CT[row t-p-n1+k][m][j]: a copy of m = k-1-p for p < k (G2 = [I | P])
        const int n2 = g.n2, size = (S + 1) * n2;
        for (int t = tid; t < u.cnt; t += kRsThreads) {
            uint8_t* f = smem + ao + t * orow;
            f[0] = uint8_t(size >> 8);
            f[1] = uint8_t(size);
            f[2] = 0;
            f[3] = 0;
            for (int b = 4 + S * n2; b < orow; ++b) f[b] = 0;
        }
        for (int p = 0; p < n2; ++p) {
            for (int it = tid; it < u.cnt * G; it += kRsThreads) {
                const int t = it / G, gq = it - t * G;
                const uint32_t src = off_ct + (t + n2 - 2 - p + k) * ctrow + 4 * gq;  // local row of seq t-p-n1+k
                uint32_t w = 0;
                if (p < k) {
                    w = *reinterpret_cast<const uint32_t*>(smem + src + (k - 1 - p) * S4);
                } else {
                    for (int m = 0; m < k; ++m)
                        w ^= gf_mul4x(tb + ((p - k) * k + m) * 5, *reinterpret_cast<const uint32_t*>(smem + src + m * S4));
                }
                uint8_t* o = smem + ao + t * orow + 4 + p + 4 * gq * n2;
                const int ne = min(4, S - 4 * gq);
                o[0] = uint8_t(w);
                if (ne > 1) o[n2] = uint8_t(w >> 8);
                if (ne > 2) o[2 * n2] = uint8_t(w >> 16);
                if (ne > 3) o[3 * n2] = uint8_t(w >> 24);
            }
        }
    } else {
        // out[t][j*k + i] = d_t[k-1-i][j] = CT[row t-n2+k-i][k-1-i][j]
        for (int i = 0; i < k; ++i) {
            for (int it = tid; it < u.cnt * G; it += kRsThreads) {
                const int t = it / G, gq = it - t * G;
                const uint32_t w = *reinterpret_cast<const uint32_t*>(smem + off_ct + (t + k - 1 - i) * ctrow +
                                                                      (k - 1 - i) * S4 + 4 * gq);
                uint8_t* o = smem + ao + t * orow + i + 4 * gq * k;
                const int ne = min(4, S - 4 * gq);
                o[0] = uint8_t(w);
                if (ne > 1) o[k] = uint8_t(w >> 8);
                if (ne > 2) o[2 * k] = uint8_t(w >> 16);
                if (ne > 3) o[3 * k] = uint8_t(w >> 24);
            }
        }
    }
    __syncthreads();
    if (OS == orow) {
        burst_flush(gout, smem, ao, u.cnt * orow, tid, kRsThreads);
    } else {  // a wave per row: the code's row, then zeros up to the group's stride
        for (int t = wave; t < u.cnt; t += kRsThreads / 64) {
            burst_flush(gout + static_cast<int64_t>(t) * OS, smem, ao + t * orow, orow, lane, 64);
            burst_zero(gout + static_cast<int64_t>(t) * OS + orow, OS - orow, lane, 64);
        }
    }
    if (!first) return;
    // 5. the burst's last min(total, H) rows into the ring (the ring's rows were read in step 1),
    // through LDS: the call's rows again (they may lie behind this chunk), zero for an erased one
    __syncthreads();
    const int nr = min(u.total, H), t0 = u.total - nr;
    for (int r = wave; r < nr; r += kRsThreads / 64) {
        const int64_t row = u.row0 + t0 + r;
        const uint8_t* gr = a.in + row * a.in_stride + in_off;
        const bool erased = (a.masks[row] >> (n - 1)) & 1u;
        if (erased) {
            for (int w = lane; 4 * w < RS; w += 64) *reinterpret_cast<uint32_t*>(smem + off_raw + r * RS + 4 * w) = 0;
        } else {
            burst_stage(smem, off_raw + r * RS, gr, RB, lane, 64);
        }
        if (lane == 0) rst[r] = erased ? 0 : static_cast<int>(reinterpret_cast<uintptr_t>(gr) & 3);  // the row's byte phase
    }
    __syncthreads();
    for (int r = wave; r < nr; r += kRsThreads / 64)
        burst_flush(ringb + ((u.seq0 + t0 + r) % H) * RB, smem, off_raw + r * RS + rst[r], RB, lane, 64);
}

// Two kernels per side that differ only in where the chunk's geometry comes from.  A unit names its
// code, the same for the whole workgroup (readfirstlane), so a mixed kernel's table entry arrives by
// scalar loads, once, before the kernel's first store.
template <bool RELAY>
__global__ __launch_bounds__(kRsThreads) void fec_relay_streams_kernel(RsArgs a) {
    const RsUnit u = a.r.units[blockIdx.x];
    rs_chunk<RELAY>(a.g, a.off_ct, u, a.r, a.r.ring + static_cast<int64_t>(u.id) * a.g.H * a.g.RB, a.g.out_row);
}

// waves_per_eu(6): the one-code kernels take 80 VGPRs, six waves per SIMD; left alone the mixed ones
// take 88, five waves, which costs the destination side a tenth where LDS would let six workgroups
// share a CU ((10,3,10,3) in bursts of 16; profiles/relay_streams_mixed/README.txt, the 88vgpr files,
// measured on this source without the attribute).  Held to 80 they spill two registers.
template <bool RELAY>
__global__ __launch_bounds__(kRsThreads) __attribute__((amdgpu_waves_per_eu(6))) void fec_relay_streams_mixed_kernel(
    RsMixedArgs a) {
    const RsUnit u = a.r.units[blockIdx.x];
    const RsGeom c = a.codes[__builtin_amdgcn_readfirstlane(u.code)];
    rs_chunk<RELAY>(c, static_cast<int>(rs_off_ct(c, min(a.cap, c.tpmax))), u, a.r,
                    a.r.ring + static_cast<int64_t>(u.id) * a.slot, a.out_stride);
}

// every chunk's rows and decoded packets have a place in the fixed part: H <= n1+n2-2, chunks <= kRsTP
static_assert(2 * kMaxRuleN - 2 + kRsTP <= kRsMaxD, "LDS carve-up");

// LDS bytes of a launch whose chunks hold at most tp packets.
size_t rs_lds(const RsGeom& s, int tp) {
    return align16(static_cast<size_t>(rs_off_ct(s, tp)) + (static_cast<size_t>(s.H) + tp) * s.k * s.S4);
}

// (T1, N1, T2, N2) as fec_swdf_create takes them, and n <= 17 (the window-n rule tables).
bool rs_tuple_ok(int max_payload, int T1, int N1, int T2, int N2) {
    if (max_payload < 1 || T1 < 0 || N1 < 0 || T2 < 1 || N2 < 0 || T1 - N1 != T2 - N2) return false;
    const int k = T1 - N1 + 1;
    return k >= 1 && k <= kMaxK && T1 + 1 <= kMaxRuleN && T2 + 1 <= kMaxRuleN;
}

// One side's geometry: everything of RsGeom but the pointers and ES.
RsGeom rs_side(bool relay, int max_payload, int T1, int N1, int T2, int N2) {
    RsGeom s{};
    const int n1 = T1 + 1, n2 = T2 + 1;
    s.k = T1 - N1 + 1;
    s.n = relay ? n1 : n2;
    s.n2 = n2;
    s.S = (max_payload + 2 + s.k - 1) / s.k;
    s.S4 = (s.S + 3) & ~3;
    s.blocks = std::min(s.S, max_payload / s.k + 1);
    s.H = relay ? n1 + n2 - 2 : n2 - 1;
    s.D0 = relay ? n2 - 1 : 0;
    s.RB = s.S * s.n;
    s.RS = 4 * ((s.RB + 6) >> 2);
    s.in_off = relay ? 0 : 4;
    s.out_row = relay ? 2 + (s.S + 1) * n2 : s.S * s.k;
    s.off_raw = static_cast<int>(align16(kRsOffTab + (relay ? static_cast<size_t>(s.n2 - s.k) * s.k * 20 : 0)));
    // a burst of more than one chunk takes chunks of at least H packets (the rows in front of a
    // later chunk all lie in the burst); the smallest chunk is one packet of a one-packet call
    for (int tp = kRsTP; tp >= s.H && !s.tpmax; --tp)
        if (rs_lds(s, tp) <= static_cast<size_t>(kCuLds)) s.tpmax = tp;
    return s;
}

// Whether both sides of a tuple can run at this payload size (what create asks before it allocates).
bool rs_tuple_fits(int max_payload, const int32_t* t, RsGeom* relay, RsGeom* dest) {
    if (!rs_tuple_ok(max_payload, t[0], t[1], t[2], t[3])) return false;
    *relay = rs_side(true, max_payload, t[0], t[1], t[2], t[3]);
    *dest = rs_side(false, max_payload, t[0], t[1], t[2], t[3]);
    return relay->tpmax && dest->tpmax;
}

// The flag half for one stream: the rows' window masks from the stream's flag register w (bit 63 =
// the newest flag), which it advances.
void rs_plan_rows(uint64_t* w, int n, const uint8_t* er, int64_t count, uint32_t* mask) {
    for (int64_t t = 0; t < count; ++t) {
        *w = (*w >> 1) | (static_cast<uint64_t>(er[t] != 0) << 63);
        mask[t] = static_cast<uint32_t>(*w >> (64 - n));
    }
}

}  // namespace
}  // namespace fec

struct fec_relay_streams {
    struct Side {
        std::vector<fec::RsGeom> geo;  // per code, as the kernels take it (the mixed kernels' table on the host)
        fec::RsGeom* d_codes = nullptr;  // that table on the device (mixed groups)
        std::vector<int64_t> seq;    // seqs fed so far per stream
        std::vector<uint64_t> hist;  // flags of the last 64 seqs per stream (bit 63 = the newest)
        uint8_t* d_ring = nullptr;
        int64_t slot = 0;            // a stream's ring slot: the largest H*RB of the group's codes
        int in_min = 0;              // the largest in_off + RB: what an input row stride must hold
        int out_stride = 0;          // the largest out_row
    };
    struct Hop {                     // one hop code (T, N, N): shared by every tuple that uses it on either hop
        int T = 0, N = 0;
        fec_codec* codec = nullptr;
        uint32_t* d_tab = nullptr;   // as a hop-2 code: gf_mul4x tables of G's parity columns
    };
    std::vector<Hop> hops;
    Side relay, dest;
    int nstreams = 0;
    bool mixed = false;                      // made by fec_relay_streams_create_mixed: the table-driven kernels
    std::vector<int32_t> code_of;            // per stream
    std::vector<uint64_t> next_hist;         // a call's new flag registers, committed after the launch
    fec::GroupStage stage;                   // per-call records: chunks + masks
    ~fec_relay_streams() {
        for (void* p : {static_cast<void*>(relay.d_ring), static_cast<void*>(dest.d_ring),
                        static_cast<void*>(relay.d_codes), static_cast<void*>(dest.d_codes)})
            if (p) (void)hipFree(p);
        for (Hop& hp : hops) {
            if (hp.d_tab) (void)hipFree(hp.d_tab);
            if (hp.codec) fec_codec_destroy(hp.codec);
        }
    }
};

namespace {

// One side's call.  in: R rows of in_stride bytes; out: R rows of the side's out_stride.  A stream's
// geometry and chunk size are its code's (one code: a constant).
template <bool RELAY>
int rs_call(fec_relay_streams* h, fec_relay_streams::Side& sd, const int32_t* ids, const int32_t* counts, int M,
            const uint8_t* erasure, const uint8_t* in, int64_t in_stride, uint8_t* out, uint8_t* flag, hipStream_t s) {
    if (M < 0 || M > h->nstreams) return FEC_ERR_ARG;
    if (M == 0) return FEC_OK;
    if (!ids || !erasure || !in || !out || in_stride < sd.in_min) return FEC_ERR_ARG;
    fec::GroupStage& stage = h->stage;
    int64_t R = 0;
    int maxc = 0;
    if (int st = fec::check_counts(counts, M, &R, &maxc)) return st;
    if (int st = stage.check_ids(ids, M)) return st;
    // A code's bursts are one chunk each when the call's longest burst fits its chunk; else chunks of
    // tpmax >= H.  The launch takes the LDS of the largest chunk among the codes present in the call.
    int tp_of[fec::kRsMaxCodes];
    const int ncodes = static_cast<int>(sd.geo.size());
    std::fill(tp_of, tp_of + ncodes, 0);
    int lds = 0;
    int64_t nu = 0;
    for (int m = 0; m < M; ++m) {
        const int c = h->code_of[ids[m]];
        if (!tp_of[c]) {
            tp_of[c] = std::min(maxc, sd.geo[c].tpmax);
            lds = std::max(lds, static_cast<int>(fec::rs_lds(sd.geo[c], tp_of[c])));
        }
        nu += ((counts ? counts[m] : 1) + tp_of[c] - 1) / tp_of[c];
    }
    if (nu > INT32_MAX) return FEC_ERR_ARG;
    const void* kern = h->mixed ? reinterpret_cast<const void*>(fec::fec_relay_streams_mixed_kernel<RELAY>)
                                : reinterpret_cast<const void*>(fec::fec_relay_streams_kernel<RELAY>);
    static int lds_raised[2] = {0, 0};  // per kernel (of this template instance), not per group
    if (int st = fec::lds_allow(kern, lds, &lds_raised[h->mixed])) return st;
    if (int st = stage.begin(s)) return st;
    fec::StageGuard guard{stage};
    const size_t off_masks = fec::align16(static_cast<size_t>(nu) * sizeof(fec::RsUnit));
    if (int st = stage.reserve(off_masks + static_cast<size_t>(R) * 4)) return st;
    fec::RsUnit* un = reinterpret_cast<fec::RsUnit*>(stage.host());
    uint32_t* masks = reinterpret_cast<uint32_t*>(stage.host() + off_masks);
    int64_t row = 0;
    for (int m = 0; m < M; ++m) {
        const int id = ids[m], cnt = counts ? counts[m] : 1, c = h->code_of[id], tp = tp_of[c];
        const fec::RsGeom& g = sd.geo[c];
        uint64_t w = sd.hist[id];
        const uint32_t front = static_cast<uint32_t>(w >> (64 - g.H));  // bit i = flag of seq - H + i
        fec::rs_plan_rows(&w, g.n, erasure + row, cnt, masks + row);
        h->next_hist[m] = w;
        for (int lead = 0; lead < cnt; lead += tp, ++un) {
            un->row0 = row + lead;
            un->seq0 = sd.seq[id] + lead;
            un->id = id;
            un->cnt = std::min(tp, cnt - lead);
            un->lead = lead;
            un->total = cnt;
            un->hist = front;
            un->code = c;
        }
        row += cnt;
    }
    const uint8_t* rec = stage.device();
    fec::RsRows r{};
    r.in = in;
    r.in_stride = in_stride;
    r.units = reinterpret_cast<const fec::RsUnit*>(rec);
    r.masks = reinterpret_cast<const uint32_t*>(rec + off_masks);
    r.ring = sd.d_ring;
    r.out = out;
    r.flag = flag;
    const dim3 grid(static_cast<unsigned>(nu)), block(fec::kRsThreads);
    if (h->mixed) {
        const fec::RsMixedArgs a{r, sd.d_codes, sd.slot, sd.out_stride, maxc};
        hipLaunchKernelGGL(fec::fec_relay_streams_mixed_kernel<RELAY>, grid, block, static_cast<size_t>(lds), s, a);
    } else {
        const fec::RsArgs a{r, sd.geo[0], static_cast<int>(fec::rs_off_ct(sd.geo[0], tp_of[0]))};
        hipLaunchKernelGGL(fec::fec_relay_streams_kernel<RELAY>, grid, block, static_cast<size_t>(lds), s, a);
    }
    if (int st = stage.commit(s)) return st;
    for (int m = 0; m < M; ++m) {
        sd.seq[ids[m]] += counts ? counts[m] : 1;
        sd.hist[ids[m]] = h->next_hist[m];
    }
    return FEC_OK;
}

// The group's hop code (T, N, N), made on first use: the codec of fec_swdf_create, Decoder(n-1, n-k,
// n-k); as a hop-2 code also the gf_mul4x tables (fec_device.h) of G[k-1-m][p], p >= k:
// c*{0..7}, c*({0..7}<<3), c*({0..3}<<6).  *idx: its place in h->hops.
int rs_hop(fec_relay_streams* h, int max_payload, int T, int N, bool hop2, int* idx) {
    int i = 0;
    while (i < static_cast<int>(h->hops.size()) && (h->hops[i].T != T || h->hops[i].N != N)) ++i;
    if (i == static_cast<int>(h->hops.size())) {
        h->hops.emplace_back();
        h->hops[i].T = T, h->hops[i].N = N;
        if (int st = fec_codec_create(max_payload, T, N, N, &h->hops[i].codec)) return st;
    }
    *idx = i;
    if (!hop2 || h->hops[i].d_tab) return FEC_OK;
    const int n2 = T + 1, k = T - N + 1;
    const std::vector<uint8_t> G2 = fec::make_generator(T, N, N);
    const fec::Field& f = fec::field();
    std::vector<uint32_t> tab(static_cast<size_t>(std::max(1, (n2 - k) * k)) * 5, 0);
    for (int p = k; p < n2; ++p)
        for (int m = 0; m < k; ++m) {
            const uint8_t c = G2[(k - 1 - m) * n2 + p];
            uint32_t* t = &tab[(static_cast<size_t>(p - k) * k + m) * 5];
            for (int x = 0; x < 8; ++x) {
                t[x >> 2] |= uint32_t(f.mt[c][x]) << (8 * (x & 3));
                t[2 + (x >> 2)] |= uint32_t(f.mt[c][x << 3]) << (8 * (x & 3));
            }
            for (int x = 0; x < 4; ++x) t[4] |= uint32_t(f.mt[c][x << 6]) << (8 * x);
        }
    FEC_HIP(hipMalloc(&h->hops[i].d_tab, tab.size() * 4));
    FEC_HIP(hipMemcpy(h->hops[i].d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    return FEC_OK;
}

// One side's state: a ring slot per stream that holds any of the group's codes, zero at create.
int rs_create_side(fec_relay_streams::Side& sd, int nstreams, bool mixed) {
    for (const fec::RsGeom& g : sd.geo) {
        sd.slot = std::max(sd.slot, static_cast<int64_t>(g.H) * g.RB);
        sd.in_min = std::max(sd.in_min, g.in_off + g.RB);
        sd.out_stride = std::max(sd.out_stride, g.out_row);
    }
    sd.seq.assign(nstreams, 0);
    sd.hist.assign(nstreams, 0);
    const size_t rb = static_cast<size_t>(nstreams) * sd.slot;
    FEC_HIP(hipMalloc(&sd.d_ring, rb));
    FEC_HIP(hipMemset(sd.d_ring, 0, rb));
    if (mixed) {
        FEC_HIP(hipMalloc(reinterpret_cast<void**>(&sd.d_codes), sd.geo.size() * sizeof(fec::RsGeom)));
        FEC_HIP(hipMemcpy(sd.d_codes, sd.geo.data(), sd.geo.size() * sizeof(fec::RsGeom), hipMemcpyHostToDevice));
    }
    return FEC_OK;
}

// A group of ncodes tuples {T1, N1, T2, N2}; code_of null: every stream on code 0.  Everything that
// can refuse the arguments comes before the first allocation.
int rs_create(int max_payload, const int32_t* tuples, int ncodes, const int32_t* code_of, int nstreams, bool mixed,
              fec_relay_streams** out) {
    try {
        std::vector<fec::RsGeom> rg(ncodes), dg(ncodes);
        for (int c = 0; c < ncodes; ++c)
            if (!fec::rs_tuple_fits(max_payload, tuples + 4 * c, &rg[c], &dg[c])) return FEC_ERR_ARG;
        std::unique_ptr<fec_relay_streams> h(new fec_relay_streams());
        h->nstreams = nstreams;
        h->mixed = mixed;
        if (code_of)
            h->code_of.assign(code_of, code_of + nstreams);
        else
            h->code_of.assign(nstreams, 0);
        for (int c = 0; c < ncodes; ++c) {
            const int32_t* t = tuples + 4 * c;
            int i1 = 0, i2 = 0;
            if (int st = rs_hop(h.get(), max_payload, t[0], t[1], false, &i1)) return st;
            if (int st = rs_hop(h.get(), max_payload, t[2], t[3], true, &i2)) return st;
            fec::CodecView v1, v2;
            if (int st = fec::codec_view(h->hops[i1].codec, &v1)) return st;
            if (int st = fec::codec_view(h->hops[i2].codec, &v2)) return st;
            if (v1.wbase_n < 0 || v1.S != rg[c].S || v1.n != rg[c].n) return FEC_ERR_ARG;
            if (v2.wbase_n < 0 || v2.S != dg[c].S || v2.n != dg[c].n) return FEC_ERR_ARG;
            rg[c].rules = v1.rules + v1.wbase_n, rg[c].gf = v1.gf, rg[c].ES = v1.ES, rg[c].tab = h->hops[i2].d_tab;
            dg[c].rules = v2.rules + v2.wbase_n, dg[c].gf = v2.gf, dg[c].ES = v2.ES;
        }
        h->relay.geo = std::move(rg);
        h->dest.geo = std::move(dg);
        if (int st = rs_create_side(h->relay, nstreams, mixed)) return st;
        if (int st = rs_create_side(h->dest, nstreams, mixed)) return st;
        h->next_hist.assign(nstreams, 0);
        const size_t stage = static_cast<size_t>(nstreams) * (sizeof(fec::RsUnit) + 4) + 64;
        if (int st = h->stage.init(nstreams, stage)) return st;
        *out = h.release();
        return FEC_OK;
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

}  // namespace

extern "C" {

int fec_relay_streams_fit(int relay, int max_payload, int T1, int N1, int T2, int N2, int* chunk_packets,
                          int* lds_bytes) {
    if (!fec::rs_tuple_ok(max_payload, T1, N1, T2, N2)) return FEC_ERR_ARG;
    const fec::RsGeom s = fec::rs_side(relay != 0, max_payload, T1, N1, T2, N2);
    if (chunk_packets) *chunk_packets = s.tpmax;
    if (lds_bytes) *lds_bytes = s.tpmax ? static_cast<int>(fec::rs_lds(s, s.tpmax)) : 0;
    return s.tpmax ? 1 : 0;
}

int fec_relay_streams_mixed_fit(int max_payload, const int32_t* tuples, int ncodes, int32_t* relay_chunk,
                                int32_t* relay_lds, int32_t* dest_chunk, int32_t* dest_lds) {
    if (!tuples || ncodes < 1 || ncodes > fec::kRsMaxCodes || !relay_chunk || !relay_lds || !dest_chunk || !dest_lds)
        return FEC_ERR_ARG;
    for (int c = 0; c < ncodes; ++c) {
        fec::RsGeom r, d;
        if (!fec::rs_tuple_fits(max_payload, tuples + 4 * c, &r, &d)) return FEC_ERR_ARG;
        relay_chunk[c] = r.tpmax, relay_lds[c] = static_cast<int32_t>(fec::rs_lds(r, r.tpmax));
        dest_chunk[c] = d.tpmax, dest_lds[c] = static_cast<int32_t>(fec::rs_lds(d, d.tpmax));
    }
    return FEC_OK;
}

int fec_relay_streams_plan_host(int k, int n, const uint8_t* erasure, const int32_t* counts, int ncounts,
                                uint32_t* mask, uint8_t* flag) {
    if (k < 1 || n < k || n > fec::kMaxN || !erasure || !counts || ncounts < 0 || !mask || !flag) return FEC_ERR_ARG;
    for (int c = 0; c < ncounts; ++c)
        if (counts[c] < 1) return FEC_ERR_ARG;
    uint64_t w = 0;
    int64_t seq = 0;
    for (int c = 0; c < ncounts; ++c) {
        fec::rs_plan_rows(&w, n, erasure + seq, counts[c], mask + seq);
        for (int64_t t = seq; t < seq + counts[c]; ++t) flag[t] = __builtin_popcount(mask[t]) >= n - k + 1 ? 1 : 0;
        seq += counts[c];
    }
    return FEC_OK;
}

int fec_relay_streams_create(int max_payload, int T1, int N1, int T2, int N2, int nstreams, fec_relay_streams** out) {
    if (!out) return FEC_ERR_ARG;
    *out = nullptr;
    if (nstreams <= 0) return FEC_ERR_ARG;
    const int32_t tuple[4] = {T1, N1, T2, N2};
    return rs_create(max_payload, tuple, 1, nullptr, nstreams, false, out);
}

int fec_relay_streams_create_mixed(int max_payload, const int32_t* tuples, int ncodes, const int32_t* code_of,
                                   int nstreams, fec_relay_streams** out) {
    if (!out) return FEC_ERR_ARG;
    *out = nullptr;
    if (!tuples || !code_of || ncodes < 1 || ncodes > fec::kRsMaxCodes || nstreams <= 0) return FEC_ERR_ARG;
    for (int i = 0; i < nstreams; ++i)
        if (code_of[i] < 0 || code_of[i] >= ncodes) return FEC_ERR_ARG;
    return rs_create(max_payload, tuples, ncodes, code_of, nstreams, true, out);
}

int fec_relay_streams_destroy(fec_relay_streams* h) {
    delete h;
    return FEC_OK;
}

int fec_relay_streams_codes(const fec_relay_streams* h, int* ncodes, int* cw_bytes, int* frame_stride, int* out_stride) {
    if (!h) return FEC_ERR_ARG;
    if (ncodes) *ncodes = static_cast<int>(h->relay.geo.size());
    if (cw_bytes) *cw_bytes = h->relay.in_min;
    if (frame_stride) *frame_stride = h->relay.out_stride;
    if (out_stride) *out_stride = h->dest.out_stride;
    return FEC_OK;
}

int fec_relay_streams_stream_geometry(const fec_relay_streams* h, int id, int* code, int* k, int* n1, int* n2, int* S,
                                      int* cw_bytes, int* frame_bytes, int* out_bytes, int* delay) {
    if (!h || id < 0 || id >= h->nstreams) return FEC_ERR_ARG;
    const int c = h->code_of[id];
    const fec::RsGeom& r = h->relay.geo[c];
    if (code) *code = c;
    if (k) *k = r.k;
    if (n1) *n1 = r.n;
    if (n2) *n2 = r.n2;
    if (S) *S = r.S;
    if (cw_bytes) *cw_bytes = r.RB;
    if (frame_bytes) *frame_bytes = r.out_row;
    if (out_bytes) *out_bytes = h->dest.geo[c].out_row;
    if (delay) *delay = r.n + r.n2 - r.k - 1;
    return FEC_OK;
}

int fec_relay_streams_geometry(const fec_relay_streams* h, int* k, int* n1, int* n2, int* S, int* cw_bytes,
                               int* frame_bytes, int* delay) {
    if (!h || h->relay.geo.size() != 1) return FEC_ERR_ARG;
    return fec_relay_streams_stream_geometry(h, 0, nullptr, k, n1, n2, S, cw_bytes, frame_bytes, nullptr, delay);
}

int fec_relay_streams_set_code(fec_relay_streams* h, int id, int code) {
    if (!h || id < 0 || id >= h->nstreams || code < 0 || code >= static_cast<int>(h->relay.geo.size()))
        return FEC_ERR_ARG;
    // host work only: a chunk reads a ring row only for a seq >= 0 of the stream's current life, and
    // every such row was written in this life, so the slot's old bytes are never seen; calls already
    // queued carry their own seqs and codes in their staged records
    h->code_of[id] = code;
    for (fec_relay_streams::Side* sd : {&h->relay, &h->dest}) {
        sd->seq[id] = 0;
        sd->hist[id] = 0;
    }
    return FEC_OK;
}

int fec_relay_streams_relay(fec_relay_streams* h, const int32_t* ids, const int32_t* counts, int M,
                            const uint8_t* erasure, const uint8_t* d_cw, int64_t cw_stride, uint8_t* d_frames,
                            uint8_t* d_flag, void* stream) {
    if (!h) return FEC_ERR_ARG;
    try {
        return rs_call<true>(h, h->relay, ids, counts, M, erasure, d_cw, cw_stride, d_frames, d_flag,
                             static_cast<hipStream_t>(stream));
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    }
}

int fec_relay_streams_destination(fec_relay_streams* h, const int32_t* ids, const int32_t* counts, int M,
                                  const uint8_t* erasure, const uint8_t* d_frames, uint8_t* d_out, uint8_t* d_flag,
                                  void* stream) {
    if (!h) return FEC_ERR_ARG;
    try {
        return rs_call<false>(h, h->dest, ids, counts, M, erasure, d_frames, h->relay.out_stride, d_out, d_flag,
                              static_cast<hipStream_t>(stream));
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    }
}

int fec_relay_streams_state(const fec_relay_streams* h, int id, int64_t* relayed, int64_t* delivered) {
    if (!h || id < 0 || id >= h->nstreams) return FEC_ERR_ARG;
    if (relayed) *relayed = h->relay.seq[id];
    if (delivered) *delivered = h->dest.seq[id];
    return FEC_OK;
}

}  // extern "C"
