// fec_mw_relay_streams.hip -- the message-wise decode-and-forward relay (RELAYING_TYPE 1) at fixed
// rate for many independent flows of one (max_payload, T1,B1,N1, T2,B2,N2), one packet or a burst of
// each named flow per call, hop-1 decode and hop-2 encode in one launch.
//
// Reference: per flow an FEC_Decoder of the hop-1 code feeding an FEC_Encoder of the hop-2 code, one
// packet per call: FEC_Decoder::onReceive (FEC_Decoder.cpp:38-75: its own zero-padded copy of the
// codeword :55-63, Decoder::decodeStream, Decoder.cpp:72-175) outputs message seq - T1, and
// FEC_Encoder::onTransmit (FEC_Encoder.cpp:38-62: the window [len_hi, len_lo, payload, zero pad],
// Encoder.cpp:73-95, the closed form :65-98, the trimmed size FEC_Encoder.cpp:55-60) codes it as its
// packet number seq - T1.  A message the relay loses is forwarded as the empty message, so relay seq
// and source seq stay equal (the driver's constant-transmission case).  This is the fixed-rate relay
// of this library's per-packet contract, not the reference's adaptive session
// (Variable_Rate_FEC_Decoder's stored-message vector, the 12-byte relay header, T2_ack).
// The destination is an ordinary (T2,B2,N2) decoder: fec_streams_decode_burst of a fec_streams group
// serves it, and there is no destination entry here.
//
// The rule is equivalence: per flow the rows of all calls together equal fec_streams_decode_burst over
// the flow's hop-1 sequence, its first T1 rows dropped, then fec_streams_encode_burst over the rest
// with lengths clipped to [0, L].  Both hops' lengths meet in one number: the decoder outputs hdr or
// min(hdr, L) (the clamp rule, kRowClamp) and copies min(that, L) bytes; the encoder clips the length
// to L; so the forwarded window is [min(hdr, L), the message's first min(hdr, L) bytes, zeros]
// whichever way the decoder went, and no payload row has to exist in between.
//
// State in HBM per flow: the decoder's ring of the last kRR received hop-1 codewords (slot seq % kRR)
// and the encoder's ring of the last n2-1 message windows (S2*k2 bytes, slot message % (n2-1)); on the
// host the flow's symbolic decoder (fec::StreamPlanner) and its seq counter.
//
// A burst is cut into chunks of at most TP packets, one workgroup each.  A chunk of cnt rows decodes
// its cnt messages and, unless it is the burst's first, the H2 = n2-1 messages in front of them
// (another workgroup computes those, so they are decoded again from the call's own rows) into the
// hop-2 position planes; then it encodes.  Each run of messages is one pass over its HR1 + count hop-1
// codewords staged in LDS (HR1 = T1+k1-1): first the H2 in front (HR1 + H2 rows), then the chunk's own
// (HR1 + cnt rows) over the same LDS -- HR1 + H2 + cnt rows at once do not fit a CU at 1 500-byte payloads.
// Only a burst's first chunk has packets from before the call in front of it: it reads the codeword
// ring and the window ring, and it alone writes them, after the barrier behind its staging, with the
// burst's last min(total, T1+k1) received codewords and last min(messages, n2-1) windows -- decoded
// again from the call's rows when they lie behind the chunk.  So no workgroup reads a ring row that
// another workgroup of the launch writes; it takes TP >= HR1 + H2 whenever a burst has several chunks.
//
// A mixed group (fec_mw_relay_streams_create_mixed) gives every flow its own pair (T1,B1,N1) -> (T2,B2,N2).
// There is one chunk body (mw_chunk) and two kernels that differ only in where the chunk's geometry comes
// from: a one-code group's kernel has it in its arguments, a mixed group's takes both codes' constants
// from a per-pair table in device memory, indexed by the unit's pair, and works out the chunk-size part
// (mw_carve: the rows of a pass and the LDS carve-up) from the call's longest burst, as the host does for
// the launch's LDS.  A pair's chunks hold min(the call's longest burst, the pair's tpmax) packets, as a
// one-code group's, so a burst longer than its chunk has chunks of tpmax >= HR1 + H2.  A group's rows and
// slots have one stride for all its pairs: input rows of at least the largest CW1, output rows of the
// largest CW2, of which a flow uses the first bytes of its own code (the rest of an output row is
// written zero), a codeword ring slot of kRR rows of the largest CW1 and a window slot of the largest
// W2 * SK2 per flow, in which a flow uses its own sizes.
// A flow that changes pair (fec_mw_relay_streams_set_code) starts again at seq 0 in the same slots with
// nothing cleared: a chunk reads a codeword ring row only for a hop-1 seq >= 0 (the `sq + p >= 0` test)
// and a window row only for a message number >= 0 (`e >= 0`) of the flow's current life, and what it
// reads there was written in this life -- but for the ring row of an erased packet, which keeps its old
// bytes and is never used: an erased packet's coefficients are zero and its message is not a copy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "fec_amd.h"
#include "fec_burst.h"
#include "fec_device.h"
#include "fec_host.h"
#include "fec_kernels.h"
#include "fec_status.h"

namespace fec {
namespace {

constexpr int kMwMaxCodes = 64;  // pairs of a mixed group

struct MwUnit {          // one chunk = one workgroup (48 bytes)
    int64_t row0;        // its first row in the call's row arrays
    int64_t seq0;        // that row's hop-1 sequence number in its flow
    int64_t coef;        // byte offset of the first coefficient block of the rows it decodes (recovered rows, in row order)
    int64_t tail_coef;   // first chunk of a burst cut in several: the same for the burst's last rows
    int32_t id;
    int16_t cnt;         // rows of the chunk (<= TP <= 32)
    int16_t code;        // index in the mixed kernel's table (0 in a one-code group; < kMwMaxCodes)
    int32_t lead;        // rows of the burst in front of the chunk (0: the first chunk)
    int32_t total;       // rows of the burst
};
static_assert(sizeof(MwUnit) == 48, "chunk record");

struct MwGeom {            // both codes' constants (mw_consts) and a chunk's geometry at its size (mw_carve)
    const uint8_t* gf;     // exp[512], log[256]
    const uint32_t* ptab;  // hop 2: [k2][n2-k2][8] gf_mul4x tables
    int L, T1, k1, n1, CW1, CWS1, CWD1, HR1;
    int k2, n2, S2, SP2, NS4, CW2, SK2, W2, H2;
    int TP, PR, ROWS1, ROWS2;  // messages of a pass (max(TP, H2) where bursts are cut); staged codewords HR1 + PR; window rows H2 + TP
    int off_gf, off_rows, off_coef, off_planes, off_meta;  // dynamic LDS carve-up (multiples of 16)
    FastDiv dk1, dk2, dns4, dnq, dcwd;
};

struct MwRows {              // a call's row arrays (R rows) and the group's state
    const uint8_t* cw_in;    // R rows of `stride` bytes (rows of erased packets are not read)
    int64_t stride;
    const uint8_t* flags;    // R bytes: fate | kRowClamp | kRowErased (plan_burst_rows)
    const uint8_t* coefs;    // the recovered rows' k1 x n1 blocks
    uint8_t* cw_out;         // R rows of the group's output stride
    int32_t* cw_len;
    uint8_t* fate;           // R bytes (may be null)
    const MwUnit* units;
    uint8_t* ring1;          // a slot per flow: [kRR][CW1] of its pair
    uint8_t* win2;           // a slot per flow: [W2][SK2] of its pair
};

struct MwArgs {              // one-code group: the geometry in the arguments
    MwRows r;
    MwGeom g;
};
struct MwCode {              // a pair of a mixed group: MwGeom but its chunk-size part (mw_carve), which the kernel fills
    MwGeom g;
    int tpmax;               // packets per chunk of a burst cut in several
    int pad;
};
struct MwMixedArgs {         // mixed group: the geometry from codes[unit.code]
    MwRows r;
    const MwCode* codes;
    int64_t slot1, slot2;    // bytes of a flow's codeword ring slot and of its window slot
    int out_stride;          // the group's output row stride
    int cap;                 // the call's longest burst: a pair's chunks hold min(cap, tpmax) packets
};

// The chunk-size part of the geometry for chunks of tp packets, from the constants already in *a: the
// messages of a pass, the staged rows and the dynamic LDS carve-up.  Returns the LDS bytes.  The host
// calls it for a launch's LDS size and a one-code group's arguments, the mixed kernel for its own chunk.
__host__ __device__ inline int mw_carve(MwGeom* a, int tp) {
    const auto max2 = [](int64_t x, int64_t y) { return x > y ? x : y; };
    const auto al16 = [](int64_t v) { return (v + 15) & ~int64_t(15); };
    const int np2 = a->n2 - a->k2;
    a->TP = tp;
    // a burst is cut only into chunks of at least HR1 + H2 packets; then a pass may hold the H2 messages in
    // front of a chunk, or the burst's last max(H2, 1) for the rings
    a->PR = tp >= a->HR1 + a->H2 ? static_cast<int>(max2(max2(tp, a->H2), 1)) : tp;
    a->ROWS1 = a->HR1 + a->PR;
    a->ROWS2 = a->H2 + tp;
    int64_t off = al16(max2(1, a->k2 * np2) * 32);
    a->off_gf = static_cast<int>(off);
    off += 768;
    a->off_rows = static_cast<int>(off);
    off = al16(off + max2(static_cast<int64_t>(a->ROWS1) * a->CWS1, static_cast<int64_t>(tp) * a->CW2 + 32));
    a->off_coef = static_cast<int>(off);
    off = al16(off + static_cast<int64_t>(a->PR) * a->k1 * a->n1 + 16);
    a->off_planes = static_cast<int>(off);
    off = al16(off + static_cast<int64_t>(a->k2) * a->ROWS2 * a->SP2);
    a->off_meta = static_cast<int>(off);
    off = al16(off + static_cast<int64_t>(a->ROWS1) * 4 + static_cast<int64_t>(a->PR) * 9);
    return static_cast<int>(off < (int64_t(1) << 30) ? off : (int64_t(1) << 30));
}

// One workgroup's chunk u of a flow whose geometry is g.  ring1, win2: the flow's slots; OS: the output
// row stride (the one-code kernel passes g.CW2 itself, and the zero fill at the end folds away).
// LDS: the hop-2 parity tables; the GF tables; a pass's staged hop-1 codewords, each row at its own
// dword phase (later the chunk's hop-2 codewords); its recovered rows' coefficient blocks; the hop-2
// windows as position planes [i][row][sub-stream] (window row r = message seq0 - T1 + r - H2); per
// row offsets, flags and lengths.
__device__ __forceinline__ void mw_chunk(const MwRows& a, const MwGeom& g, const MwUnit& u, uint8_t* ring1,
                                         uint8_t* win2, int OS) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int L = g.L, T1 = g.T1, k1 = g.k1, n1 = g.n1, CW1 = g.CW1, CWS1 = g.CWS1, CWD1 = g.CWD1, HR1 = g.HR1;
    const int k2 = g.k2, n2 = g.n2, S2 = g.S2, SP2 = g.SP2, NS4 = g.NS4, CW2 = g.CW2, SK2 = g.SK2;
    const int W2 = g.W2, H2 = g.H2, PR = g.PR, ROWS2 = g.ROWS2, np2 = n2 - k2, kn1 = k1 * n1;
    uint32_t* tab = reinterpret_cast<uint32_t*>(smem);
    const uint8_t* gexp = smem + g.off_gf;
    const uint8_t* glog = gexp + 512;
    uint8_t* planes = smem + g.off_planes;
    int* rowoff = reinterpret_cast<int*>(smem + g.off_meta);  // [ROWS1] LDS offset of the codeword's byte 0; -1: none
    int* cord = rowoff + g.ROWS1;                             // [PR] coefficient block of a recovered message
    int* lnS = cord + PR;                                     // [PR] forwarded length min(hdr, L)
    uint8_t* fl = reinterpret_cast<uint8_t*>(lnS + PR);       // [PR] row flags
    // the tables are device memory: said here, because a pointer read from the mixed kernel's table is
    // generic to the compiler, which then loads through it with flat instructions
    const auto* ptab = (const __attribute__((address_space(1))) uint32_t*)g.ptab;
    const auto* ggf = (const __attribute__((address_space(1))) uint8_t*)g.gf;
    for (int i = tid; i < k2 * np2 * 8; i += 256) tab[i] = ptab[i];
    for (int i = tid; i < 768; i += 256) smem[g.off_gf + i] = ggf[i];
    const bool first = u.lead == 0;
    const int nq = (SK2 + 3) >> 2;
    const uint8_t* coefs = nullptr;

    // hop-1 window byte h of a pass's output j (message sq + j - T1 = staged row j + k1 - 1); staged row R
    // is packet sq + R - HR1
    auto byte_at = [&](int j, int h) -> uint8_t {
        const int s = fdiv(g.dk1, h), i = h - s * k1;
        if ((fl[j] & 3) == kCopy) {
            const int ro = rowoff[j + k1 - 1];
            return ro < 0 ? 0 : smem[ro + s * n1 + i];
        }
        const uint8_t* coef = coefs + cord[j] * kn1 + i * n1;
        uint8_t acc = 0;
        for (int q = 0; q < n1; ++q) {  // symbol q of packet x - i + q
            const uint8_t c = coef[q];
            const int R = j + k1 - 1 - i + q;
            if (!c || R > j + HR1) continue;
            const int ro = rowoff[R];
            if (ro >= 0) acc ^= gmul(gexp, glog, c, smem[ro + s * n1 + q]);
        }
        return acc;
    };

    // One pass: the messages of outputs j = 0 .. cnt-1 of the rows from call row rb (hop-1 seq sq) on,
    // decoded into window rows prow0 + j of the planes; `front` rows of the burst lie in front of rb,
    // older packets come from the ring.  Ends before the barrier that completes the planes; returns the
    // recovered messages among them (the coefficient blocks it took from coef_off on).
    auto decode_pass = [&](int64_t rb, int64_t sq, int cnt, int front, int64_t coef_off, int prow0) -> int {
        const int R1 = HR1 + cnt;
        auto call_row = [&](int R) { return R - HR1 >= -front; };
        for (int R = tid; R < R1; R += 256) {
            const int p = R - HR1;
            const uint8_t* gr = nullptr;
            if (call_row(R)) {
                if (!(a.flags[rb + p] & kRowErased)) gr = a.cw_in + (rb + p) * a.stride;
            } else if (sq + p >= 0) {
                gr = ring1 + ((sq + p) % kRR) * CW1;
            }
            rowoff[R] = gr ? g.off_rows + R * CWS1 + static_cast<int>(reinterpret_cast<uintptr_t>(gr) & 3) : -1;
        }
        for (int j = tid; j < cnt; j += 256) fl[j] = a.flags[rb + j];
        __syncthreads();
        auto row_src = [&](int R) -> const uint8_t* {
            if (rowoff[R] < 0) return nullptr;
            const int p = R - HR1;
            return call_row(R) ? a.cw_in + (rb + p) * a.stride : ring1 + ((sq + p) % kRR) * CW1;
        };
        if (tid < cnt) {
            int c = 0;
            for (int j = 0; j < tid; ++j) c += (fl[j] & 3) == kRecovered;
            cord[tid] = c;
        }
        int nrec = 0;
        for (int j = 0; j < cnt; ++j) nrec += (fl[j] & 3) == kRecovered;
        const uint8_t* gco = a.coefs + coef_off;
        if (nrec) burst_stage(smem, g.off_coef, gco, nrec * kn1, tid, 256);
        coefs = smem + g.off_coef + static_cast<int>(reinterpret_cast<uintptr_t>(gco) & 3);
        // dword w of staged row R (the row's first CW1 bytes from its dword phase on): batches of loads in flight
        const int nw = R1 * CWD1;
        for (int base = 0; base < nw; base += 256 * 4) {
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = base + q * 256 + tid;
                v[q] = 0;
                if (idx >= nw) continue;
                const int rr = fdiv(g.dcwd, idx), w = idx - rr * CWD1;
                const uint8_t* gr = row_src(rr);
                if (!gr) continue;
                const int ph = static_cast<int>(reinterpret_cast<uintptr_t>(gr) & 3);
                const int lo = 4 * w - ph;  // the dword's first byte in the row
                if (lo >= CW1) continue;
                if (lo >= 0 && lo + 4 <= CW1) {
                    v[q] = *reinterpret_cast<const uint32_t*>(gr + lo);
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (lo + e >= 0 && lo + e < CW1) v[q] |= uint32_t(gr[lo + e]) << (8 * e);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = base + q * 256 + tid;
                if (idx >= nw) continue;
                const int rr = fdiv(g.dcwd, idx), w = idx - rr * CWD1;
                *reinterpret_cast<uint32_t*>(smem + g.off_rows + rr * CWS1 + 4 * w) = v[q];
            }
        }
        __syncthreads();
        if (tid < cnt) {  // header bytes first: they bound the copy (both hops' clips: min(hdr, L))
            const int fate = fl[tid] & 3;
            int ln = 0;
            if (fate == kCopy || fate == kRecovered) ln = min(byte_at(tid, 0) * 256 + byte_at(tid, 1), L);
            lnS[tid] = ln;
        }
        __syncthreads();
        // window bytes 4q .. 4q+3 of message j: [len_hi, len_lo, payload, zero pad] (Encoder.cpp:75-83)
        for (int idx = tid; idx < cnt * nq; idx += 256) {
            const int j = fdiv(g.dnq, idx), q = idx - j * nq, r = prow0 + j;
            const int ln = lnS[j];
            const bool copy = (fl[j] & 3) == kCopy;
            const int ro = rowoff[j + k1 - 1];
            int s1 = fdiv(g.dk1, 4 * q), i1 = 4 * q - s1 * k1;
            int s2 = fdiv(g.dk2, 4 * q), i2 = 4 * q - s2 * k2;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = 4 * q + e;
                if (b < SK2) {
                    uint8_t v = 0;
                    if (b < 2)
                        v = b == 0 ? static_cast<uint8_t>(ln >> 8) : static_cast<uint8_t>(ln & 0xff);
                    else if (b < ln + 2)  // systematic byte of the message's own codeword, or through its block
                        v = copy ? (ro >= 0 ? smem[ro + s1 * n1 + i1] : uint8_t(0)) : byte_at(j, b);
                    planes[(i2 * ROWS2 + r) * SP2 + s2] = v;
                }
                if (++i1 == k1) i1 = 0, ++s1;
                if (++i2 == k2) i2 = 0, ++s2;
            }
        }
        return nrec;
    };

    // The burst's last received codewords and message windows into the rings, from the staged rows and
    // the planes (from window row prow0 on) of the pass that decoded cntp messages ending with the burst's last row
    // (first chunk only).
    const int m1 = min(u.total, T1 + k1);
    const int64_t early = T1 - u.seq0;  // rows of seq < T1: no message yet
    const int nmsg = early <= 0 ? u.total : (early >= u.total ? 0 : u.total - static_cast<int>(early));
    const int m2 = min(nmsg, H2);
    auto write_rings = [&](int cntp, int prow0) {
        for (int tt = tid >> 6; tt < m1; tt += 4) {  // missing ones leave their slot as it is
            const int ro = rowoff[HR1 + cntp - m1 + tt];
            if (ro >= 0) burst_flush(ring1 + ((u.seq0 + u.total - m1 + tt) % kRR) * CW1, smem, ro, CW1, tid & 63, 64);
        }
        for (int idx = tid; idx < m2 * nq; idx += 256) {
            const int tt = fdiv(g.dnq, idx), q = idx - tt * nq, r = prow0 + cntp - m2 + tt;
            uint8_t v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = min(4 * q + e, SK2 - 1);
                const int s = fdiv(g.dk2, b), i = b - s * k2;
                v[e] = planes[(i * ROWS2 + r) * SP2 + s];
            }
            uint8_t* dst = win2 + ((u.seq0 - T1 + u.total - m2 + tt) % W2) * SK2 + 4 * q;
            if ((SK2 & 3) == 0) {  // then dst is a dword address
                *reinterpret_cast<uint32_t*>(dst) = uint32_t(v[0]) | (uint32_t(v[1]) << 8) | (uint32_t(v[2]) << 16) |
                                                    (uint32_t(v[3]) << 24);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < SK2) dst[e] = v[e];
            }
        }
    };

    // ---- the windows of the H2 messages in front of the chunk: from the window ring (a message before
    // the flow's first is a zero window), or decoded again from the call's rows
    int nfront = 0;
    if (first) {
        for (int idx = tid; idx < H2 * nq; idx += 256) {
            const int r = fdiv(g.dnq, idx), q = idx - r * nq;
            const int64_t e = u.seq0 - T1 + r - H2;
            uint32_t w = 0;
            if (e >= 0) {
                const uint8_t* src = win2 + (e % W2) * SK2 + 4 * q;
                if ((SK2 & 3) == 0) {  // then src is a dword address
                    w = *reinterpret_cast<const uint32_t*>(src);
                } else {
                    for (int x = 0; x < 4; ++x)
                        if (4 * q + x < SK2) w |= uint32_t(src[x]) << (8 * x);
                }
            }
            int s = fdiv(g.dk2, 4 * q), i = 4 * q - s * k2;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                if (4 * q + x < SK2) planes[(i * ROWS2 + r) * SP2 + s] = static_cast<uint8_t>(w >> (8 * x));
                if (++i == k2) i = 0, ++s;
            }
        }
    } else {
        nfront = decode_pass(u.row0 - H2, u.seq0 - H2, H2, u.lead - H2, u.coef, 0);
        __syncthreads();  // its rows and row records give way to the chunk's own
    }
    // ---- the chunk's own messages
    decode_pass(u.row0, u.seq0, u.cnt, u.lead, u.coef + static_cast<int64_t>(nfront) * kn1, H2);
    __syncthreads();  // the planes are complete
    const bool far = u.total > u.cnt;  // the burst's last rows lie behind this chunk
    if (first) {
        if (!far) write_rings(u.cnt, H2);
        __syncthreads();  // the staged codewords give way to the hop-2 codewords
    }
    // ---- encode, as burst_encode_chunk: systematic bytes, parity columns, trimmed sizes, flush
    uint8_t* gcw = a.cw_out + u.row0 * OS;
    const int ao = g.off_rows + static_cast<int>(reinterpret_cast<uintptr_t>(gcw) & 3);
    uint8_t* out = smem + ao;  // the chunk's codewords, packed at CW2
    for (int idx = tid; idx < u.cnt * nq; idx += 256) {
        const int p = fdiv(g.dnq, idx), q = idx - p * nq;
        int s = fdiv(g.dk2, 4 * q), i = 4 * q - s * k2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * q + e < SK2) out[p * CW2 + s * n2 + i] = planes[(i * ROWS2 + p + H2) * SP2 + s];
            if (++i == k2) i = 0, ++s;
        }
    }
    // parity column j of four sub-streams: XOR_i G[i][j] * X_{t-(j-i)}[s][i]; rows without a message are zero
    for (int jj = 0; jj < np2; ++jj) {
        const int j = k2 + jj;
        for (int it = tid; it < u.cnt * NS4; it += 256) {
            const int p = fdiv(g.dns4, it), gq = it - p * NS4;
            uint32_t acc = 0;
            for (int i = 0; i < k2; ++i) {
                const uint32_t* t = tab + (i * np2 + jj) * 8;
                if (!t[5]) continue;
                const int r = p + H2 - (j - i);
                acc ^= gf_mul4x(t, *reinterpret_cast<const uint32_t*>(planes + (i * ROWS2 + r) * SP2 + 4 * gq));
            }
            uint8_t* o = out + p * CW2 + 4 * gq * n2 + j;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * gq + e < S2) o[e * n2] = static_cast<uint8_t>(acc >> (8 * e));
        }
    }
    __syncthreads();
    if (tid < u.cnt) {
        a.cw_len[u.row0 + tid] = last_nonzero_end(out + tid * CW2, CW2);  // FEC_Encoder.cpp:55-60
        if (a.fate) a.fate[u.row0 + tid] = a.flags[u.row0 + tid] & 3;
    }
    if (OS == CW2) {
        burst_flush(gcw, smem, ao, u.cnt * CW2, tid, 256);
    } else {  // a wave per row: the pair's codeword, then zeros up to the group's stride
        for (int t = tid >> 6; t < u.cnt; t += 4) {
            burst_flush(gcw + static_cast<int64_t>(t) * OS, smem, ao + t * CW2, CW2, tid & 63, 64);
            burst_zero(gcw + static_cast<int64_t>(t) * OS + CW2, OS - CW2, tid & 63, 64);
        }
    }
    if (!first || !far) return;
    // ---- first chunk of a burst cut in several: the burst's last rows again, for the rings
    __syncthreads();
    const int mt = max(m2, 1);
    decode_pass(u.row0 + u.total - mt, u.seq0 + u.total - mt, mt, u.total - mt, u.tail_coef, 0);
    __syncthreads();
    write_rings(mt, 0);
}

// Two kernels that differ only in where the chunk's geometry comes from.
__global__ __launch_bounds__(256) void fec_mw_relay_streams_kernel(MwArgs a) {
    const MwUnit u = a.r.units[blockIdx.x];
    mw_chunk(a.r, a.g, u, a.r.ring1 + static_cast<int64_t>(u.id) * kRR * a.g.CW1,
             a.r.win2 + static_cast<int64_t>(u.id) * a.g.W2 * a.g.SK2, a.g.CW2);
}

// A unit names its pair, the same for the whole workgroup (readfirstlane), so the table entry arrives by
// scalar loads; the chunk-size part is worked out here from the call's longest burst, as the host did for
// the launch's LDS.
__global__ __launch_bounds__(256) void fec_mw_relay_streams_mixed_kernel(MwMixedArgs a) {
    const MwUnit u = a.r.units[blockIdx.x];
    const MwCode* c = a.codes + __builtin_amdgcn_readfirstlane(u.code);
    MwGeom g = c->g;
    mw_carve(&g, min(a.cap, c->tpmax));
    mw_chunk(a.r, g, u, a.r.ring1 + static_cast<int64_t>(u.id) * a.slot1, a.r.win2 + static_cast<int64_t>(u.id) * a.slot2,
             a.out_stride);
}

// Both codes' constants and the fast dividers of a pair: the geometry but the pointers and the
// chunk-size part (mw_carve)
void mw_consts(const Geometry& g1, const Geometry& g2, MwGeom* a) {
    a->L = g1.L, a->T1 = g1.T, a->k1 = g1.k, a->n1 = g1.n, a->CW1 = g1.CW;
    a->CWD1 = (g1.CW + 6) >> 2;
    a->CWS1 = 4 * a->CWD1;
    a->HR1 = g1.T + g1.k - 1;
    a->k2 = g2.k, a->n2 = g2.n, a->S2 = g2.S, a->CW2 = g2.CW, a->SK2 = g2.S * g2.k;
    a->NS4 = (g2.S + 3) / 4;
    a->SP2 = 4 * a->NS4;
    a->H2 = g2.n - 1;
    a->W2 = std::max(1, a->H2);
    a->dk1 = fast_div(g1.k);
    a->dk2 = fast_div(g2.k);
    a->dns4 = fast_div(a->NS4);
    a->dnq = fast_div((a->SK2 + 3) >> 2);
    a->dcwd = fast_div(a->CWD1);
}

// The chunk of a burst cut in several: the most packets <= kChunkTP whose LDS fits, at least the HR1 + H2
// a later chunk needs in front of it.  0: not even that fits.
int mw_fit(const Geometry& g1, const Geometry& g2, MwGeom* a, int* lds) {
    mw_consts(g1, g2, a);
    const int front = std::max(1, g1.T + g1.k - 1 + g2.n - 1);
    for (int tp = kChunkTP; tp >= front; --tp) {
        *lds = mw_carve(a, tp);
        if (*lds <= kCuLds) return tp;
    }
    return 0;
}

}  // namespace
}  // namespace fec

struct fec_mw_relay_streams {
    struct Hop {                             // one hop code (T, B, N): shared by every pair that uses it on either hop
        int T = 0, B = 0, N = 0;
        fec_codec* codec = nullptr;          // hop 1: the GF tables; hop 2: the parity tables
        std::shared_ptr<const fec::DecodeRules> rules;  // as a hop-1 code
    };
    struct Pair {
        fec::Geometry g1, g2;
        int hop1 = 0;                        // its hop-1 code in `hops`
        fec::MwCode code;                    // as the kernels take it (the mixed kernel's table entry), pointers set
    };
    std::unique_ptr<StepPool> pool;          // symbolic steps of large calls (FEC_STREAMS_THREADS)
    std::vector<Hop> hops;
    std::vector<Pair> pairs;
    fec::MwCode* d_codes = nullptr;          // the pairs' table on the device (mixed groups)
    bool mixed = false;                      // made by fec_mw_relay_streams_create_mixed: the table-driven kernel
    int nstreams = 0;
    int cw1_min = 0, cw2_stride = 0;         // the largest S1*n1 and S2*n2 of the pairs: the row strides
    int64_t slot1 = 0, slot2 = 0;            // a flow's codeword ring slot and window slot: hold any pair
    std::vector<int32_t> code_of;            // per flow
    std::vector<std::unique_ptr<fec::StreamPlanner>> planners;
    std::vector<int64_t> seq;                // hop-1 packets fed so far per flow
    uint8_t* d_ring1 = nullptr;
    uint8_t* d_win2 = nullptr;
    fec::GroupStage stage;                   // per-call records: chunks, row flags, coefficient blocks
    ~fec_mw_relay_streams() {
        for (void* p : {static_cast<void*>(d_ring1), static_cast<void*>(d_win2), static_cast<void*>(d_codes)})
            if (p) (void)hipFree(p);
        for (Hop& hp : hops)
            if (hp.codec) fec_codec_destroy(hp.codec);
    }
};

namespace {

int mw_relay_call(fec_mw_relay_streams* h, const int32_t* ids, const int32_t* counts, int M, const uint8_t* erasure,
                  const uint8_t* d_cw1, int64_t cw1_stride, uint8_t* d_cw2, int32_t* d_cw2_len, uint8_t* d_fate,
                  hipStream_t s) {
    if (M < 0 || M > h->nstreams) return FEC_ERR_ARG;
    if (M == 0) return FEC_OK;
    if (!ids || !erasure || !d_cw1 || !d_cw2 || !d_cw2_len || cw1_stride < h->cw1_min) return FEC_ERR_ARG;
    fec::GroupStage& stage = h->stage;
    int64_t R = 0;
    int maxc = 0;
    if (int st = fec::check_counts(counts, M, &R, &maxc)) return st;
    if (int st = stage.check_ids(ids, M)) return st;
    // A pair's bursts are one chunk each when the call's longest fits its chunk; else chunks of tpmax >=
    // HR1 + H2.  The launch takes the LDS of the largest chunk among the pairs present in the call.
    int tp_of[fec::kMwMaxCodes];
    std::fill(tp_of, tp_of + h->pairs.size(), 0);
    int lds = 0;
    int64_t nu = 0;
    for (int m = 0; m < M; ++m) {
        const int c = h->code_of[ids[m]];
        if (!tp_of[c]) {
            tp_of[c] = std::min(maxc, h->pairs[c].code.tpmax);
            fec::MwGeom g = h->pairs[c].code.g;
            lds = std::max(lds, fec::mw_carve(&g, tp_of[c]));
        }
        nu += ((counts ? counts[m] : 1) + tp_of[c] - 1) / tp_of[c];
    }
    if (nu > INT32_MAX) return FEC_ERR_ARG;
    const void* kern = h->mixed ? reinterpret_cast<const void*>(fec::fec_mw_relay_streams_mixed_kernel)
                                : reinterpret_cast<const void*>(fec::fec_mw_relay_streams_kernel);
    static int lds_raised[2] = {0, 0};  // per kernel, not per group
    if (int st = fec::lds_allow(kern, lds, &lds_raised[h->mixed])) return st;
    if (int st = stage.begin(s)) return st;
    fec::StageGuard guard{stage};  // the symbolic decoders advance before the launch
    DecodePlan<fec::MwUnit> plan;
    const bool ok = plan.plan(
        h->pool.get(), counts, M, R, [&](int m) { return tp_of[h->code_of[ids[m]]]; },
        [&](int m, int64_t row0, int cnt, fec::MwUnit* u, uint8_t* fl, std::vector<uint8_t>& coefs) {
            const int id = ids[m], c = h->code_of[id], tp = tp_of[c];
            const fec::Geometry& g1 = h->pairs[c].g1;
            const int kn1 = g1.k * g1.n, H2 = h->pairs[c].g2.n - 1;
            const int64_t seq = h->seq[id], base = static_cast<int64_t>(coefs.size());
            plan_burst_rows(*h->planners[id], g1.T, kn1, seq, erasure + row0, cnt, fl, coefs);
            // a flow's recovered rows keep their blocks in row order, so the blocks of any run of its rows
            // are one range; a chunk's start with those of its first decoded row: H2 rows in front of a
            // later chunk
            int pos = 0;
            int64_t rec = 0;
            auto blocks_before = [&](int row) {
                for (; pos < row; ++pos) rec += (fl[pos] & 3) == fec::kRecovered;
                return base + rec * kn1;
            };
            fec::MwUnit* first = u;
            for (int lead = 0; lead < cnt; lead += tp, ++u) {
                u->row0 = row0 + lead;
                u->seq0 = seq + lead;
                u->coef = blocks_before(std::max(lead - H2, 0));
                u->tail_coef = 0;
                u->id = id;
                u->cnt = static_cast<int16_t>(std::min(tp, cnt - lead));
                u->code = static_cast<int16_t>(c);
                u->lead = lead;
                u->total = cnt;
            }
            if (cnt > tp) {  // the first chunk decodes the burst's last max(min(messages, H2), 1) rows again
                const int nmsg = cnt - static_cast<int>(std::min<int64_t>(std::max<int64_t>(g1.T - seq, 0), cnt));
                first->tail_coef = blocks_before(cnt - std::max(std::min(nmsg, H2), 1));
            }
        },
        [](fec::MwUnit& u, int64_t by) { u.coef += by, u.tail_coef += by; });
    if (!ok) return FEC_ERR_ARG;
    if (int st = stage.reserve(plan.bytes)) return st;
    plan.write(stage.host());
    const size_t off_flags = plan.off_flags, off_coef = plan.off_coef;
    const uint8_t* rec = stage.device();
    fec::MwRows r{};
    r.cw_in = d_cw1;
    r.stride = cw1_stride;
    r.flags = rec + off_flags;
    r.coefs = rec + off_coef;
    r.cw_out = d_cw2;
    r.cw_len = d_cw2_len;
    r.fate = d_fate;
    r.units = reinterpret_cast<const fec::MwUnit*>(rec);
    r.ring1 = h->d_ring1;
    r.win2 = h->d_win2;
    const dim3 grid(static_cast<unsigned>(nu)), block(256);
    if (h->mixed) {
        const fec::MwMixedArgs a{r, h->d_codes, h->slot1, h->slot2, h->cw2_stride, maxc};
        hipLaunchKernelGGL(fec::fec_mw_relay_streams_mixed_kernel, grid, block, static_cast<size_t>(lds), s, a);
    } else {
        fec::MwArgs a{r, h->pairs[0].code.g};
        fec::mw_carve(&a.g, tp_of[0]);
        hipLaunchKernelGGL(fec::fec_mw_relay_streams_kernel, grid, block, static_cast<size_t>(lds), s, a);
    }
    if (int st = stage.commit(s)) return st;
    for (int m = 0; m < M; ++m) h->seq[ids[m]] += counts ? counts[m] : 1;
    return FEC_OK;
}

// Whether a pair {T1,B1,N1,T2,B2,N2} can run at this payload size (what create asks before it allocates):
// both tuples ones the stream kernels take, and the smallest chunk of a cut burst within 32 packets and a
// CU's LDS.  code->g: the pair's constants without the pointers, its chunk-size part at tpmax.
bool mw_pair_fits(int max_payload, const int32_t* t, fec::Geometry* g1, fec::Geometry* g2, fec::MwCode* code, int* lds) {
    if (!fec::stream_tuple(max_payload, t[0], t[1], t[2], g1) || !fec::stream_tuple(max_payload, t[3], t[4], t[5], g2))
        return false;
    *code = fec::MwCode{};
    code->tpmax = fec::mw_fit(*g1, *g2, &code->g, lds);
    return code->tpmax != 0;
}

// The group's hop code (T, B, N), made on first use.  *idx: its place in h->hops.
int mw_hop(fec_mw_relay_streams* h, int max_payload, int T, int B, int N, int* idx) {
    int i = 0;
    while (i < static_cast<int>(h->hops.size()) && (h->hops[i].T != T || h->hops[i].B != B || h->hops[i].N != N)) ++i;
    if (i == static_cast<int>(h->hops.size())) {
        h->hops.emplace_back();
        h->hops[i].T = T, h->hops[i].B = B, h->hops[i].N = N;
        if (int st = fec_codec_create(max_payload, T, B, N, &h->hops[i].codec)) return st;
        h->hops[i].rules = fec::shared_decode_rules(T, B, N);
    }
    *idx = i;
    return FEC_OK;
}

// A group of ncodes pairs {T1,B1,N1,T2,B2,N2}; code_of null: every flow on pair 0.  Everything that can
// refuse the arguments comes before the first allocation.
int mw_create(int max_payload, const int32_t* pairs, int ncodes, const int32_t* code_of, int nstreams, bool mixed,
              fec_mw_relay_streams** out) {
    try {
        std::vector<fec_mw_relay_streams::Pair> pr(ncodes);
        for (int c = 0; c < ncodes; ++c) {
            int lds = 0;
            if (!mw_pair_fits(max_payload, pairs + 6 * c, &pr[c].g1, &pr[c].g2, &pr[c].code, &lds)) return FEC_ERR_ARG;
        }
        std::unique_ptr<fec_mw_relay_streams> h(new fec_mw_relay_streams());
        h->nstreams = nstreams;
        h->mixed = mixed;
        if (code_of)
            h->code_of.assign(code_of, code_of + nstreams);
        else
            h->code_of.assign(nstreams, 0);
        size_t kn_max = 0;
        for (int c = 0; c < ncodes; ++c) {
            const int32_t* t = pairs + 6 * c;
            int i2 = 0;
            if (int st = mw_hop(h.get(), max_payload, t[0], t[1], t[2], &pr[c].hop1)) return st;
            if (int st = mw_hop(h.get(), max_payload, t[3], t[4], t[5], &i2)) return st;
            fec::CodecView v1, v2;
            if (int st = fec::codec_view(h->hops[pr[c].hop1].codec, &v1)) return st;
            if (int st = fec::codec_view(h->hops[i2].codec, &v2)) return st;
            const fec::MwGeom& g = pr[c].code.g;
            pr[c].code.g.gf = v1.gf;
            pr[c].code.g.ptab = v2.ptab;
            h->cw1_min = std::max(h->cw1_min, g.CW1);
            h->cw2_stride = std::max(h->cw2_stride, g.CW2);
            // a one-code group's kernel places a flow's window slot itself, at W2 * SK2; a mixed group's slots
            // start at dword addresses, as the window rows of a pair with SK2 % 4 == 0 need
            const size_t win = static_cast<size_t>(g.W2) * g.SK2;
            h->slot2 = std::max(h->slot2, static_cast<int64_t>(mixed ? fec::align16(win) : win));
            kn_max = std::max(kn_max, static_cast<size_t>(g.k1) * g.n1);
        }
        h->slot1 = static_cast<int64_t>(fec::kRR) * h->cw1_min;
        h->pairs = std::move(pr);
        h->planners.resize(nstreams);
        for (int i = 0; i < nstreams; ++i) {
            const fec_mw_relay_streams::Pair& p = h->pairs[h->code_of[i]];
            h->planners[i].reset(new fec::StreamPlanner(p.g1, h->hops[p.hop1].rules.get()));
        }
        h->pool = make_step_pool(nstreams);
        h->seq.assign(nstreams, 0);
        const size_t rb = static_cast<size_t>(nstreams) * h->slot1;
        const size_t wb = static_cast<size_t>(nstreams) * h->slot2;
        FEC_HIP(hipMalloc(&h->d_ring1, rb));
        FEC_HIP(hipMemset(h->d_ring1, 0, rb));
        FEC_HIP(hipMalloc(&h->d_win2, wb));
        FEC_HIP(hipMemset(h->d_win2, 0, wb));
        if (mixed) {
            std::vector<fec::MwCode> tab(ncodes);
            for (int c = 0; c < ncodes; ++c) tab[c] = h->pairs[c].code;
            FEC_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_codes), tab.size() * sizeof(fec::MwCode)));
            FEC_HIP(hipMemcpy(h->d_codes, tab.data(), tab.size() * sizeof(fec::MwCode), hipMemcpyHostToDevice));
        }
        // a call of one packet per flow fits its buffer: sized by the largest coefficient block
        const size_t stage = static_cast<size_t>(nstreams) * (sizeof(fec::MwUnit) + 1 + kn_max + 16) + 64;
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

int fec_mw_relay_streams_fit(int max_payload, int T1, int B1, int N1, int T2, int B2, int N2, int* chunk_packets,
                             int* lds_bytes) {
    const int32_t pair[6] = {T1, B1, N1, T2, B2, N2};
    fec::Geometry g1, g2;
    fec::MwCode code;
    int lds = 0;
    if (!mw_pair_fits(max_payload, pair, &g1, &g2, &code, &lds)) return FEC_ERR_ARG;
    if (chunk_packets) *chunk_packets = code.tpmax;
    if (lds_bytes) *lds_bytes = lds;
    return FEC_OK;
}

int fec_mw_relay_streams_mixed_fit(int max_payload, const int32_t* pairs, int ncodes, int32_t* chunk, int32_t* lds) {
    if (!pairs || ncodes < 1 || ncodes > fec::kMwMaxCodes || !chunk || !lds) return FEC_ERR_ARG;
    for (int c = 0; c < ncodes; ++c) {
        fec::Geometry g1, g2;
        fec::MwCode code;
        int b = 0;
        if (!mw_pair_fits(max_payload, pairs + 6 * c, &g1, &g2, &code, &b)) return FEC_ERR_ARG;
        chunk[c] = code.tpmax, lds[c] = b;
    }
    return FEC_OK;
}

int fec_mw_relay_streams_create(int max_payload, int T1, int B1, int N1, int T2, int B2, int N2, int nstreams,
                                fec_mw_relay_streams** out) {
    if (!out) return FEC_ERR_ARG;
    *out = nullptr;
    if (nstreams <= 0) return FEC_ERR_ARG;
    const int32_t pair[6] = {T1, B1, N1, T2, B2, N2};
    return mw_create(max_payload, pair, 1, nullptr, nstreams, false, out);
}

int fec_mw_relay_streams_create_mixed(int max_payload, const int32_t* pairs, int ncodes, const int32_t* code_of,
                                      int nstreams, fec_mw_relay_streams** out) {
    if (!out) return FEC_ERR_ARG;
    *out = nullptr;
    if (!pairs || !code_of || ncodes < 1 || ncodes > fec::kMwMaxCodes || nstreams <= 0) return FEC_ERR_ARG;
    for (int i = 0; i < nstreams; ++i)
        if (code_of[i] < 0 || code_of[i] >= ncodes) return FEC_ERR_ARG;
    return mw_create(max_payload, pairs, ncodes, code_of, nstreams, true, out);
}

int fec_mw_relay_streams_destroy(fec_mw_relay_streams* h) {
    delete h;
    return FEC_OK;
}

int fec_mw_relay_streams_codes(const fec_mw_relay_streams* h, int* ncodes, int* cw1_bytes, int* cw2_stride) {
    if (!h) return FEC_ERR_ARG;
    if (ncodes) *ncodes = static_cast<int>(h->pairs.size());
    if (cw1_bytes) *cw1_bytes = h->cw1_min;
    if (cw2_stride) *cw2_stride = h->cw2_stride;
    return FEC_OK;
}

int fec_mw_relay_streams_stream_geometry(const fec_mw_relay_streams* h, int id, int* code, int* k1, int* n1, int* k2,
                                         int* n2, int* cw1_bytes, int* cw2_bytes, int* delay) {
    if (!h || id < 0 || id >= h->nstreams) return FEC_ERR_ARG;
    const int c = h->code_of[id];
    const fec::MwGeom& g = h->pairs[c].code.g;
    if (code) *code = c;
    if (k1) *k1 = g.k1;
    if (n1) *n1 = g.n1;
    if (k2) *k2 = g.k2;
    if (n2) *n2 = g.n2;
    if (cw1_bytes) *cw1_bytes = g.CW1;
    if (cw2_bytes) *cw2_bytes = g.CW2;
    if (delay) *delay = g.T1;
    return FEC_OK;
}

int fec_mw_relay_streams_geometry(const fec_mw_relay_streams* h, int* cw1_bytes, int* cw2_bytes, int* delay) {
    if (!h || h->pairs.size() != 1) return FEC_ERR_ARG;
    return fec_mw_relay_streams_stream_geometry(h, 0, nullptr, nullptr, nullptr, nullptr, nullptr, cw1_bytes, cw2_bytes,
                                                delay);
}

int fec_mw_relay_streams_set_code(fec_mw_relay_streams* h, int id, int code) {
    if (!h || id < 0 || id >= h->nstreams || code < 0 || code >= static_cast<int>(h->pairs.size())) return FEC_ERR_ARG;
    try {
        // host work only: a chunk reads a codeword ring row only for a hop-1 seq >= 0 and a window row only
        // for a message number >= 0 of the flow's current life, and every such row was written in this
        // life, so the slot's old bytes are never seen; calls already queued carry their own seqs and
        // pairs in their staged records
        const fec_mw_relay_streams::Pair& p = h->pairs[code];
        std::unique_ptr<fec::StreamPlanner> pl(new fec::StreamPlanner(p.g1, h->hops[p.hop1].rules.get()));
        h->planners[id] = std::move(pl);
        h->code_of[id] = code;
        h->seq[id] = 0;
        return FEC_OK;
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

int fec_mw_relay_streams_relay(fec_mw_relay_streams* h, const int32_t* ids, const int32_t* counts, int M,
                               const uint8_t* erasure, const uint8_t* d_cw1, int64_t cw1_stride, uint8_t* d_cw2,
                               int32_t* d_cw2_len, uint8_t* d_fate, void* stream) {
    if (!h) return FEC_ERR_ARG;
    try {
        return mw_relay_call(h, ids, counts, M, erasure, d_cw1, cw1_stride, d_cw2, d_cw2_len, d_fate,
                             static_cast<hipStream_t>(stream));
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

int fec_mw_relay_streams_state(const fec_mw_relay_streams* h, int id, int64_t* received, int64_t* forwarded) {
    if (!h || id < 0 || id >= h->nstreams) return FEC_ERR_ARG;
    if (received) *received = h->seq[id];
    if (forwarded) *forwarded = std::max<int64_t>(h->seq[id] - h->pairs[h->code_of[id]].g1.T, 0);
    return FEC_OK;
}

}  // extern "C"

