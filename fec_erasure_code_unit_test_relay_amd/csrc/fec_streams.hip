// fec_streams.hip -- many independent streams of one (T,B,N), one packet of each per call, coded in
// one launch (north_star: "many independent (T,B,N) coding windows batched across wavefronts").
//
// The reference runs one FEC_Encoder / FEC_Decoder per stream (include/FEC_Encoder.h:26-48,
// FEC_Decoder.h:27-46), one packet per onTransmit / onReceive call, and keeps each stream's state
// inside those objects.  Here a group holds the state of N streams in HBM:
//   * encoder: the last n-1 windows X_{t-1..t-n+1} of every stream (bytes [len_hi, len_lo,
//     payload, zero pad] of S*k bytes, Encoder.cpp:73-95), a ring indexed by seq % (n-1);
//   * decoder: the last RR received codewords of every stream (zero padded like
//     FEC_Decoder.cpp:55-63), a ring indexed by seq % RR, and per stream the symbolic planner
//     (fec::StreamPlanner, the reference decoder's state machine without the bytes) on the host.
// A call names M distinct streams and hands over one packet of each; one wave per packet does
// its byte work: the encoder's closed form (Encoder.cpp:65-98 -> codingOperations.cpp:131-147)
// over the stream's window, or the decoder's output for packet seq - T (fast path copy,
// Decoder.cpp:77-108, or the planner's recovery coefficients, codingOperations.cpp:149-232).
// A burst call (fec_streams_encode_burst / fec_streams_decode_burst) hands over several consecutive
// packets of each stream and equals that many one-packet calls; its kernels work on chunks of a
// burst and touch the per-stream state only at the burst's two ends (see "bursts" below).
// A mixed group (fec_streams_create_mixed) gives every stream its own (T,B,N): its calls run the same
// chunk bodies through kernels that take each chunk's geometry from a per-code table (see "bursts").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstring>
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

struct StreamsEncArgs {
    const uint8_t* payload;  // M rows of L bytes
    const int32_t* len;      // M payload sizes (null: all L)
    const int32_t* ids;      // M stream ids
    const int64_t* seq;      // M: packets the stream sent before this one
    uint8_t* win;            // [streams][W][SK] window ring
    uint8_t* cw;             // M rows of CW bytes
    int32_t* cw_len;         // M trimmed sizes
    const uint8_t* G;        // k x n
    const uint8_t* gf;       // exp[512], log[256]
    int M, L, k, n, S, CW, SK, W;
    // single-packet calls (stream_encode_one): seq / ids / len null -> seq1, stream 0, len1; after the
    // packet's outputs the wave stores ticket into the host-visible word `done` (null: none)
    int64_t seq1;
    int len1;
    uint32_t* done;
    uint32_t ticket;
};

struct StreamItem {
    int32_t id;
    int32_t fate;    // PacketFate of the packet output by this call (x = seq - T)
    int32_t clamp;   // slow path: payload clamped to L (Decoder.cpp:148-149)
    int32_t coef;    // kRecovered: index of its k x n block in coefs
    int64_t seq;     // packets the stream received before this one
    int64_t x;       // packet output by this call
    int32_t erased;  // this call's packet is missing
    int32_t pad;
};

struct StreamsDecArgs {
    const uint8_t* cw_in;    // M rows of CW bytes (rows of erased packets are not read)
    const StreamItem* items;
    const uint8_t* coefs;    // recovered outputs' coefficient blocks
    uint8_t* ring;           // [streams][RR][CW]
    const uint8_t* gf;
    uint8_t* out;            // M rows of L bytes
    int32_t* out_len;
    int M, L, k, n, CW, RR;
    // single-packet calls (stream_decode_one): items null -> item1; after the outputs the wave stores
    // ticket into the host-visible word `done` (null: none)
    StreamItem item1;
    uint32_t* done;
    uint32_t ticket;
};

// Single-packet calls (stream_encode_one, M == 1): the whole workgroup on the one codeword, a thread
// per codeword byte, so that no thread walks a long chain of table lookups (the per-packet
// FEC_Encoder's latency).  prow / wst / rowoff / cwl are the kernel's LDS (wave 0's slices).
__device__ __forceinline__ void single_packet_encode(const StreamsEncArgs& a, int tid, const uint8_t* gexp,
                                                     const uint8_t* glog, const uint8_t* Gs, const uint8_t* pay,
                                                     const uint32_t* wst, int* ro, uint32_t* cwl) {
    __shared__ int last_nz;
    const int L = a.L, k = a.k, n = a.n, CW = a.CW, SK = a.SK, W = a.W;
    const int ln = min(max(a.len1, 0), L);
    const int64_t seq = a.seq1;
    if (tid < 32) ro[tid] = (tid >= 1 && seq - tid >= 0) ? static_cast<int>((seq - tid) % W) * SK : -1;
    if (tid == 0) last_nz = -1;
    __syncthreads();  // payload row, window, offsets
    auto xbyte = [&](int b) -> uint8_t {  // [len_hi, len_lo, payload, zero pad] (Encoder.cpp:75-83)
        return b == 0 ? static_cast<uint8_t>(ln >> 8)
                      : b == 1 ? static_cast<uint8_t>(ln & 0xff) : (b - 2 < ln ? pay[b - 2] : 0);
    };
    const bool lds_out = CW <= 2048 && (reinterpret_cast<uintptr_t>(a.cw) & 3) == 0;
    uint8_t* cwb = lds_out ? reinterpret_cast<uint8_t*>(cwl) : a.cw;
    int last = -1;
    for (int c = tid; c < CW; c += 256) {
        const int s = c / n, j = c - s * n;
        uint8_t v = 0;
        if (j < k) {
            v = xbyte(s * k + j);
        } else {  // parity: XOR_i G[i][j] * X_{t-(j-i)}[s][i], rows before the stream start = 0
            for (int i = 0; i < k; ++i) {
                const int r = ro[j - i];
                if (r < 0) continue;
                const int o = r + s * k + i;
                const uint8_t xb = wst ? reinterpret_cast<const uint8_t*>(wst)[o] : a.win[o];
                v ^= gmul(gexp, glog, Gs[i * n + j], xb);
            }
        }
        cwb[c] = v;
        if (v) last = c;
    }
    if (last >= 0) atomicMax(&last_nz, last);
    __syncthreads();  // codeword complete; the window slot of seq - W (= seq % W) has been read
    const int own = static_cast<int>(seq % W) * SK;
    for (int b = tid; b < SK; b += 256) a.win[own + b] = xbyte(b);
    if (lds_out)
        for (int w = tid; 4 * w < CW; w += 256) reinterpret_cast<uint32_t*>(a.cw)[w] = cwl[w];
    if (tid == 0) a.cw_len[0] = last_nz + 1;  // FEC_Encoder.cpp:55-60
    if (a.done) {  // every thread's stores complete, then the completion word
        __threadfence_system();
        __syncthreads();
        if (tid == 0) *reinterpret_cast<volatile uint32_t*>(a.done) = a.ticket;
    }
}

// One wave per packet: lane = sub-stream (and sub-stream + 64, ...).
__global__ __launch_bounds__(256) void fec_streams_encode_kernel(StreamsEncArgs a) {
    __shared__ uint8_t gexp[512];
    __shared__ uint8_t glog[256];
    __shared__ uint8_t Gs[16 * 32];
    __shared__ uint32_t prow[4][376];  // each wave's payload row (L <= 1500), read once with dword loads
    __shared__ uint32_t wst[4][1024];  // each wave's window ring when it fits 4 KB: all loads in flight
    __shared__ uint32_t cwst[512];     // single-packet calls: the codeword (CW <= 2048)
    __shared__ int rowoff[4][32];      // per wave: window offset of packet seq - d (-1: before the stream)
    const int tid = threadIdx.x;
    for (int i = tid; i < 512; i += 256) gexp[i] = a.gf[i];
    for (int i = tid; i < 256; i += 256) glog[i] = a.gf[512 + i];
    for (int i = tid; i < a.k * a.n; i += 256) Gs[i] = a.G[i];
    const int m = blockIdx.x * 4 + (tid >> 6), lane = tid & 63;
    if (m < a.M) {  // the payload may be a host-visible row: all loads in flight at once
        const uint8_t* src = a.payload + static_cast<int64_t>(m) * a.L;
        uint8_t* dst = reinterpret_cast<uint8_t*>(prow[tid >> 6]);
        if (((a.L | static_cast<int>(reinterpret_cast<uintptr_t>(src))) & 3) == 0) {
            for (int w = lane; 4 * w < a.L; w += 64) prow[tid >> 6][w] = reinterpret_cast<const uint32_t*>(src)[w];
        } else {
            for (int b = lane; b < a.L; b += 64) dst[b] = src[b];
        }
    }
    const int wbytes = a.W * a.SK;
    const bool wlds = wbytes <= 4096 && (wbytes & 3) == 0;
    if (m < a.M && wlds) {
        const uint32_t* wsrc = reinterpret_cast<const uint32_t*>(a.win + static_cast<int64_t>(a.ids ? a.ids[m] : 0) * wbytes);
        for (int w = lane; 4 * w < wbytes; w += 64) wst[tid >> 6][w] = wsrc[w];
    }
    if (!a.ids) {
        single_packet_encode(a, tid, gexp, glog, Gs, reinterpret_cast<const uint8_t*>(prow[0]), wlds ? wst[0] : nullptr,
                             rowoff[0], cwst);
        return;
    }
    __syncthreads();
    if (m >= a.M) return;
    const int L = a.L, k = a.k, n = a.n, S = a.S, CW = a.CW, SK = a.SK, W = a.W;
    const int ln = min(max(a.len ? a.len[m] : a.len1, 0), L);
    const int64_t seq = a.seq ? a.seq[m] : a.seq1;
    uint8_t* win = a.win + static_cast<int64_t>(a.ids ? a.ids[m] : 0) * W * SK;
    const uint8_t* pay = reinterpret_cast<const uint8_t*>(prow[tid >> 6]);
    uint8_t* cwo = a.cw + static_cast<int64_t>(m) * CW;
    // single-packet calls write the codeword into LDS first, then to the (host-visible) result row
    // in dwords (the row is padded to whole dwords)
    const bool lds_out = !a.ids && CW <= 2048 && (reinterpret_cast<uintptr_t>(cwo) & 3) == 0;
    uint8_t* cwl = reinterpret_cast<uint8_t*>(cwst);
    // window byte b of this packet: [len_hi, len_lo, payload, zero pad] (Encoder.cpp:75-83)
    auto xbyte = [&](int b) -> uint8_t {
        return b == 0 ? static_cast<uint8_t>(ln >> 8)
                      : b == 1 ? static_cast<uint8_t>(ln & 0xff) : (b - 2 < ln ? pay[b - 2] : 0);
    };
    int* ro = rowoff[tid >> 6];
    if (lane < 32) ro[lane] = (lane >= 1 && seq - lane >= 0) ? static_cast<int>((seq - lane) % W) * SK : -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int own = static_cast<int>(seq % W) * SK;
    int last = -1;  // last non-zero codeword byte of this lane's sub-streams
    for (int s = lane; s < S; s += 64) {
        for (int j = 0; j < n; ++j) {
            uint8_t v;
            if (j < k) {
                v = xbyte(s * k + j);
            } else {  // parity: XOR_i G[i][j] * X_{t-(j-i)}[s][i], rows before the stream start = 0
                v = 0;
                for (int i = 0; i < k; ++i) {
                    const int r = ro[j - i];
                    if (r < 0) continue;
                    const int o = r + s * k + i;
                    const uint8_t xb = wlds ? reinterpret_cast<const uint8_t*>(wst[tid >> 6])[o] : win[o];
                    v ^= gmul(gexp, glog, Gs[i * n + j], xb);
                }
            }
            if (lds_out)
                cwl[s * n + j] = v;
            else
                cwo[s * n + j] = v;
            if (v) last = s * n + j;
        }
        // this lane's own bytes of slot seq % W: read above (d = W), now overwritten
        for (int i = 0; i < k; ++i) win[own + s * k + i] = xbyte(s * k + i);
    }
    if (lds_out) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int w = lane; 4 * w < CW; w += 64) reinterpret_cast<uint32_t*>(cwo)[w] = cwst[w];
    }
    for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d, 64));
    if (lane == 0) a.cw_len[m] = last + 1;  // FEC_Encoder.cpp:55-60
    if (a.done) {  // every lane's stores complete, then the completion word (one wave: M == 1)
        __threadfence_system();
        if (lane == 0) *reinterpret_cast<volatile uint32_t*>(a.done) = a.ticket;
    }
}

// Packet it.x from the symbols sym(packet, offset): a copy or the planner's recovery coefficients.
template <class Sym>
__device__ __forceinline__ void stream_output(const StreamsDecArgs& a, const StreamItem& it, uint8_t* orow, int m,
                                              int lane, const uint8_t* gexp, const uint8_t* glog, Sym sym) {
    const int L = a.L, k = a.k, n = a.n;
    const uint8_t* coef = a.coefs + static_cast<int64_t>(it.coef) * k * n;
    // header bytes 0, 1 (sub-stream 0, positions 0 and 1 -> (1/k)*n + 1%k) first: they bound the copy
    auto byte_at = [&](int h) -> uint8_t {
        const int s = h / k, i = h - s * k;
        if (it.fate == kCopy) return sym(it.x, s * n + i);
        uint8_t acc = 0;
        for (int q = 0; q < n; ++q) {
            const uint8_t c = coef[i * n + q];
            if (c) acc ^= gmul(gexp, glog, c, sym(it.x - i + q, s * n + q));
        }
        return acc;
    };
    const int hdr = byte_at(0) * 256 + byte_at(1);
    const int ln = it.clamp ? min(hdr, L) : hdr;
    const int cp = min(ln, L);
    for (int b = lane; b < L; b += 64) orow[b] = b < cp ? byte_at(b + 2) : 0;
    if (lane == 0) a.out_len[m] = ln;
}

// One wave per packet: store the received codeword in the stream's ring, output packet x.
__global__ __launch_bounds__(256) void fec_streams_decode_kernel(StreamsDecArgs a) {
    __shared__ uint8_t gexp[512];
    __shared__ uint8_t glog[256];
    const int tid = threadIdx.x;
    for (int i = tid; i < 512; i += 256) gexp[i] = a.gf[i];
    for (int i = tid; i < 256; i += 256) glog[i] = a.gf[512 + i];
    __syncthreads();
    const int m = blockIdx.x * 4 + (tid >> 6), lane = tid & 63;
    if (m >= a.M) return;
    const StreamItem it = a.items ? a.items[m] : a.item1;
    const int L = a.L, CW = a.CW, RR = a.RR;
    uint8_t* ring = a.ring + static_cast<int64_t>(it.id) * RR * CW;
    const uint8_t* cwin = a.cw_in + static_cast<int64_t>(m) * CW;
    if (!it.erased) {  // FEC_Decoder.cpp:55-59: the decoder keeps its own copy
        uint8_t* dst = ring + (it.seq % RR) * CW;
        if (!a.items && (reinterpret_cast<uintptr_t>(cwin) & 3) == 0) {
            // single packet from a host-visible row padded to whole dwords: dword loads, all in flight
            for (int w = lane; 4 * w < CW; w += 64) {
                const uint32_t v = reinterpret_cast<const uint32_t*>(cwin)[w];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * w + e < CW) dst[4 * w + e] = static_cast<uint8_t>(v >> (8 * e));
            }
        } else {
            for (int b = lane; b < CW; b += 64) dst[b] = cwin[b];
        }
    }
    // symbol (s, q) of packet sp: this call's codeword straight from the input (the ring row it
    // was just written to is not read back), older ones from the ring
    auto sym = [&](int64_t sp, int o) -> uint8_t {
        return sp == it.seq ? cwin[o] : ring[(((sp % RR) + RR) % RR) * CW + o];  // sp < 0: a zero row
    };
    uint8_t* orow = a.out + static_cast<int64_t>(m) * L;
    if (it.fate == kNone || it.fate == kLost) {
        for (int b = lane; b < L; b += 64) orow[b] = 0;
        if (lane == 0) a.out_len[m] = 0;
    } else {
        stream_output(a, it, orow, m, lane, gexp, glog, sym);
    }
    if (a.done) {  // every lane's stores complete, then the completion word (one wave: M == 1)
        __threadfence_system();
        if (lane == 0) *reinterpret_cast<volatile uint32_t*>(a.done) = a.ticket;
    }
}

// ---- bursts: counts[m] consecutive packets of each stream per call ---------------------------
// A burst is cut into chunks of at most TP packets, one workgroup each.  A chunk takes the packets
// in front of it that it needs (the encoder's n-1 windows, the decoder's T+k-1 codewords) from the
// call's own rows; only a burst's first chunk has packets from before the call in front of it, and
// reads them from the stream's ring.  The same workgroup, after a barrier, writes the ring with the
// burst's last packets (from the call's rows): no other workgroup of the launch touches that
// stream's ring, which takes TP >= n-1 (T+k-1) whenever a burst has more than one chunk.
//
// Each direction has one chunk body (burst_encode_chunk, burst_decode_chunk) and two kernels that
// differ only in where the chunk's geometry comes from: a one-code group's kernel has it in its
// arguments, sized to the call's largest burst; a mixed group's kernel takes it from a per-code table
// in device memory, sized at create.  A chunk's unit names its code, and since the code is the same
// for the whole workgroup (read through readfirstlane) the table entry arrives by scalar loads, once,
// before the kernel's first store.
// A group's rows and slots have one stride for all its codes: codeword rows of the largest CW (a
// stream's codeword is the first CW bytes of its row, its own code's CW; encode zeroes the rest,
// decode never reads it), a window slot of `slot` bytes and a ring slot of kRR rows per stream, in
// which a stream uses its own W, SK and CW.  In a one-code group the stride is CW.
// A stream that changes code (fec_streams_set_code) starts again at seq 0 in the same slots with
// nothing cleared: a body reads a window / ring row only for a packet seq >= 0 of the stream's
// current life (the `u.seq0 + p >= 0` tests), and every such window row was written in this life; a
// ring row of a missing packet keeps older bytes, which meet only zero coefficients.


struct BurstEncGeom {      // a chunk's geometry (burst_enc_lds) and its code's constants
    const uint32_t* ptab;  // [k][n-k][8] gf_mul4x tables
    int L, k, n, S, SP, NS4, CW, SK, SKS, W, TP, ROWS;
    int off_planes, off_io, off_ring, off_len;  // dynamic LDS carve-up (bytes, multiples of 16)
    FastDiv dk, dns4, dnq;
};
struct BurstDecGeom {  // burst_dec_lds
    const uint8_t* gf;
    int L, k, n, CW, CWS, CWD, LW, T, TP, HR, ROWS;
    int off_rows, off_out, off_coef, off_meta;  // dynamic LDS carve-up
    FastDiv dk, dlw, dcwd;
};

struct BurstEncRows {        // an encode call's row arrays (R rows)
    const uint8_t* payload;  // rows of L bytes
    const int32_t* len;      // payload sizes (null: all L)
    uint8_t* cw;             // rows of the group's codeword stride
    int32_t* cw_len;
};
struct BurstDecRows {        // a decode call's row arrays (R rows)
    const uint8_t* cw_in;    // rows of the group's codeword stride (rows of erased packets are not read)
    const uint8_t* flags;    // a byte each: fate | kRowClamp | kRowErased
    const uint8_t* coefs;    // the recovered rows' k x n blocks
    uint8_t* out;            // rows of L bytes
    int32_t* out_len;
};

struct BurstEncArgs {  // one-code group: the geometry in the arguments
    BurstEncRows rows;
    const BurstUnit* units;
    uint8_t* win;      // [streams][W][SK] window ring
    BurstEncGeom g;
};
struct BurstDecArgs {
    BurstDecRows rows;
    const BurstUnit* units;
    uint8_t* ring;     // [streams][kRR][CW]
    BurstDecGeom g;
};

struct MixedEncCode {  // table entry of one code
    BurstEncGeom g;    // at the code's chunk size
    int64_t slot;      // bytes of a stream's window slot
    int cwr;           // the group's codeword row stride
    int pad;
};
struct MixedDecCode {
    BurstDecGeom g;
    int cwr;
    int pad;
};
struct MixedEncArgs {  // mixed group: the geometry from codes[unit.code]
    BurstEncRows rows;
    const BurstUnit* units;
    uint8_t* win;      // [streams][slot]
    const MixedEncCode* codes;
};
struct MixedDecArgs {
    BurstDecRows rows;
    const BurstUnit* units;
    uint8_t* ring;     // [streams][kRR][cwr]
    const MixedDecCode* codes;
};

// One workgroup's chunk u of an encode call.  slot: the stream's windows ([W][SK]); CWR: the codeword
// row stride (a one-code kernel passes g.CW itself, and the zero fill below folds away).
// LDS: the parity tables; the windows of the chunk's packets and of the n-1 in front of them as
// position planes [i][row][sub-stream] (the four sub-streams of one gf_mul4x sit in one dword); the
// chunk's payload rows, later its codewords; the ring's rows.
__device__ __forceinline__ void burst_encode_chunk(const BurstEncGeom& g, const BurstUnit& u, const BurstEncRows& a,
                                                   uint8_t* slot, int CWR) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int L = g.L, k = g.k, n = g.n, S = g.S, SP = g.SP, NS4 = g.NS4, CW = g.CW, SK = g.SK, SKS = g.SKS;
    const int W = g.W, ROWS = g.ROWS, np = n - k, H = n - 1;
    uint32_t* tab = reinterpret_cast<uint32_t*>(smem);
    uint8_t* planes = smem + g.off_planes;
    int* lens = reinterpret_cast<int*>(smem + g.off_len);  // per row: payload size; -1 no packet; -2 ring row
    // the tables are device memory: said here, because a pointer read from the mixed kernels' table is
    // generic to the compiler, which then loads through it with flat instructions and leaves this loop rolled
    const auto* ptab = (const __attribute__((address_space(1))) uint32_t*)g.ptab;
    for (int i = tid; i < k * np * 8; i += 256) tab[i] = ptab[i];
    const int hb = min(H, u.lead);  // rows in front of the chunk that lie in the burst
    // row r = packet seq0 + r - H; a ring row only for a packet of the stream's current life (seq >= 0)
    for (int r = tid; r < ROWS; r += 256) {
        const int p = r - H;
        int v = -1;
        if (p < u.cnt) {
            if (p >= -hb)
                v = a.len ? min(max(a.len[u.row0 + p], 0), L) : L;
            else if (u.seq0 + p >= 0)
                v = -2;
        }
        lens[r] = v;
    }
    const uint8_t* g0 = a.payload + (u.row0 - hb) * L;
    burst_stage(smem, g.off_io, g0, (hb + u.cnt) * L, tid, 256);
    for (int r = 0; r < H - hb; ++r) {  // ring rows (first chunk only)
        const int64_t seq = u.seq0 + r - H;
        if (seq >= 0) burst_stage(smem, g.off_ring + r * SKS, slot + (seq % W) * SK, SK, tid, 256);
    }
    __syncthreads();
    // payload byte b of row r at smem[rawoff + r * L + b]
    const int rawoff = g.off_io + static_cast<int>(reinterpret_cast<uintptr_t>(g0) & 3) - (H - hb) * L;
    const int nq = (SK + 3) >> 2;
    const FastDiv dnq = g.dnq;
    auto lds_word = [&](int off) -> uint32_t {  // the dword at any LDS byte offset: two aligned reads
        const uint32_t* w = reinterpret_cast<const uint32_t*>(smem + (off & ~3));
        return __builtin_amdgcn_alignbyte(w[1], w[0], off & 3);
    };
    for (int idx = tid; idx < ROWS * nq; idx += 256) {  // window bytes 4q .. 4q+3 of row r
        const int r = fdiv(dnq, idx), q = idx - r * nq;
        const int ln = lens[r];
        uint32_t w = 0;  // [len_hi, len_lo, payload, zero pad] (Encoder.cpp:75-83)
        if (ln >= 0) {
            w = lds_word(rawoff + r * L + 4 * q - 2) & keep_bytes(ln + 2 - 4 * q);
            if (q == 0) w = (w & 0xffff0000u) | static_cast<uint32_t>(ln >> 8) | (static_cast<uint32_t>(ln & 0xff) << 8);
        } else if (ln == -2) {
            const uint8_t* gr = slot + ((u.seq0 + r - H) % W) * SK;
            w = lds_word(g.off_ring + r * SKS + static_cast<int>(reinterpret_cast<uintptr_t>(gr) & 3) + 4 * q);
        }
        int s = fdiv(g.dk, 4 * q), i = 4 * q - s * k;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * q + e < SK) planes[(i * ROWS + r) * SP + s] = static_cast<uint8_t>(w >> (8 * e));
            if (++i == k) i = 0, ++s;
        }
    }
    __syncthreads();  // the planes are complete; the payload rows give way to the codewords
    uint8_t* gcw = a.cw + u.row0 * CWR;
    const int ao = g.off_io + static_cast<int>(reinterpret_cast<uintptr_t>(gcw) & 3);
    uint8_t* out = smem + ao;  // the chunk's codewords, packed at CW
    for (int idx = tid; idx < u.cnt * nq; idx += 256) {  // systematic bytes
        const int p = fdiv(dnq, idx), q = idx - p * nq;
        int s = fdiv(g.dk, 4 * q), i = 4 * q - s * k;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (4 * q + e < SK) out[p * CW + s * n + i] = planes[(i * ROWS + p + H) * SP + s];
            if (++i == k) i = 0, ++s;
        }
    }
    // parity column j of four sub-streams: XOR_i G[i][j] * X_{t-(j-i)}[s][i]; rows without a packet are zero
    for (int jj = 0; jj < np; ++jj) {
        const int j = k + jj;
        for (int it = tid; it < u.cnt * NS4; it += 256) {
            const int p = fdiv(g.dns4, it), gq = it - p * NS4;
            uint32_t acc = 0;
            for (int i = 0; i < k; ++i) {
                const uint32_t* t = tab + (i * np + jj) * 8;
                if (!t[5]) continue;
                const int r = p + H - (j - i);
                acc ^= gf_mul4x(t, *reinterpret_cast<const uint32_t*>(planes + (i * ROWS + r) * SP + 4 * gq));
            }
            uint8_t* o = out + p * CW + 4 * gq * n + j;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * gq + e < S) o[e * n] = static_cast<uint8_t>(acc >> (8 * e));
        }
    }
    __syncthreads();
    if (tid < u.cnt) a.cw_len[u.row0 + tid] = last_nonzero_end(out + tid * CW, CW);  // FEC_Encoder.cpp:55-60
    if (CWR == CW) {
        burst_flush(gcw, smem, ao, u.cnt * CW, tid, 256);
    } else {  // a wave per row: the codeword, then zeros up to the group's stride
        for (int p = tid >> 6; p < u.cnt; p += 4) {
            burst_flush(gcw + p * CWR, smem, ao + p * CW, CW, tid & 63, 64);
            burst_zero(gcw + p * CWR + CW, CWR - CW, tid & 63, 64);
        }
    }
    if (u.lead != 0) return;
    // the burst's last min(total, W) windows into the stream's slot
    const int m = min(u.total, W), t0 = u.total - m;
    const bool far = u.total > u.cnt;  // they lie (partly) behind this chunk: their payload rows again
    const uint8_t* g1 = a.payload + (u.row0 + t0) * L;
    const int raw1 = g.off_io + static_cast<int>(reinterpret_cast<uintptr_t>(g1) & 3);
    if (far) {
        __syncthreads();
        burst_stage(smem, g.off_io, g1, m * L, tid, 256);
        __syncthreads();
    }
    for (int idx = tid; idx < m * nq; idx += 256) {
        const int tt = fdiv(dnq, idx), q = idx - tt * nq, t = t0 + tt;
        const int ln = far ? (a.len ? min(max(a.len[u.row0 + t], 0), L) : L) : 0;
        uint8_t v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int b = min(4 * q + e, SK - 1);
            if (far) {
                v[e] = b == 0 ? static_cast<uint8_t>(ln >> 8)
                              : b == 1 ? static_cast<uint8_t>(ln & 0xff) : (b - 2 < ln ? smem[raw1 + tt * L + b - 2] : 0);
            } else {
                const int s = fdiv(g.dk, b), i = b - s * k;
                v[e] = planes[(i * ROWS + t + H) * SP + s];
            }
        }
        uint8_t* dst = slot + ((u.seq0 + t) % W) * SK + 4 * q;  // dword aligned whenever SK is a multiple of 4
        if ((SK & 3) == 0) {
            *reinterpret_cast<uint32_t*>(dst) = uint32_t(v[0]) | (uint32_t(v[1]) << 8) | (uint32_t(v[2]) << 16) |
                                                (uint32_t(v[3]) << 24);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e < SK) dst[e] = v[e];
        }
    }
}

// One workgroup's chunk u of a decode call.  ring: the stream's kRR ring rows; CWR: the row stride of
// the ring and of the call's codeword rows.
// LDS: the GF tables; the codewords of the chunk's packets and of the T+k-1 in front of them (each
// row at its own dword phase); the recovered rows' coefficient blocks; the chunk's output rows.
__device__ __forceinline__ void burst_decode_chunk(const BurstDecGeom& g, const BurstUnit& u, const BurstDecRows& a,
                                                   uint8_t* ring, int CWR) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int L = g.L, k = g.k, n = g.n, CW = g.CW, CWS = g.CWS, CWD = g.CWD, LW = g.LW, T = g.T;
    const int HR = g.HR, ROWS = g.ROWS, TP = g.TP, kn = k * n;
    uint8_t* gexp = smem;
    uint8_t* glog = smem + 512;
    int* rowoff = reinterpret_cast<int*>(smem + g.off_meta);  // [ROWS] LDS offset of the row's byte 0; -1: none
    int* cord = rowoff + ROWS;                                // [TP] coefficient block of a recovered row
    int* lnS = cord + TP;                                     // [TP] output length
    int* cpS = lnS + TP;                                      // [TP] payload bytes copied
    uint8_t* fl = reinterpret_cast<uint8_t*>(cpS + TP);       // [TP] row flags
    for (int i = tid; i < 768; i += 256) smem[i] = g.gf[i];
    const int hb = min(HR, u.lead);
    // row r = packet seq0 + r - HR; its codeword's address (null: missing, or before the stream's
    // current life: a ring row is read only for seq >= 0)
    for (int r = tid; r < ROWS; r += 256) {
        const int p = r - HR;
        const uint8_t* gr = nullptr;
        if (p < u.cnt) {
            if (p >= -hb) {
                const uint8_t f = a.flags[u.row0 + p];
                if (p >= 0) fl[p] = f;
                if (!(f & kRowErased)) gr = a.cw_in + (u.row0 + p) * CWR;
            } else if (u.seq0 + p >= 0) {
                gr = ring + ((u.seq0 + p) % kRR) * CWR;
            }
        }
        rowoff[r] = gr ? g.off_rows + r * CWS + static_cast<int>(reinterpret_cast<uintptr_t>(gr) & 3) : -1;
    }
    __syncthreads();
    auto row_src = [&](int r) -> const uint8_t* {
        if (rowoff[r] < 0) return nullptr;
        const int p = r - HR;
        return p >= -hb ? a.cw_in + (u.row0 + p) * CWR : ring + ((u.seq0 + p) % kRR) * CWR;
    };
    if (tid < u.cnt) {
        int c = 0;
        for (int j = 0; j < tid; ++j) c += (fl[j] & 3) == kRecovered;
        cord[tid] = c;
    }
    int nrec = 0;
    for (int j = 0; j < u.cnt; ++j) nrec += (fl[j] & 3) == kRecovered;
    const uint8_t* gco = a.coefs + u.coef;
    if (nrec) burst_stage(smem, g.off_coef, gco, nrec * kn, tid, 256);
    const uint8_t* coefs = smem + g.off_coef + static_cast<int>(reinterpret_cast<uintptr_t>(gco) & 3);
    // dword w of row r (the row's first CW bytes from its dword phase on): batches of loads in flight
    auto stage_rows = [&](int nrows, auto src_of) {
        for (int base = 0; base < nrows * CWD; base += 256 * 4) {
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = base + q * 256 + tid;
                v[q] = 0;
                if (idx >= nrows * CWD) continue;
                const int r = fdiv(g.dcwd, idx), w = idx - r * CWD;
                const uint8_t* gr = src_of(r);
                if (!gr) continue;
                const int ph = static_cast<int>(reinterpret_cast<uintptr_t>(gr) & 3);
                const int lo = 4 * w - ph;  // the dword's first byte in the row
                if (lo >= CW) continue;
                if (lo >= 0 && lo + 4 <= CW) {
                    v[q] = *reinterpret_cast<const uint32_t*>(gr + lo);
                } else {
                    for (int e = 0; e < 4; ++e)
                        if (lo + e >= 0 && lo + e < CW) v[q] |= uint32_t(gr[lo + e]) << (8 * e);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int idx = base + q * 256 + tid;
                if (idx >= nrows * CWD) continue;
                const int r = fdiv(g.dcwd, idx), w = idx - r * CWD;
                *reinterpret_cast<uint32_t*>(smem + g.off_rows + r * CWS + 4 * w) = v[q];
            }
        }
    };
    stage_rows(HR + u.cnt, row_src);
    __syncthreads();
    // window byte h of output row j (packet x = seq0 + j - T = row j + k - 1)
    auto byte_at = [&](int j, int h) -> uint8_t {
        const int s = fdiv(g.dk, h), i = h - s * k;
        if ((fl[j] & 3) == kCopy) {
            const int ro = rowoff[j + k - 1];
            return ro < 0 ? 0 : smem[ro + s * n + i];
        }
        const uint8_t* coef = coefs + cord[j] * kn + i * n;
        uint8_t acc = 0;
        for (int q = 0; q < n; ++q) {  // symbol q of packet x - i + q
            const uint8_t c = coef[q];
            const int r = j + k - 1 - i + q;
            if (!c || r > j + HR) continue;
            const int ro = rowoff[r];
            if (ro >= 0) acc ^= gmul(gexp, glog, c, smem[ro + s * n + q]);
        }
        return acc;
    };
    if (tid < u.cnt) {  // header bytes first: they bound the copy
        const int fate = fl[tid] & 3;
        int ln = 0;
        if (fate == kCopy || fate == kRecovered) {
            const int hdr = byte_at(tid, 0) * 256 + byte_at(tid, 1);
            ln = (fl[tid] & kRowClamp) ? min(hdr, L) : hdr;
        }
        lnS[tid] = ln;
        cpS[tid] = min(ln, L);
        a.out_len[u.row0 + tid] = ln;
    }
    __syncthreads();
    uint8_t* gout = a.out + u.row0 * L;
    const int ao = g.off_out + static_cast<int>(reinterpret_cast<uintptr_t>(gout) & 3);
    for (int it = tid; it < u.cnt * LW; it += 256) {
        const int j = fdiv(g.dlw, it), w = it - j * LW;
        const int cp = cpS[j];
        uint8_t* o = smem + ao + j * L + 4 * w;
        if ((fl[j] & 3) == kCopy) {  // systematic bytes of the packet's own codeword
            const int ro = rowoff[j + k - 1];
            int s = fdiv(g.dk, 4 * w + 2), i = 4 * w + 2 - s * k;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = 4 * w + e;
                if (b < L) o[e] = (b < cp && ro >= 0) ? smem[ro + s * n + i] : 0;
                if (++i == k) i = 0, ++s;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = 4 * w + e;
                if (b < L) o[e] = b < cp ? byte_at(j, b + 2) : 0;
            }
        }
    }
    __syncthreads();
    burst_flush(gout, smem, ao, u.cnt * L, tid, 256);
    if (u.lead != 0) return;
    // the burst's last min(total, T + k) codewords into the ring (missing ones leave their slot as it is)
    const int m = min(u.total, T + k), t0 = u.total - m;
    int slot0 = HR + t0;  // LDS row of burst row t0
    if (u.total > u.cnt) {  // they lie (partly) behind this chunk: staged again, rows 0 .. m-1
        slot0 = 0;
        for (int r = tid; r < m; r += 256) {
            const uint8_t* gr = a.cw_in + (u.row0 + t0 + r) * CWR;
            rowoff[r] = (a.flags[u.row0 + t0 + r] & kRowErased)
                            ? -1 : g.off_rows + r * CWS + static_cast<int>(reinterpret_cast<uintptr_t>(gr) & 3);
        }
        __syncthreads();
        auto tail_src = [&](int r) -> const uint8_t* {
            return rowoff[r] < 0 ? nullptr : a.cw_in + (u.row0 + t0 + r) * CWR;
        };
        stage_rows(m, tail_src);
        __syncthreads();
    }
    for (int tt = tid >> 6; tt < m; tt += 4) {
        const int ro = rowoff[slot0 + tt];
        if (ro >= 0) burst_flush(ring + ((u.seq0 + t0 + tt) % kRR) * CWR, smem, ro, CW, tid & 63, 64);
    }
}

__global__ __launch_bounds__(256) void fec_streams_encode_burst_kernel(BurstEncArgs a) {
    const BurstUnit u = a.units[blockIdx.x];
    burst_encode_chunk(a.g, u, a.rows, a.win + static_cast<int64_t>(u.id) * a.g.W * a.g.SK, a.g.CW);
}

__global__ __launch_bounds__(256) void fec_streams_decode_burst_kernel(BurstDecArgs a) {
    const BurstUnit u = a.units[blockIdx.x];
    burst_decode_chunk(a.g, u, a.rows, a.ring + static_cast<int64_t>(u.id) * kRR * a.g.CW, a.g.CW);
}

__global__ __launch_bounds__(256) void fec_streams_encode_mixed_kernel(MixedEncArgs a) {
    const BurstUnit u = a.units[blockIdx.x];
    const MixedEncCode c = a.codes[__builtin_amdgcn_readfirstlane(u.code)];
    burst_encode_chunk(c.g, u, a.rows, a.win + static_cast<int64_t>(u.id) * c.slot, c.cwr);
}

__global__ __launch_bounds__(256) void fec_streams_decode_mixed_kernel(MixedDecArgs a) {
    const BurstUnit u = a.units[blockIdx.x];
    const MixedDecCode c = a.codes[__builtin_amdgcn_readfirstlane(u.code)];
    burst_decode_chunk(c.g, u, a.rows, a.ring + static_cast<int64_t>(u.id) * kRR * c.cwr, c.cwr);
}

}  // namespace
}  // namespace fec

struct fec_streams {
    std::unique_ptr<StepPool> pool;          // symbolic steps of large calls (FEC_STREAMS_THREADS)
    fec_codec* codec = nullptr;
    fec::Geometry g;
    int nstreams = 0, W = 1, SK = 0;
    std::shared_ptr<const fec::DecodeRules> rules;
    std::vector<std::unique_ptr<fec::StreamPlanner>> planners;
    std::vector<int64_t> enc_seq, dec_seq;   // packets sent / received so far per stream
    uint8_t* d_win = nullptr;                // encoder windows
    uint8_t* d_ring = nullptr;               // decoder rings
    // Per-call records (ids + seqs / items + coefs / chunks + flags + coefs).  The kernels read them
    // straight from the pinned buffers: an upload per call put an SDMA copy and its hand-off to the
    // kernel on the GPU's path, twice per encode + decode pair.
    fec::GroupStage stage;
    // Mixed groups (fec_streams_create_mixed; empty otherwise, and then codec / g / W / SK / rules above
    // are unused): the codes, each stream's code, the uniform row and slot strides, and the kernels'
    // per-code tables.  A code's chunk sizes are fixed at create (for bursts of kChunkTP or more).
    struct Code {
        fec_codec* codec = nullptr;
        fec::Geometry g;
        std::shared_ptr<const fec::DecodeRules> rules;
        int enc_tp = 0, enc_lds = 0, dec_tp = 0, dec_lds = 0;
    };
    std::vector<Code> codes;
    std::vector<int32_t> code_of;
    int cw_stride = 0;                       // the largest CW
    size_t win_slot = 0;                     // the largest W * SK, rounded up to 16
    fec::MixedEncCode* d_enc_codes = nullptr;
    fec::MixedDecCode* d_dec_codes = nullptr;
    ~fec_streams() {
        for (Code& c : codes)
            if (c.codec) fec_codec_destroy(c.codec);
        for (void* p : {static_cast<void*>(d_enc_codes), static_cast<void*>(d_dec_codes)})
            if (p) (void)hipFree(p);
        for (void* p : {static_cast<void*>(d_win), static_cast<void*>(d_ring)})
            if (p) (void)hipFree(p);
        if (codec) fec_codec_destroy(codec);
    }
};

namespace {

using fec::align16;
using fec::check_counts;

// LDS carve-up of burst_encode_chunk for chunks of tp packets: fills the geometry but ptab; returns its bytes
int burst_enc_lds(const fec::Geometry& g, int tp, fec::BurstEncGeom* a) {
    const int np = g.n - g.k, H = g.n - 1, SK = g.S * g.k;
    a->L = g.L, a->k = g.k, a->n = g.n, a->S = g.S, a->CW = g.CW, a->SK = SK;
    a->NS4 = (g.S + 3) / 4;
    a->SP = 4 * a->NS4;
    a->SKS = (SK + 7) & ~3;
    a->W = std::max(1, H);
    a->TP = tp;
    a->ROWS = tp + H;
    size_t off = align16(static_cast<size_t>(std::max(1, g.k * np)) * 32);
    a->off_planes = static_cast<int>(off);
    off = align16(off + static_cast<size_t>(g.k) * a->ROWS * a->SP);
    a->off_io = static_cast<int>(off);
    off = align16(off + std::max(static_cast<size_t>(a->ROWS) * g.L, static_cast<size_t>(tp) * g.CW) + 32);
    a->off_ring = static_cast<int>(off);
    off = align16(off + static_cast<size_t>(H) * a->SKS);
    a->off_len = static_cast<int>(off);
    off = align16(off + static_cast<size_t>(a->ROWS) * 4);
    a->dk = fec::fast_div(g.k);
    a->dns4 = fec::fast_div(a->NS4);
    a->dnq = fec::fast_div((SK + 3) >> 2);
    return static_cast<int>(std::min<size_t>(off, 1u << 30));
}

int burst_dec_lds(const fec::Geometry& g, int tp, fec::BurstDecGeom* a) {
    a->L = g.L, a->k = g.k, a->n = g.n, a->CW = g.CW, a->T = g.T;
    a->CWD = (g.CW + 6) >> 2;
    a->CWS = 4 * a->CWD;
    a->LW = (g.L + 3) >> 2;
    a->TP = tp;
    a->HR = g.T + g.k - 1;
    a->ROWS = a->HR + tp;
    size_t off = 768;
    a->off_rows = static_cast<int>(off);
    off = align16(off + static_cast<size_t>(a->ROWS) * a->CWS);
    a->off_coef = static_cast<int>(off);
    off = align16(off + static_cast<size_t>(tp) * g.k * g.n + 16);
    a->off_out = static_cast<int>(off);
    off = align16(off + static_cast<size_t>(tp) * g.L + 32);
    a->off_meta = static_cast<int>(off);
    off = align16(off + static_cast<size_t>(a->ROWS) * 4 + static_cast<size_t>(tp) * 13);
    a->dk = fec::fast_div(g.k);
    a->dlw = fec::fast_div(a->LW);
    a->dcwd = fec::fast_div(a->CWD);
    return static_cast<int>(std::min<size_t>(off, 1u << 30));
}

// Packets per chunk for a call whose longest burst has maxc packets: at most kChunkTP (or maxc), at
// least `front` (the packets a chunk needs in front of it, so that only a burst's first chunk reads
// the ring), and within kCuLds.  0: this geometry does not fit.
template <class Geom, class F>
int burst_chunk(const fec::Geometry& g, int maxc, int front, F lds_of, Geom* a, int* lds) {
    if (g.S * g.k > 16384 || g.CW > 16384) return 0;
    const int lo = std::max(1, front);
    for (int tp = std::max(lo, std::min(maxc, fec::kChunkTP)); tp >= lo; --tp) {
        *lds = lds_of(g, tp, a);
        if (*lds <= fec::kCuLds) return tp;
    }
    return 0;
}

// The chunks of one burst of `count` rows, cut every tp rows; returns the unit after them.
fec::BurstUnit* burst_fill_units(fec::BurstUnit* u, int id, int code, int count, int64_t row, int tp, int64_t seq) {
    for (int lead = 0; lead < count; lead += tp, ++u) {
        u->row0 = row + lead;
        u->seq0 = seq + lead;
        u->coef = 0;
        u->id = id;
        u->cnt = std::min(tp, count - lead);
        u->lead = lead;
        u->total = count;
        u->code = code;
        u->pad = 0;
    }
    return u;
}

// What every group has besides its codes and planners (h->nstreams set): the step pool, the seq
// counters, zeroed windows (wb bytes) and rings (rb bytes), the staging buffers and the events.
int group_state_init(fec_streams* h, size_t wb, size_t rb, size_t stage_bytes) {
    const int nstreams = h->nstreams;
    h->pool = make_step_pool(nstreams);
    h->enc_seq.assign(nstreams, 0);
    h->dec_seq.assign(nstreams, 0);
    FEC_HIP(hipMalloc(&h->d_win, wb));
    FEC_HIP(hipMemset(h->d_win, 0, wb));
    FEC_HIP(hipMalloc(&h->d_ring, rb));
    FEC_HIP(hipMemset(h->d_ring, 0, rb));
    return h->stage.init(nstreams, stage_bytes);
}

// ---- mixed groups ------------------------------------------------------------------------------

constexpr int kMaxCodes = 64;

// One code of a mixed group at payload size L: its geometry and its burst chunks, fixed for bursts of
// kChunkTP or more, through the routines the one-code calls use.  FEC_ERR_ARG: a tuple that
// fec_streams_create refuses (fec_codec_create's bounds, then the stream kernels'), or whose smallest
// chunk does not fit the LDS.
struct CodeFit {
    fec::Geometry g;
    int enc_tp = 0, enc_lds = 0, dec_tp = 0, dec_lds = 0;
    fec::BurstEncGeom enc;
    fec::BurstDecGeom dec;
};
int mixed_code_fit(int L, const int32_t* tbn, CodeFit* f) {
    if (!fec::stream_tuple(L, tbn[0], tbn[1], tbn[2], &f->g)) return FEC_ERR_ARG;
    const fec::Geometry& g = f->g;
    f->enc = fec::BurstEncGeom{};
    f->dec = fec::BurstDecGeom{};
    f->enc_tp = burst_chunk(g, fec::kChunkTP, g.n - 1, burst_enc_lds, &f->enc, &f->enc_lds);
    f->dec_tp = burst_chunk(g, fec::kChunkTP, g.T + g.k - 1, burst_dec_lds, &f->dec, &f->dec_lds);
    return f->enc_tp && f->dec_tp ? FEC_OK : FEC_ERR_ARG;
}

// ---- chunk calls: bursts of any group, and a mixed group's one-packet calls ----------------------

// What the chunks of one stream follow in a call: its code's index in the mixed kernels' table, the
// chunk size and LDS of this direction, T and k x n.
struct ChunkCode {
    int code, tp, lds, T, kn;
};
// A one-code group: `one` for every stream, its chunk cut for the call's largest burst (burst_chunk).
// A mixed group: the stream's own code, its chunk fixed at create.
inline ChunkCode chunk_code(const fec_streams* h, bool enc, const ChunkCode& one, int id) {
    if (h->codes.empty()) return one;
    const int code = h->code_of[id];
    const fec_streams::Code& c = h->codes[code];
    return ChunkCode{code, enc ? c.enc_tp : c.dec_tp, enc ? c.enc_lds : c.dec_lds, c.g.T, c.g.k * c.g.n};
}
// The call's chunks (counts null: one packet per stream), and the largest chunk LDS among its streams' codes.
int64_t chunk_count(const fec_streams* h, bool enc, const ChunkCode& one, const int32_t* ids, const int32_t* counts,
                    int M, int* lds) {
    int64_t nu = 0;
    *lds = 0;
    for (int m = 0; m < M; ++m) {
        const ChunkCode c = chunk_code(h, enc, one, ids[m]);
        nu += ((counts ? counts[m] : 1) + c.tp - 1) / c.tp;
        *lds = std::max(*lds, c.lds);
    }
    return nu;
}

// The encode half of a chunk call; counts (null: all 1) are checked, the largest is maxc.
int encode_chunks(fec_streams* h, const int32_t* ids, const int32_t* counts, int M, int maxc, const uint8_t* d_payload,
                  const int32_t* d_payload_len, uint8_t* d_codeword, int32_t* d_codeword_len, hipStream_t s) {
    fec::GroupStage& stage = h->stage;
    if (int st = stage.check_ids(ids, M)) return st;
    const bool mixed = !h->codes.empty();
    fec::BurstEncArgs a1;  // a one-code group's arguments: its geometry
    ChunkCode one{};
    if (!mixed) {
        one = ChunkCode{0, 0, 0, h->g.T, h->g.k * h->g.n};
        one.tp = burst_chunk(h->g, maxc, h->g.n - 1, burst_enc_lds, &a1.g, &one.lds);
        if (one.tp == 0) return FEC_ERR_ARG;
    }
    int lds = 0;
    const int64_t nu = chunk_count(h, true, one, ids, counts, M, &lds);
    if (nu > INT32_MAX) return FEC_ERR_ARG;
    static int lds_raised[2] = {0, 0};  // per kernel
    const void* kernel = mixed ? reinterpret_cast<const void*>(fec::fec_streams_encode_mixed_kernel)
                               : reinterpret_cast<const void*>(fec::fec_streams_encode_burst_kernel);
    if (int st = fec::lds_allow(kernel, lds, &lds_raised[mixed])) return st;
    if (int st = stage.begin(s)) return st;
    fec::StageGuard guard{stage};
    if (int st = stage.reserve(static_cast<size_t>(nu) * sizeof(fec::BurstUnit))) return st;
    fec::BurstUnit* u = reinterpret_cast<fec::BurstUnit*>(stage.host());
    int64_t row = 0;
    for (int m = 0; m < M; ++m) {
        const int id = ids[m], cnt = counts ? counts[m] : 1;
        const ChunkCode c = chunk_code(h, true, one, id);
        u = burst_fill_units(u, id, c.code, cnt, row, c.tp, h->enc_seq[id]);
        row += cnt;
    }
    const fec::BurstEncRows rows{d_payload, d_payload_len, d_codeword, d_codeword_len};
    const fec::BurstUnit* du = reinterpret_cast<const fec::BurstUnit*>(stage.device());
    const dim3 grid(static_cast<unsigned>(nu));
    if (mixed) {
        const fec::MixedEncArgs a{rows, du, h->d_win, h->d_enc_codes};
        hipLaunchKernelGGL(fec::fec_streams_encode_mixed_kernel, grid, dim3(256), lds, s, a);
    } else {
        fec::CodecView v;
        fec::codec_view(h->codec, &v);
        a1.rows = rows, a1.units = du, a1.win = h->d_win, a1.g.ptab = v.ptab;
        hipLaunchKernelGGL(fec::fec_streams_encode_burst_kernel, grid, dim3(256), lds, s, a1);
    }
    if (int st = stage.commit(s)) return st;
    for (int m = 0; m < M; ++m) h->enc_seq[ids[m]] += counts ? counts[m] : 1;
    return FEC_OK;
}

// The decode half of a chunk call; counts (null: all 1) are checked, their sum is R and the largest maxc.
int decode_chunks(fec_streams* h, const int32_t* ids, const int32_t* counts, int M, int64_t R, int maxc,
                  const uint8_t* erasure, const uint8_t* d_codeword, uint8_t* d_payload_out, int32_t* d_payload_len,
                  hipStream_t s) {
    fec::GroupStage& stage = h->stage;
    if (int st = stage.check_ids(ids, M)) return st;
    const bool mixed = !h->codes.empty();
    fec::BurstDecArgs a1;  // a one-code group's arguments: its geometry
    ChunkCode one{};
    if (!mixed) {
        one = ChunkCode{0, 0, 0, h->g.T, h->g.k * h->g.n};
        one.tp = burst_chunk(h->g, maxc, h->g.T + h->g.k - 1, burst_dec_lds, &a1.g, &one.lds);
        if (one.tp == 0) return FEC_ERR_ARG;
    }
    int lds = 0;
    const int64_t nu = chunk_count(h, false, one, ids, counts, M, &lds);
    if (nu > INT32_MAX) return FEC_ERR_ARG;
    static int lds_raised[2] = {0, 0};  // per kernel
    const void* kernel = mixed ? reinterpret_cast<const void*>(fec::fec_streams_decode_mixed_kernel)
                               : reinterpret_cast<const void*>(fec::fec_streams_decode_burst_kernel);
    if (int st = fec::lds_allow(kernel, lds, &lds_raised[mixed])) return st;
    if (int st = stage.begin(s)) return st;
    fec::StageGuard guard{stage};  // the symbolic decoders advance before the launch
    try {
        DecodePlan<fec::BurstUnit> plan;
        const bool ok = plan.plan(
            h->pool.get(), counts, M, R, [&](int m) { return chunk_code(h, false, one, ids[m]).tp; },
            [&](int m, int64_t row0, int cnt, fec::BurstUnit* u, uint8_t* fl, std::vector<uint8_t>& coefs) {
                const int id = ids[m];
                const ChunkCode c = chunk_code(h, false, one, id);
                int64_t cbytes = static_cast<int64_t>(coefs.size());  // the part's coefficient bytes so far
                fec::BurstUnit* end = burst_fill_units(u, id, c.code, cnt, row0, c.tp, h->dec_seq[id]);
                plan_burst_rows(*h->planners[id], c.T, c.kn, h->dec_seq[id], erasure + row0, cnt, fl, coefs);
                h->dec_seq[id] += cnt;
                for (; u != end; ++u) {
                    u->coef = cbytes;
                    for (int j = 0; j < u->cnt; ++j)
                        if ((fl[u->lead + j] & 3) == fec::kRecovered) cbytes += c.kn;
                }
            },
            [](fec::BurstUnit& u, int64_t by) { u.coef += by; });
        if (!ok) return FEC_ERR_ARG;
        if (int st = stage.reserve(plan.bytes)) return st;
        plan.write(stage.host());
        const uint8_t* rec = stage.device();
        const fec::BurstDecRows rows{d_codeword, rec + plan.off_flags, rec + plan.off_coef, d_payload_out, d_payload_len};
        const fec::BurstUnit* du = reinterpret_cast<const fec::BurstUnit*>(rec);
        const dim3 grid(static_cast<unsigned>(nu));
        if (mixed) {
            const fec::MixedDecArgs a{rows, du, h->d_ring, h->d_dec_codes};
            hipLaunchKernelGGL(fec::fec_streams_decode_mixed_kernel, grid, dim3(256), lds, s, a);
        } else {
            fec::CodecView v;
            fec::codec_view(h->codec, &v);
            a1.rows = rows, a1.units = du, a1.ring = h->d_ring, a1.g.gf = v.gf;
            hipLaunchKernelGGL(fec::fec_streams_decode_burst_kernel, grid, dim3(256), lds, s, a1);
        }
        return stage.commit(s);
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

}  // namespace

int fec::stream_encode_one(const CodecView& v, uint8_t* win, const uint8_t* payload, int payload_len, int64_t seq,
                           uint8_t* cw, int32_t* cw_len, uint32_t* done, uint32_t ticket, hipStream_t s) {
    if (v.k > 16 || v.k * v.n > 16 * 32) return FEC_ERR_ARG;  // the kernel's register / LDS bounds
    fec::StreamsEncArgs a;
    a.payload = payload;
    a.len = nullptr;
    a.ids = nullptr;
    a.seq = nullptr;
    a.win = win;
    a.cw = cw;
    a.cw_len = cw_len;
    a.G = v.G;
    a.gf = v.gf;
    a.M = 1;
    a.L = v.L;
    a.k = v.k;
    a.n = v.n;
    a.S = v.S;
    a.CW = v.CW;
    a.SK = v.S * v.k;
    a.W = std::max(1, v.n - 1);
    a.seq1 = seq;
    a.len1 = payload_len;
    a.done = done;
    a.ticket = ticket;
    hipLaunchKernelGGL(fec::fec_streams_encode_kernel, dim3(1), dim3(256), 0, s, a);  // 256: the table loads
    FEC_HIP(hipGetLastError());
    return FEC_OK;
}

int fec::stream_decode_one(const CodecView& v, uint8_t* ring, const uint8_t* cw, int64_t seq, int erased,
                           int fate, int clamp, int64_t x, const uint8_t* coef, uint8_t* out, int32_t* out_len,
                           uint32_t* done, uint32_t ticket, hipStream_t s) {
    fec::StreamsDecArgs a;
    a.cw_in = cw;
    a.items = nullptr;
    a.coefs = coef;
    a.ring = ring;
    a.gf = v.gf;
    a.out = out;
    a.out_len = out_len;
    a.M = 1;
    a.L = v.L;
    a.k = v.k;
    a.n = v.n;
    a.CW = v.CW;
    a.RR = kRR;
    a.item1 = fec::StreamItem{0, fate, clamp, 0, seq, x, erased, 0};
    a.done = done;
    a.ticket = ticket;
    hipLaunchKernelGGL(fec::fec_streams_decode_kernel, dim3(1), dim3(256), 0, s, a);  // 256: the table loads
    FEC_HIP(hipGetLastError());
    return FEC_OK;
}

extern "C" {

int fec_streams_create(int max_payload, int T, int B, int N, int nstreams, fec_streams** out) {
    if (!out || nstreams <= 0) return FEC_ERR_ARG;
    *out = nullptr;
    try {
        std::unique_ptr<fec_streams> h(new fec_streams());
        if (!fec::stream_tuple(max_payload, T, B, N, &h->g)) return FEC_ERR_ARG;
        const fec::Geometry& g = h->g;
        if (int st = fec_codec_create(max_payload, T, B, N, &h->codec)) return st;
        h->nstreams = nstreams;
        h->W = std::max(1, g.n - 1);
        h->SK = g.S * g.k;
        h->rules = fec::shared_decode_rules(T, B, N);
        h->planners.resize(nstreams);
        for (auto& p : h->planners) p.reset(new fec::StreamPlanner(g, h->rules.get()));
        const size_t wb = static_cast<size_t>(nstreams) * h->W * h->SK;
        const size_t rb = static_cast<size_t>(nstreams) * fec::kRR * g.CW;
        const size_t stage = static_cast<size_t>(nstreams) * (sizeof(fec::StreamItem) + g.k * g.n + 16) + 64;
        if (int st = group_state_init(h.get(), wb, rb, stage)) return st;
        *out = h.release();
        return FEC_OK;
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

int fec_streams_destroy(fec_streams* h) {
    delete h;
    return FEC_OK;
}

int fec_streams_encode(fec_streams* h, const int32_t* ids, int M, const uint8_t* d_payload,
                       const int32_t* d_payload_len, uint8_t* d_codeword, int32_t* d_codeword_len,
                       void* stream) {
    if (!h || M < 0 || M > h->nstreams || (M > 0 && (!ids || !d_payload || !d_codeword || !d_codeword_len)))
        return FEC_ERR_ARG;
    if (M == 0) return FEC_OK;
    if (!h->codes.empty())  // a mixed group: chunks of one packet
        return encode_chunks(h, ids, nullptr, M, 1, d_payload, d_payload_len, d_codeword, d_codeword_len,
                             static_cast<hipStream_t>(stream));
    fec::GroupStage& stage = h->stage;
    if (int st = stage.check_ids(ids, M)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int st = stage.begin(s)) return st;
    fec::StageGuard guard{stage};
    int64_t* hseq = reinterpret_cast<int64_t*>(stage.host());  // M seqs, M ids: within the buffers' size at create
    int32_t* hid = reinterpret_cast<int32_t*>(hseq + M);
    for (int m = 0; m < M; ++m) {
        hseq[m] = h->enc_seq[ids[m]];  // committed below, once the launch is in
        hid[m] = ids[m];
    }
    const void* rec = stage.device();
    fec::CodecView v;
    fec::codec_view(h->codec, &v);
    fec::StreamsEncArgs a;
    a.payload = d_payload;
    a.len = d_payload_len;
    a.seq = static_cast<const int64_t*>(rec);
    a.ids = reinterpret_cast<const int32_t*>(static_cast<const int64_t*>(rec) + M);
    a.win = h->d_win;
    a.cw = d_codeword;
    a.cw_len = d_codeword_len;
    a.G = v.G;
    a.gf = v.gf;
    a.M = M;
    a.L = h->g.L;
    a.k = h->g.k;
    a.n = h->g.n;
    a.S = h->g.S;
    a.CW = h->g.CW;
    a.SK = h->SK;
    a.W = h->W;
    a.seq1 = 0;
    a.len1 = h->g.L;
    a.done = nullptr;
    a.ticket = 0;
    hipLaunchKernelGGL(fec::fec_streams_encode_kernel, dim3((M + 3) / 4), dim3(256), 0, s, a);
    if (int st = stage.commit(s)) return st;
    for (int m = 0; m < M; ++m) ++h->enc_seq[ids[m]];
    return FEC_OK;
}

int fec_streams_decode(fec_streams* h, const int32_t* ids, int M, const uint8_t* erasure,
                       const uint8_t* d_codeword, uint8_t* d_payload_out, int32_t* d_payload_len,
                       void* stream) {
    if (!h || M < 0 || M > h->nstreams || (M > 0 && (!ids || !erasure || !d_codeword || !d_payload_out ||
                                                     !d_payload_len)))
        return FEC_ERR_ARG;
    if (M == 0) return FEC_OK;
    if (!h->codes.empty())  // a mixed group: chunks of one packet
        return decode_chunks(h, ids, nullptr, M, M, 1, erasure, d_codeword, d_payload_out, d_payload_len,
                             static_cast<hipStream_t>(stream));
    fec::GroupStage& stage = h->stage;
    if (int st = stage.check_ids(ids, M)) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int st = stage.begin(s)) return st;
    fec::StageGuard guard{stage};  // the symbolic decoders advance below, before the launch
    const fec::Geometry& g = h->g;
    // M items and at most M coefficient blocks: within the buffers' size at create
    fec::StreamItem* items = reinterpret_cast<fec::StreamItem*>(stage.host());
    uint8_t* coefs = reinterpret_cast<uint8_t*>(items + M);
    const int kn = g.k * g.n;
    std::atomic<int> ncoef_a{0};
    std::atomic<bool> failed{false};
    // one symbolic decoder step per item; the recovered packets' coefficient rows take slots in
    // arrival order (an item carries its slot)
    auto steps = [&](int m0, int m1) {
        try {
            for (int m = m0; m < m1; ++m) {
                const int id = ids[m];
                const bool er = erasure[m] != 0;
                const int64_t seq = h->dec_seq[id]++;
                const fec::StepResult r = h->planners[id]->step(seq, er);
                fec::StreamItem& it = items[m];
                it.id = id;
                it.fate = r.fate;
                it.clamp = r.slow ? 1 : 0;
                it.coef = 0;
                it.seq = seq;
                it.x = r.x;
                it.erased = er ? 1 : 0;
                it.pad = 0;
                if (r.fate == fec::kRecovered) {
                    const int slot = ncoef_a.fetch_add(1, std::memory_order_relaxed);
                    std::memcpy(coefs + static_cast<size_t>(slot) * kn, r.coef, kn);
                    it.coef = slot;
                }
            }
        } catch (...) {
            failed.store(true);
        }
    };
    if (h->pool && M >= 2 * kPoolMinItems) {
        const int np = h->pool->parts();
        h->pool->run([&](int p) { steps(static_cast<int>(static_cast<int64_t>(M) * p / np),
                                        static_cast<int>(static_cast<int64_t>(M) * (p + 1) / np)); });
    } else {
        steps(0, M);
    }
    if (failed.load()) return FEC_ERR_ARG;
    const void* rec = stage.device();
    fec::CodecView v;
    fec::codec_view(h->codec, &v);
    fec::StreamsDecArgs a;
    a.cw_in = d_codeword;
    a.items = static_cast<const fec::StreamItem*>(rec);
    a.coefs = reinterpret_cast<const uint8_t*>(a.items + M);
    a.ring = h->d_ring;
    a.gf = v.gf;
    a.out = d_payload_out;
    a.out_len = d_payload_len;
    a.M = M;
    a.L = g.L;
    a.k = g.k;
    a.n = g.n;
    a.CW = g.CW;
    a.RR = fec::kRR;
    a.done = nullptr;
    a.ticket = 0;
    hipLaunchKernelGGL(fec::fec_streams_decode_kernel, dim3((M + 3) / 4), dim3(256), 0, s, a);
    return stage.commit(s);
}

int fec_streams_encode_burst(fec_streams* h, const int32_t* ids, const int32_t* counts, int M,
                             const uint8_t* d_payload, const int32_t* d_payload_len, uint8_t* d_codeword,
                             int32_t* d_codeword_len, void* stream) {
    if (!h || M < 0 || M > h->nstreams ||
        (M > 0 && (!ids || !counts || !d_payload || !d_codeword || !d_codeword_len)))
        return FEC_ERR_ARG;
    if (M == 0) return FEC_OK;
    int64_t R = 0;
    int maxc = 0;
    if (int st = check_counts(counts, M, &R, &maxc)) return st;
    if (h->codes.empty() && maxc == 1)  // one packet per stream of a one-code group: the one-packet kernel
        return fec_streams_encode(h, ids, M, d_payload, d_payload_len, d_codeword, d_codeword_len, stream);
    return encode_chunks(h, ids, counts, M, maxc, d_payload, d_payload_len, d_codeword, d_codeword_len,
                         static_cast<hipStream_t>(stream));
}

int fec_streams_decode_burst(fec_streams* h, const int32_t* ids, const int32_t* counts, int M,
                             const uint8_t* erasure, const uint8_t* d_codeword, uint8_t* d_payload_out,
                             int32_t* d_payload_len, void* stream) {
    if (!h || M < 0 || M > h->nstreams ||
        (M > 0 && (!ids || !counts || !erasure || !d_codeword || !d_payload_out || !d_payload_len)))
        return FEC_ERR_ARG;
    if (M == 0) return FEC_OK;
    int64_t R = 0;
    int maxc = 0;
    if (int st = check_counts(counts, M, &R, &maxc)) return st;
    if (h->codes.empty() && maxc == 1)  // one packet per stream of a one-code group: the one-packet kernel
        return fec_streams_decode(h, ids, M, erasure, d_codeword, d_payload_out, d_payload_len, stream);
    return decode_chunks(h, ids, counts, M, R, maxc, erasure, d_codeword, d_payload_out, d_payload_len,
                         static_cast<hipStream_t>(stream));
}

int fec_streams_plan_burst_host(int max_payload, int T, int B, int N, const uint8_t* erasure,
                                const int32_t* counts, int ncounts, uint8_t* fate) {
    if (!erasure || !fate || !counts || ncounts < 0) return FEC_ERR_ARG;
    try {
        const fec::Geometry g = fec::Geometry::make(max_payload, T, B, N);
        if (g.B < g.N || g.n > fec::kMaxN - 1) return FEC_ERR_ARG;  // fec_plan_host's bounds
        int64_t P = 0;
        int maxc = 0;
        if (int st = check_counts(counts, ncounts, &P, &maxc)) return st;
        const auto rules = fec::shared_decode_rules(T, B, N);
        fec::StreamPlanner pl(g, rules.get());
        std::vector<uint8_t> flags(static_cast<size_t>(P)), coefs;
        int64_t seq = 0;
        for (int c = 0; c < ncounts; ++c) {
            coefs.clear();
            plan_burst_rows(pl, g.T, g.k * g.n, seq, erasure + seq, counts[c], flags.data() + seq, coefs);
            seq += counts[c];
        }
        for (int64_t t = g.T; t < P; ++t) fate[t - g.T] = flags[t] & 3;
        return FEC_OK;
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

int fec_streams_state(const fec_streams* h, int id, int64_t* sent, int64_t* received) {
    if (!h || id < 0 || id >= h->nstreams) return FEC_ERR_ARG;
    if (sent) *sent = h->enc_seq[id];
    if (received) *received = h->dec_seq[id];
    return FEC_OK;
}

int fec_streams_mixed_fit(int max_payload, const int32_t* tuples, int ncodes, int32_t* enc_chunk, int32_t* enc_lds,
                          int32_t* dec_chunk, int32_t* dec_lds) {
    if (!tuples || ncodes < 1 || ncodes > kMaxCodes || !enc_chunk || !enc_lds || !dec_chunk || !dec_lds)
        return FEC_ERR_ARG;
    for (int c = 0; c < ncodes; ++c) {
        CodeFit f;
        if (int st = mixed_code_fit(max_payload, tuples + 3 * c, &f)) return st;
        enc_chunk[c] = f.enc_tp, enc_lds[c] = f.enc_lds, dec_chunk[c] = f.dec_tp, dec_lds[c] = f.dec_lds;
    }
    return FEC_OK;
}

int fec_streams_create_mixed(int max_payload, const int32_t* tuples, int ncodes, const int32_t* code_of, int nstreams,
                             fec_streams** out) {
    if (!out) return FEC_ERR_ARG;
    *out = nullptr;
    if (!tuples || !code_of || ncodes < 1 || ncodes > kMaxCodes || nstreams <= 0) return FEC_ERR_ARG;
    for (int i = 0; i < nstreams; ++i)
        if (code_of[i] < 0 || code_of[i] >= ncodes) return FEC_ERR_ARG;
    try {
        std::vector<CodeFit> fit(ncodes);
        for (int c = 0; c < ncodes; ++c)
            if (int st = mixed_code_fit(max_payload, tuples + 3 * c, &fit[c])) return st;
        std::unique_ptr<fec_streams> h(new fec_streams());
        h->nstreams = nstreams;
        h->codes.resize(ncodes);
        for (int c = 0; c < ncodes; ++c) {
            fec_streams::Code& code = h->codes[c];
            const int32_t* t = tuples + 3 * c;
            if (int st = fec_codec_create(max_payload, t[0], t[1], t[2], &code.codec)) return st;
            code.g = fit[c].g;
            code.rules = fec::shared_decode_rules(t[0], t[1], t[2]);
            code.enc_tp = fit[c].enc_tp, code.enc_lds = fit[c].enc_lds;
            code.dec_tp = fit[c].dec_tp, code.dec_lds = fit[c].dec_lds;
            h->cw_stride = std::max(h->cw_stride, code.g.CW);
            h->win_slot = std::max(h->win_slot, align16(static_cast<size_t>(fit[c].enc.W) * fit[c].enc.SK));
        }
        h->code_of.assign(code_of, code_of + nstreams);
        h->planners.resize(nstreams);
        for (int i = 0; i < nstreams; ++i) {
            const fec_streams::Code& code = h->codes[code_of[i]];
            h->planners[i].reset(new fec::StreamPlanner(code.g, code.rules.get()));
        }
        // the kernels' tables: a code's geometry at its chunk sizes, its constants, the group's strides
        std::vector<fec::MixedEncCode> et(ncodes);
        std::vector<fec::MixedDecCode> dt(ncodes);
        size_t kn_max = 0;
        for (int c = 0; c < ncodes; ++c) {
            fec::CodecView v;
            if (int st = fec::codec_view(h->codes[c].codec, &v)) return st;
            et[c].g = fit[c].enc;
            et[c].g.ptab = v.ptab;
            et[c].slot = static_cast<int64_t>(h->win_slot);
            et[c].cwr = h->cw_stride;
            et[c].pad = 0;
            dt[c].g = fit[c].dec;
            dt[c].g.gf = v.gf;
            dt[c].cwr = h->cw_stride;
            dt[c].pad = 0;
            kn_max = std::max(kn_max, static_cast<size_t>(v.k) * v.n);
        }
        FEC_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_enc_codes), et.size() * sizeof(et[0])));
        FEC_HIP(hipMemcpy(h->d_enc_codes, et.data(), et.size() * sizeof(et[0]), hipMemcpyHostToDevice));
        FEC_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_dec_codes), dt.size() * sizeof(dt[0])));
        FEC_HIP(hipMemcpy(h->d_dec_codes, dt.data(), dt.size() * sizeof(dt[0]), hipMemcpyHostToDevice));
        const size_t wb = static_cast<size_t>(nstreams) * h->win_slot;
        const size_t rb = static_cast<size_t>(nstreams) * fec::kRR * h->cw_stride;
        const size_t stage = static_cast<size_t>(nstreams) * (sizeof(fec::BurstUnit) + 1 + kn_max + 16) + 64;
        if (int st = group_state_init(h.get(), wb, rb, stage)) return st;
        *out = h.release();
        return FEC_OK;
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

int fec_streams_codes(const fec_streams* h, int* ncodes, int* cw_stride) {
    if (!h) return FEC_ERR_ARG;
    if (ncodes) *ncodes = h->codes.empty() ? 1 : static_cast<int>(h->codes.size());
    if (cw_stride) *cw_stride = h->codes.empty() ? h->g.CW : h->cw_stride;
    return FEC_OK;
}

int fec_streams_stream_geometry(const fec_streams* h, int id, int* code, int* T, int* k, int* n, int* S, int* CW) {
    if (!h || id < 0 || id >= h->nstreams) return FEC_ERR_ARG;
    const int c = h->codes.empty() ? 0 : h->code_of[id];
    const fec::Geometry& g = h->codes.empty() ? h->g : h->codes[c].g;
    if (code) *code = c;
    if (T) *T = g.T;
    if (k) *k = g.k;
    if (n) *n = g.n;
    if (S) *S = g.S;
    if (CW) *CW = g.CW;
    return FEC_OK;
}

int fec_streams_set_code(fec_streams* h, int id, int code) {
    if (!h || id < 0 || id >= h->nstreams || code < 0 || code >= (h->codes.empty() ? 1 : static_cast<int>(h->codes.size())))
        return FEC_ERR_ARG;
    try {
        // host work only: the kernels read a window or ring row only for a packet seq >= 0 of the
        // stream's current life, so the slot's old bytes are never seen (see "bursts")
        std::unique_ptr<fec::StreamPlanner> pl(
            h->codes.empty() ? new fec::StreamPlanner(h->g, h->rules.get())
                             : new fec::StreamPlanner(h->codes[code].g, h->codes[code].rules.get()));
        if (h->codes.empty()) {
            // a one-code group's one-packet decode kernel reads the ring rows of packets before the
            // stream's start as the zero rows they were at create: zero them again, between the
            // last call and the next (both are ordered by `done`)
            if (h->stage.poisoned) return FEC_ERR_HIP;
            uint8_t* ring = h->d_ring + static_cast<size_t>(id) * fec::kRR * h->g.CW;
            FEC_HIP(hipStreamWaitEvent(nullptr, h->stage.done, 0));
            FEC_HIP(hipMemsetAsync(ring, 0, static_cast<size_t>(fec::kRR) * h->g.CW, nullptr));
            FEC_HIP(hipEventRecord(h->stage.done, nullptr));
        }
        h->planners[id] = std::move(pl);
        if (!h->codes.empty()) h->code_of[id] = code;
        h->enc_seq[id] = 0;
        h->dec_seq[id] = 0;
        return FEC_OK;
    } catch (const std::bad_alloc&) {
        return FEC_ERR_NOMEM;
    } catch (...) {
        return FEC_ERR_ARG;
    }
}

}  // extern "C"
