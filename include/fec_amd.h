/*
 * fec_amd.h -- C ABI of the MI355X-native GF(2^8) streaming-erasure codec.
 *
 * Drop-in boundary for the hot path of domanovi/FEC_Erasure_Code_Unit_Test_Relay.  Every entry
 * point takes plain pointers and sizes (no torch, no C++ types) and returns an int status
 * (FEC_OK = 0, negative = error, see fec_strerror); nothing throws across the ABI.
 *
 * Two layers:
 *   1. Streaming per-packet API (host buffers), one call per sequence number in increasing order
 *      starting at 0 -- exactly the reference's FEC_Encoder::onTransmit / FEC_Decoder::onReceive
 *      contract.  The C++ classes in fec_amd_dropin.h wrap it with the reference's names.
 *   2. Batched device-resident API: many packets of one stream per call, inputs and outputs in
 *      HBM, asynchronous on a caller-supplied hipStream_t (passed as void*; NULL = null stream).
 *
 * Wire formats are the reference's: codeword = S sub-streams of n bytes (k systematic bytes of
 * [len_hi, len_lo, payload, zero pad] then n-k parity bytes); the wire form is that codeword with
 * trailing zero bytes trimmed; a received wire codeword is zero-padded back to CW bytes.
 */
#ifndef FEC_AMD_H
#define FEC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FEC_OK 0
#define FEC_ERR_ARG (-1)          /* bad argument / unsupported (T,B,N) */
#define FEC_ERR_HIP (-2)          /* HIP runtime error (no device, launch failure, ...) */
#define FEC_ERR_NOMEM (-3)        /* allocation failed */
#define FEC_ERR_WORKSPACE (-4)    /* decode workspace too small */
#define FEC_ERR_SEQUENCE (-5)     /* streaming call out of sequence order */
#define FEC_ERR_HISTORY (-6)      /* continuing decode: not enough earlier packets in memory */

typedef struct fec_codec fec_codec;        /* one (max_payload,T,B,N) configuration on a device */
typedef struct fec_encoder fec_encoder;    /* one streaming encoder (per stream) */
typedef struct fec_decoder fec_decoder;    /* one streaming decoder (per stream) */

/* ABI version of this header, returned by fec_version().  2: fec_vr_parse_batch takes the plan
 * first and writes the compact cur/old layout (the d_cw_cur / d_cw_old of the fec_vr_* calls are
 * compact arrays since then, fec_vr.h); a caller built against version 1 must be rebuilt. */
#define FEC_AMD_ABI_VERSION 2

const char *fec_strerror(int status);
/* The last failed HIP runtime call behind an FEC_ERR_HIP (its error name and source line), as a
 * NUL-terminated string written to buf (truncated to size); returns its length, 0 when none. */
int fec_last_error(char *buf, size_t size);
int fec_version(void);

/* ---- configuration -------------------------------------------------------------------------
 * Replaces the constructors Encoder::Encoder / Decoder::Decoder (src/Encoder.cpp:26-50,
 * src/Decoder.cpp:24-53) and init_at_sender/gen_G_cauchy (src/codingOperations.cpp:48-116):
 * derives k=T-N+1, n=k+B, S=ceil((max_payload+2)/k), CW=S*n, builds G and the decode rules and
 * uploads them to the current HIP device.  Requires N <= B (as every reference configuration). */
int fec_codec_create(int max_payload, int T, int B, int N, fec_codec **out);
int fec_codec_destroy(fec_codec *codec);
int fec_codec_geometry(const fec_codec *codec, int *k, int *n, int *S, int *CW);
/* Kernel configuration chosen for this codec and device (tiles, resident workgroups), as a JSON
 * object written to buf (NUL-terminated, truncated to size). */
int fec_codec_info(const fec_codec *codec, char *buf, size_t size);
/* Encode kernel selection: 0 = automatic (the tile kernel -- contiguous runs of LDS-staged packet
 * tiles per workgroup -- when one is compiled for (k, n-k), max_payload % 4 == 0, the payload is
 * 4-byte and the codeword buffer 16-byte aligned; else the generic one), 1 = generic kernel,
 * 5 = tile kernel (FEC_ERR_ARG if unavailable).  Ids 2-4 (round 2's per-tile, streaming and
 * wave-sequence kernels, all slower) are retired and return FEC_ERR_ARG.  Every path produces
 * identical bytes; the switch exists for tests and A/B timing. */
int fec_codec_set_encode_path(fec_codec *codec, int path);
/* Host-only (no device call): the payload fetch of the tile encoder for (max_payload, T, B, N), one
 * stream (seg = 0) or the variable-rate schedule's segment mode (seg = 1).  Returns 1 when a tile
 * kernel exists for the tuple, else 0 (outputs zeroed).  R: packets per tile; issued: 16-byte
 * LDS-DMA pieces a tile's instructions cover; live_body: those fetched from memory in a tile of a
 * workgroup's run (R * ceil(max_payload / 16); the others are issued out of range); live_front:
 * those fetched in the tile in front of a run (the parity history; 0 without parity). */
int fec_encode_tile_fetch(int max_payload, int T, int B, int N, int seg, int *R, int *issued, int *live_body,
                          int *live_front);
/* The same switch for the decoder's received-packet copy kernel: 0 automatic (the LDS-tile
 * specialised kernel when one is compiled for (k, n-k) and max_payload % 4 == 0, else the generic
 * one), 1 generic, 2 LDS-tile specialised.  Ids 3-6 (barrier-free wave, persistent tile, chunk and
 * per-wave LDS-DMA pipeline copies, all measured slower in the step) are retired. */
int fec_codec_set_copy_path(fec_codec *codec, int path);
/* The same switch for the decoder's recovery kernel: 0 automatic (the (k, n-k)-specialised kernel
 * of packed GF(2^8) products when one is compiled for the pair and the k+n-1 codeword rows a packet
 * touches fit its 12 KB staging limit, for any max_payload and any alignment of the buffers; else
 * the generic one), 1 generic, 2 specialised (FEC_ERR_ARG where it does not apply).  fec_codec_info
 * names the kernel ("recover_kernel") and gives its launch's wave count: min(recover_waves,
 * ceil(output rows / recover_wave_rows)). */
int fec_codec_set_recover_path(fec_codec *codec, int path);
/* Host-only (no device call): the index arithmetic of the specialised recovery kernel, through the
 * functions the kernel itself uses (fec_recover_fast.h).  Returns its work items per packet,
 * k * ceil(S / 4), for (max_payload, T, B, N), or 0 when the kernel does not apply (outputs
 * untouched); FEC_ERR_ARG for a refused tuple or x outside [0, P - T).  With span != NULL, for
 * packet x of a P-packet buffer: span[0..1] = first and one-past-last codeword row of the
 * diagonals inside [0, P), span[2..3] = the byte range of the codeword buffer the wave loads,
 * span[4] = the LDS bytes set aside for it.  With src_off and out_idx too: src_off[(item * n + q)
 * * 4 + e] = byte of the codeword buffer that term q of the item's sub-stream e reads (-1: absent),
 * out_idx[item * 4 + e] = the byte of [len_hi, len_lo, payload] it produces (-1: none). */
int fec_recover_fast_items(int max_payload, int T, int B, int N, int64_t P, int64_t x, int64_t *span,
                           int64_t *src_off, int32_t *out_idx);
/* Host-only: c * (each byte of x4) in GF(2^8), through the kernel's packed-doubling table builder. */
uint32_t fec_recover_fast_mul(uint32_t c, uint32_t x4);
/* The same switch for the decoder's planner (per-episode block replay). */
int fec_codec_set_plan_path(fec_codec *codec, int path);
/* Planner: replay one episode per distinct loss shape and copy its results to the other episodes
 * of that shape (default 1), or replay every episode (0).  Outputs are identical either way. */
int fec_codec_set_episode_dedup(fec_codec *codec, int on);
/* Encoder::getG / Decoder::getG (src/Encoder.cpp:61, src/Decoder.cpp:68): k*n bytes row-major. */
int fec_codec_generator(const fec_codec *codec, uint8_t *G);

/* ---- batched device-resident encode --------------------------------------------------------
 * Batched FEC_Encoder::onTransmit (src/FEC_Encoder.cpp:42-68) for P consecutive packets of one
 * stream.  d_payload: P rows of max_payload bytes (row p = packet seq0+p); d_payload_len: P
 * payload lengths (<= max_payload) or NULL = all max_payload.  `history` rows BEFORE d_payload
 * (d_payload - history*max_payload, and d_payload_len - history) are earlier packets of the same
 * stream; packets before those count as zero (encoder created there).  Writes d_codeword (P rows
 * of CW bytes, untrimmed, zero padded exactly as the decoder re-pads) and d_codeword_len (P
 * trimmed wire sizes). */
int fec_encode_batch(fec_codec *codec, const uint8_t *d_payload, const int32_t *d_payload_len,
                     int64_t history, int64_t P, uint8_t *d_codeword, int32_t *d_codeword_len,
                     void *hip_stream);

/* ---- batched device-resident decode --------------------------------------------------------
 * A fresh FEC_Decoder (src/FEC_Decoder.cpp:26-72) fed packets seq 0..P-1 of one stream:
 * d_codeword: P rows of CW bytes (zero padded; rows of erased packets are never read);
 * d_erasure: P bytes, 1 = packet missing.  Produces the reference's output for packets
 * 0..P-T-1: d_payload_out ((P-T) rows of max_payload bytes, zero beyond the payload) and
 * d_payload_len ((P-T) ints, 0 = lost).  d_workspace: fec_decode_workspace_bytes(P) bytes. */
size_t fec_decode_workspace_bytes(const fec_codec *codec, int64_t P);
int fec_decode_batch(fec_codec *codec, const uint8_t *d_codeword, const uint8_t *d_erasure,
                     int64_t P, uint8_t *d_payload_out, int32_t *d_payload_len, void *d_workspace,
                     size_t workspace_bytes, void *hip_stream);
/* ---- continuing batched decode --------------------------------------------------------------
 * One stream decoded in consecutive batches, each call continuing where the previous one ended
 * (the state of src/Decoder.cpp:72-175 -- latest erasure, stored codewords, open episode -- carried
 * across calls): equal, row for row, to fec_decode_batch over the concatenated stream.
 * fec_decode_stream_push takes the next P packets (d_codeword, d_erasure on the device; h_erasure
 * the same P flags on the host -- the receiver knows which packets arrived); `history` rows
 * BEFORE each of the three pointers are the stream's preceding packets (at least T of them after
 * the first call).  It writes *n_out rows (the packets whose output became available: from the
 * first packet not yet output up to the T-th last packet pushed) to d_payload_out / d_payload_len.
 * Internally the decode restarts at the latest packet where the reference decoder is on its fast
 * path for T+1 packets on both sides; FEC_ERR_HISTORY if no such packet lies within `history`
 * (keep more earlier packets: an erasure episode never exceeds the burst length + 2T + 2).
 * Workspace: fec_decode_workspace_bytes(P + history). */
typedef struct fec_decode_stream fec_decode_stream;
int fec_decode_stream_create(fec_decode_stream **out);
int fec_decode_stream_destroy(fec_decode_stream *st);
int fec_decode_stream_push(fec_codec *codec, fec_decode_stream *st, const uint8_t *d_codeword,
                           const uint8_t *d_erasure, const uint8_t *h_erasure, int64_t P, int64_t history,
                           uint8_t *d_payload_out, int32_t *d_payload_len, int64_t *n_out,
                           void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* Packets pushed so far and the packet the last push restarted the decode at. */
int fec_decode_stream_state(const fec_decode_stream *st, int64_t *consumed, int64_t *last_cut);
/* The same decode in two halves.  fec_decode_plan needs only the erasure pattern (it can run
 * while the codewords are still being produced or transferred); fec_decode_apply needs the
 * codewords and must be ordered after the plan (same stream, or an event).  fec_decode_batch =
 * plan on an internal side stream concurrently with the systematic copy, joined before the
 * recovery pass. */
int fec_decode_plan(fec_codec *codec, const uint8_t *d_erasure, int64_t P, void *d_workspace,
                    size_t workspace_bytes, void *hip_stream);
int fec_decode_apply(fec_codec *codec, const uint8_t *d_codeword, const uint8_t *d_erasure,
                     int64_t P, uint8_t *d_payload_out, int32_t *d_payload_len, void *d_workspace,
                     size_t workspace_bytes, void *hip_stream);
/* fec_decode_apply = fec_decode_copy (received packets' rows and lengths; independent of the plan,
 * may run concurrently with it) followed by fec_decode_recover (erased packets' rows and lengths:
 * recovered bytes, or zeros and length 0 when lost; after the plan). */
int fec_decode_copy(fec_codec *codec, const uint8_t *d_codeword, const uint8_t *d_erasure,
                    int64_t P, uint8_t *d_payload_out, int32_t *d_payload_len, void *hip_stream);
int fec_decode_recover(fec_codec *codec, const uint8_t *d_codeword, int64_t P,
                       uint8_t *d_payload_out, int32_t *d_payload_len, void *d_workspace,
                       size_t workspace_bytes, void *hip_stream);
/* After the stream has finished the decode: erasure episodes, recovered and lost packets. */
int fec_decode_counters(const void *d_workspace, int64_t *episodes, int64_t *recovered,
                        int64_t *lost);
/* Planner statistics of the last plan in d_ws: episodes replayed and episodes filled from a
 * replayed episode of the same loss shape (fec_codec_set_episode_dedup). */
int fec_decode_plan_stats(const void *d_ws, int64_t *replayed, int64_t *filled);

/* ---- many independent streams, one packet of each per call ---------------------------------
 * A group of `nstreams` independent streams of one (max_payload,T,B,N): the state of one
 * FEC_Encoder and one FEC_Decoder per stream (include/FEC_Encoder.h:26-48, FEC_Decoder.h:27-46)
 * held in HBM (encoder windows, decoder codeword rings) plus the decoders' symbolic state on the
 * host.  One call hands over the next packet of each of M distinct streams (ids[m], host array)
 * and codes all of them in one launch -- the relay / receiver load of many 300-byte streams.
 *   fec_streams_encode  = FEC_Encoder::onTransmit per stream: d_payload M rows of max_payload
 *                         bytes, d_payload_len M sizes (NULL = all max_payload) -> d_codeword M rows
 *                         of CW bytes (untrimmed) + d_codeword_len M trimmed wire sizes.
 *   fec_streams_decode  = FEC_Decoder::onReceive per stream: erasure M host flags (1 = packet
 *                         missing), d_codeword M rows of CW bytes (zero padded; rows of missing
 *                         packets are not read) -> d_payload_out row m = the stream's packet seq-T
 *                         (seq = packets that stream had received before), d_payload_len m
 *                         (0 = lost or not available yet).
 * Asynchronous on hip_stream; ids must be distinct within a call (FEC_ERR_ARG otherwise). */
typedef struct fec_streams fec_streams;
int fec_streams_create(int max_payload, int T, int B, int N, int nstreams, fec_streams **out);
int fec_streams_destroy(fec_streams *group);
int fec_streams_encode(fec_streams *group, const int32_t *ids, int M, const uint8_t *d_payload,
                       const int32_t *d_payload_len, uint8_t *d_codeword, int32_t *d_codeword_len,
                       void *hip_stream);
int fec_streams_decode(fec_streams *group, const int32_t *ids, int M, const uint8_t *erasure,
                       const uint8_t *d_codeword, uint8_t *d_payload_out, int32_t *d_payload_len,
                       void *hip_stream);
/* Bursts: one call hands over counts[m] >= 1 consecutive packets of each of M distinct streams
 * (ids, counts: host arrays).  With R = the sum of the counts, every row array has R rows (payload,
 * sizes, codewords, the host erasure flags, the outputs), stream ids[m]'s rows starting at row
 * counts[0] + ... + counts[m-1], its next counts[m] packets in order.  A call equals counts[m]
 * one-packet calls per stream, byte for byte and in the group's state afterwards, and bursts and
 * one-packet calls on one group continue each other; R is not bounded by nstreams.  The burst
 * kernels (fec_streams.hip) cut a burst into chunks of up to 32 packets, one workgroup each: a
 * chunk takes the packets in front of it from the call's own rows, the stream's state in HBM is
 * read by a burst's first chunk only and written once per burst (the last n-1 windows, the last
 * T+k codewords); parity runs on packed 4-byte GF tables over LDS, a received row costs one
 * staged byte, only recovered rows carry a coefficient block.  Measured on an MI355X at 10 000
 * streams of (10,3,3), 300-byte payloads, encode + decode with the host's symbolic steps
 * (tools/streams_burst_ab.py, profiles/streams_burst/): 12.2 ns per packet one packet per call,
 * 8.9 ns in bursts of 4, 3.43 ns in bursts of 16, 2.67 ns in bursts of 64; the burst kernels
 * alone run at 0.07 - 0.11 of the 8.0 TB/s peak over L + CW / CW + 1 + L bytes per packet.
 * FEC_ERR_ARG (group unchanged): repeated or out-of-range id, count < 1, null pointer, or a
 * geometry whose smallest chunk does not fit a CU's 160 KB of LDS: an encode chunk holds
 * 2(n-1) windows as position planes plus the larger of 2(n-1) payload rows and n-1 codewords plus
 * n-1 ring windows, a decode chunk 2(T+k-1) codewords plus T+k-1 payload rows and k x n blocks --
 * (10,3,3) fits at every max_payload a group takes (up to 1 500 bytes; 99 KB for the decode
 * chunk there), (24,12,12) at 1 500 bytes does not.  Any other failure
 * after the arguments passed (a HIP call, among them growing the pinned staging buffer to the
 * call, or memory for the decode's records) poisons the group like a failed one-packet decode:
 * every later call returns FEC_ERR_HIP. */
int fec_streams_encode_burst(fec_streams *group, const int32_t *ids, const int32_t *counts, int M,
                             const uint8_t *d_payload, const int32_t *d_payload_len,
                             uint8_t *d_codeword, int32_t *d_codeword_len, void *hip_stream);
int fec_streams_decode_burst(fec_streams *group, const int32_t *ids, const int32_t *counts, int M,
                             const uint8_t *erasure, const uint8_t *d_codeword,
                             uint8_t *d_payload_out, int32_t *d_payload_len, void *hip_stream);
/* Host only, no device: the symbolic half of fec_streams_decode_burst for one stream fed its
 * packets in bursts of counts[0 .. ncounts-1] -- fate[x] for packets 0 .. sum(counts)-T-1 in
 * fec_plan_host's encoding, through the routine the decode call builds its records with. */
int fec_streams_plan_burst_host(int max_payload, int T, int B, int N, const uint8_t *erasure,
                                const int32_t *counts, int ncounts, uint8_t *fate);
/* Packets stream `id` has sent (encoded) and received (decoded) so far. */
int fec_streams_state(const fec_streams *group, int id, int64_t *sent, int64_t *received);
/* Mixed groups: every stream has its own code, and one call codes streams of different (T,B,N) in
 * one launch per direction -- the node that serves many flows of the adaptive loop, each on the code
 * its own loss calls for.  tuples: ncodes x {T,B,N} (1 <= ncodes <= 64, equal tuples may repeat),
 * code_of: nstreams indices into it.  FEC_ERR_ARG, nothing created: a tuple fec_streams_create
 * refuses at this max_payload, a tuple whose smallest burst chunk does not fit the LDS in either
 * direction (fec_streams_mixed_fit), a code index outside [0, ncodes), a null pointer.
 * The result is an ordinary group: fec_streams_encode / _decode / _encode_burst / _decode_burst /
 * _state / _destroy take it unchanged, with this row layout: payload rows are max_payload bytes;
 * codeword rows, in and out, have one stride for the whole group, cw_stride = the largest CW of its
 * codes (a one-code group is this case with cw_stride = CW).  A stream's codeword is the first CW
 * bytes of its row, CW its own code's; encode writes zero into the rest of the row, decode never
 * reads it.  Output row m of a decode call is packet seq - T of stream ids[m], with its own T.  Per
 * stream, all its rows over all calls equal fec_encode_batch / fec_decode_batch of its own (T,B,N)
 * over its whole sequence, whatever the cutting into one-packet calls and bursts and whichever
 * streams shared its calls.  Both directions run the two mixed kernels (fec_streams.hip: the burst
 * kernels' chunks, each with its code's geometry from a table in device memory), one-packet calls
 * as chunks of one packet; a code's chunk size is fixed at create, and a launch takes the LDS of the
 * largest chunk among the codes present in that call.  Device state per stream: a window slot of
 * max_c((n_c-1) S_c k_c) bytes and a ring of 64 rows of cw_stride bytes. */
int fec_streams_create_mixed(int max_payload, const int32_t *tuples, int ncodes,
                             const int32_t *code_of, int nstreams, fec_streams **out);
/* The number of codes of a group (1 for fec_streams_create's) and its codeword row stride. */
int fec_streams_codes(const fec_streams *group, int *ncodes, int *cw_stride);
/* Stream `id`'s code index and that code's geometry (any pointer may be NULL). */
int fec_streams_stream_geometry(const fec_streams *group, int id, int *code, int *T, int *k, int *n,
                                int *S, int *CW);
/* Makes stream `id` a fresh encoder and a fresh decoder of code `code`, as an adaptive endpoint
 * does when it constructs a new FEC_Encoder at a switch: both seq counters go to 0 and the
 * decoder's symbolic state is new.  Host work on a mixed group (calls already queued carry their
 * own seqs; the kernels never read a stream's device state from before seq 0).  The old code's
 * last T packets are never output: a caller that wants them keeps the old stream id alive beside
 * the new one through the double-coded seqs.  On a group made by fec_streams_create only code 0
 * is accepted, and resets the stream.  FEC_ERR_ARG (group unchanged): id or code out of range. */
int fec_streams_set_code(fec_streams *group, int id, int code);
/* Host only, no device call: per code the packets per chunk and the LDS bytes of the mixed group's
 * encode and decode chunks (ncodes entries each), through the routines the calls use; a chunk lies
 * between the packets it needs in front of it (n-1 / T+k-1) and 32.  FEC_ERR_ARG if any tuple is
 * refused or does not fit, ncodes is outside [1, 64] or a pointer is null. */
int fec_streams_mixed_fit(int max_payload, const int32_t *tuples, int ncodes, int32_t *enc_chunk,
                          int32_t *enc_lds, int32_t *dec_chunk, int32_t *dec_lds);

/* ---- per-kernel timing (HIP events recorded on the launch stream) --------------------------- */
#define FEC_KERNEL_ENCODE 0
#define FEC_KERNEL_DEC_SCAN 1
#define FEC_KERNEL_DEC_PLAN 2
#define FEC_KERNEL_DEC_COPY 3
#define FEC_KERNEL_DEC_RECOVER 4
#define FEC_KERNEL_COUNT 5
int fec_timing_enable(fec_codec *codec, int enable);
/* Synchronises the recorded events; total_ms[FEC_KERNEL_COUNT], launches[FEC_KERNEL_COUNT]. */
int fec_timing_collect(fec_codec *codec, double *total_ms, int64_t *launches);

/* Diagnostics: the next launches of `kernel` (FEC_KERNEL_ENCODE or FEC_KERNEL_DEC_COPY, the
 * specialised kernels) write s_memtime phase stamps, 8 uint64 per workgroup, to d_stamps
 * (NULL switches it off).  Timing-only; no output depends on it. */
int fec_debug_stamps(fec_codec *codec, int kernel, void *d_stamps);

/* ---- streaming per-packet API (host buffers) -----------------------------------------------
 * fec_encoder_transmit = FEC_Encoder::onTransmit: data (payload bytes), payload (<= max_payload),
 * seq (0,1,2,... consecutive); writes the wire codeword (cw_out must hold CW bytes; the trimmed
 * length goes to *codeword_size, bytes past it are zero).
 * fec_decoder_receive = FEC_Decoder::onReceive: codeword/codeword_size = wire bytes (ignored when
 * erasure != 0), seq consecutive from 0; writes packet seq-T's payload to payload_out
 * (max_payload bytes, zero beyond) and its length to *payload (0 = lost / not yet available).
 * Each call is one kernel launch (the stream-group kernels of fec_streams.hip on a one-stream
 * window / ring) reading and writing pinned, mapped host rows, and a poll of a completion word
 * (FEC_STREAM_SPIN=0: hipStreamSynchronize instead).  The encoder needs k = T-N+1 <= 16. */
int fec_encoder_create(int max_payload, int T, int B, int N, fec_encoder **out);
int fec_encoder_destroy(fec_encoder *enc);
int fec_encoder_transmit(fec_encoder *enc, const uint8_t *data, int payload, int seq,
                         uint8_t *cw_out, int *codeword_size);
int fec_decoder_create(int max_payload, int T, int B, int N, fec_decoder **out);
int fec_decoder_destroy(fec_decoder *dec);
int fec_decoder_receive(fec_decoder *dec, const uint8_t *codeword, int codeword_size, int seq,
                        int erasure, uint8_t *payload_out, int *payload);

/* ---- host-side planner probe (control plane only, no device needed) -------------------------
 * Runs the symbolic decoder over an erasure pattern of P packets and reports, for packets
 * 0..P-T-1, fate[x] (1 copy, 2 recovered, 3 lost).  Used by tests and by the streaming decoder. */
int fec_plan_host(int max_payload, int T, int B, int N, const uint8_t *erasure, int64_t P,
                  uint8_t *fate);

/* ---- block mode: many independent code blocks ------------------------------------------------
 * Batched forms of the reference's free functions as the relay (Decoder_Symbol_Wise,
 * src/Decoder_Symbol_Wise.cpp:322-328, 532-533, 573-575, 610, 643) calls them per code block:
 *   encodeBlock(data, G, cw, k, n, t = k-1)  (src/codingOperations.cpp:131-147): d_data nblk x k ->
 *     d_codeword nblk x n = [data, parity] (the relay pre-fills cw with the data, so the k-1
 *     systematic bytes encodeBlock leaves alone are the data too);
 *   decodeBlock(cw, G, cw, erasure, k, n, T = n-1, t = 0)  (src/codingOperations.cpp:149-232):
 *     d_codeword nblk x n + d_erasure nblk x n (1 = erased) -> d_out nblk x n with every data symbol
 *     the reference recovers written in, d_erasure_out (may be NULL) with those flags cleared.
 * G is the codec's generator (init_at_sender for its (T,B,N)). */
int fec_block_encode_batch(fec_codec *codec, const uint8_t *d_data, int64_t nblk, uint8_t *d_codeword,
                           void *hip_stream);
int fec_block_decode_batch(fec_codec *codec, const uint8_t *d_codeword, const uint8_t *d_erasure,
                           int64_t nblk, uint8_t *d_out, uint8_t *d_erasure_out, void *hip_stream);

/* ---- variable-rate (adaptive) coding: BASELINE config 4 --------------------------------------
 * The reference's P2P loop (application_local_simulation.cpp:328-345): Application_Layer_Sender +
 * Variable_Rate_FEC_Encoder (src/Variable_Rate_FEC_Encoder.cpp:74-235) with double coding at every
 * (T,B,N) switch, Application_Layer_Receiver + foreground/background Parameter_Estimator
 * (src/Parameter_Estimator.cpp:58-190, swapped every 100 packets) + Variable_Rate_FEC_Decoder
 * (src/Variable_Rate_FEC_Decoder.cpp:2133-2400), the receiver's 6-byte feedback read by the sender at
 * the next packet.  Everything but the coding bytes depends only on the erasure pattern, so a plan
 * runs the loop symbolically on the host and records the schedule; the byte work then runs batched
 * on the device.  T = T_INITIAL, B = N = -1 for adaptive (else fixed (T,B,N)); the pattern is the
 * receiver's erasure.bin (ERASURE_TYPE 5: packets seq < P+T with pattern byte 1 are dropped); P =
 * NUMBER_OF_ITERATIONS, the packets whose outputs are counted. */
typedef struct fec_vr_plan fec_vr_plan;
int fec_vr_plan_create(int max_payload, int T, int B, int N, int adaptive_mode_MDS,
                       const uint8_t *erasure, int64_t n_erasure, int64_t P, fec_vr_plan **out);
int fec_vr_plan_destroy(fec_vr_plan *plan);
/* Plan again, in place, with the plan's (max_payload, T, B, N, adaptive_mode_MDS) on a new pattern
 * and P: the host buffers, device tables and worker threads of the plan are reused.  async != 0:
 * returns after the serial control loop (instances, frames, sent, switches final); the symbolic
 * decoder instances run on worker threads meanwhile, so fec_vr_encode_batch's launch overlaps them;
 * every call that needs their results (stats, timing, packets, decode) waits for them. */
int fec_vr_plan_rerun(fec_vr_plan *plan, const uint8_t *erasure, int64_t n_erasure, int64_t P, int async);
/* lost: packets among 0..P-1 the receiver outputs empty ("Final FEC loss rate" x P); switches:
 * "Start double coding at the source" count; coding_rate: Variable_Rate_FEC_Encoder's final rate;
 * sent: packets the sender produced; cw_max: the widest codeword row (16-byte multiple). */
int fec_vr_plan_stats(const fec_vr_plan *plan, int64_t *lost, int64_t *switches, double *coding_rate,
                      int64_t *sent, int *n_encoders, int *n_decoders, int *cw_max);
/* wall time of the plan's two phases: the serial control loop (sender, estimators, switches,
 * decoder swaps) and the parallel symbolic decoder instances, in ms */
int fec_vr_plan_timing(const fec_vr_plan *plan, double *control_ms, double *decoders_ms);
/* the control loop's time waiting for the estimator feedback jobs (which run on the plan's worker
 * threads, ahead of its decoder jobs) in the last run */
int fec_vr_plan_feedback_wait(const fec_vr_plan *plan, double *waited_ms);
/* instances, 6 int64 each: T, B, N, first seq, seq from which it is the old one, end seq */
int fec_vr_plan_instances(const fec_vr_plan *plan, int64_t *encoders, int64_t *decoders);
/* per sent packet: frames (6 int32: header T, B, N, counter_for_start_and_end, current encoder,
 * old encoder or -1), erased (1 = dropped); per counted packet x < P: fate (1 received, 2
 * recovered, 3 lost) and the decoder instance that reported it.  NULL pointers are skipped. */
int fec_vr_plan_packets(const fec_vr_plan *plan, int32_t *frames, uint8_t *erased, uint8_t *fate,
                        int32_t *fate_decoder);
/* Device-resident execution.  The frames' codewords live in two compact arrays (no per-row padding
 * beyond 16-byte alignment): row s of d_cw_cur = the codeword of frame s's current encoder, row s
 * of d_cw_old = the old encoder's during double coding (empty otherwise); each row is its
 * instance's CW rounded up to 16 bytes, rows in seq order.  fec_vr_plan_layout gives the two array
 * sizes, fec_vr_plan_row_offsets the per-row byte offsets (sent + 1 each, prefix form).  Encode:
 * d_payload (sent rows of max_payload bytes) -> d_cw_cur / d_cw_old rows, trimmed sizes in
 * d_len_cur / d_len_old (sent each; 0 when no old codeword).  Decode: those arrays + d_erased
 * (sent bytes) -> d_out (P rows of max_payload) and d_out_len (P ints, 0 = lost), the receiver's
 * reported outputs. */
int fec_vr_plan_layout(const fec_vr_plan *plan, int64_t *cur_bytes, int64_t *old_bytes);
int fec_vr_plan_row_offsets(const fec_vr_plan *plan, int64_t *cur_off, int64_t *old_off);
int fec_vr_encode_batch(fec_vr_plan *plan, const uint8_t *d_payload, const int32_t *d_payload_len,
                        uint8_t *d_cw_cur, int32_t *d_len_cur, uint8_t *d_cw_old, int32_t *d_len_old,
                        void *hip_stream);
int fec_vr_decode_batch(fec_vr_plan *plan, const uint8_t *d_cw_cur, const uint8_t *d_cw_old,
                        const uint8_t *d_erased, uint8_t *d_out, int32_t *d_out_len, void *hip_stream);
/* Wire framing above the boundary.  Sender: row s of d_packets (stride >= 10 + 2*cw_max) = the P2P
 * packet Application_Layer_Sender sends (Application_Layer_Sender.cpp:259-269): [seq BE32][T][B][N]
 * [counter_for_start_and_end] + Variable_Rate_FEC_Encoder's frame (Variable_Rate_FEC_Encoder.cpp:
 * 194-217): [size_current BE16][codeword_current (trimmed)][codeword_old (trimmed)]; sizes in
 * d_packet_len.  Receiver: the split of the plan's sent packets into the current / old codeword
 * rows of the compact arrays, zero-padded to their row size (Application_Layer_Receiver.cpp:361-366,
 * Variable_Rate_FEC_Decoder.cpp:2156-2160), header fields to d_header (sent x 5 int32: seq, T, B,
 * N, counter; may be NULL). */
int fec_vr_frames_batch(fec_vr_plan *plan, const uint8_t *d_cw_cur, const int32_t *d_len_cur,
                        const uint8_t *d_cw_old, const int32_t *d_len_old, uint8_t *d_packets,
                        int64_t stride, int32_t *d_packet_len, void *hip_stream);
int fec_vr_parse_batch(fec_vr_plan *plan, const uint8_t *d_packets, int64_t stride, const int32_t *d_packet_len,
                       uint8_t *d_cw_cur, uint8_t *d_cw_old, int32_t *d_header, void *hip_stream);

/* ---- relay: symbol-wise decode-and-forward (SWDF, RELAYING_TYPE 2) ---------------------------
 * Decoder_Symbol_Wise (src/Decoder_Symbol_Wise.cpp) as the relay and the destination drive it
 * (src/Variable_Rate_FEC_Decoder.cpp:950-1601 relay, :1603-1879 destination; one relay frame per
 * seq as with FLAG_FOR_CONSTANT_TRANS = 1, application_local_simulation.cpp:532-587), fixed rate.
 * Hop 1 carries the source's FEC_Encoder(max_payload, T1, N1, N1) codewords; the relay decodes
 * with window n1 = T1+1 and re-encodes for n2 = T2+1 with k = T1-N1+1 = T2-N2+1 (k2 == k, the
 * only case the reference handles).  Batches run a fresh relay / destination over seqs 0..P-1.
 *   fec_swdf_relay_batch: d_cw P rows of cw_stride bytes (the source codewords, zero-padded to at
 *     least S*n1 bytes; rows of erased packets are never read), d_erasure P hop-1 flags ->
 *     d_frames P rows of frame_bytes (the relay's transmitted frame: [size BE16][codeword_new_vector
 *     [n2-1][0..size)], size = (S+1)*n2), d_flag P bytes (may be NULL): 1 when the window held too
 *     many erasures to decode (the relay's loss counter).  d_work: fec_swdf_workspace_bytes(P).
 *   fec_swdf_destination_batch: d_frames + d_erasure P hop-2 flags -> d_out P rows of S*k bytes:
 *     row t = data_with_header ([len BE16][payload][zero pad]) of source packet t - delay, as
 *     symbol_wise_decode_1 + extract_data produce it; d_flag as above (may be NULL). */
typedef struct fec_swdf fec_swdf;
int fec_swdf_create(int max_payload, int T1, int N1, int T2, int N2, fec_swdf **out);
int fec_swdf_destroy(fec_swdf *swdf);
/* delay = n1 + n2 - k - 1: destination row t carries source packet t - delay */
int fec_swdf_geometry(const fec_swdf *swdf, int *k, int *n1, int *n2, int *S, int *frame_bytes,
                      int *delay);
size_t fec_swdf_workspace_bytes(const fec_swdf *swdf, int64_t P);
int fec_swdf_relay_batch(fec_swdf *swdf, const uint8_t *d_cw, int64_t cw_stride, const uint8_t *d_erasure,
                         int64_t P, uint8_t *d_frames, uint8_t *d_flag, void *d_work, size_t work_bytes,
                         void *hip_stream);
int fec_swdf_destination_batch(fec_swdf *swdf, const uint8_t *d_frames, const uint8_t *d_erasure, int64_t P,
                               uint8_t *d_out, uint8_t *d_flag, void *hip_stream);

/* ---- relay stream groups: SWDF for many relay streams per launch ------------------------------
 * nstreams independent type-2 relay chains of one (max_payload, T1, N1, T2, N2) (the constraints of
 * fec_swdf_create, and n1, n2 <= 17: the window-n rule tables), each stream's state on the device
 * between calls: one Decoder_Symbol_Wise per stream and side, fed one packet or a burst per call.
 * A relay node uses the relay side, a destination node the destination side of one group.
 *   fec_relay_streams_relay = push_current_codeword / rotate_pointers_and_insert_zero_word +
 *     symbol_wise_encode_1 (src/Decoder_Symbol_Wise.cpp:119-176, :547-619, driven by
 *     Variable_Rate_FEC_Decoder.cpp:950-1601) for the next counts[m] seqs of stream ids[m];
 *   fec_relay_streams_destination = the same window over the relay's frames + symbol_wise_decode_1 +
 *     extract_data (:621-665, driven by Variable_Rate_FEC_Decoder.cpp:1603-1879).
 * Rows: ids M distinct stream ids (host); counts M burst sizes >= 1 (host; NULL: one packet of
 * each); with R = the sum of the counts every row array has R rows, stream ids[m]'s from row
 * counts[0] + .. + counts[m-1] on, its next counts[m] seqs in order (the layout of
 * fec_streams_encode_burst; R is not bounded by nstreams).  erasure: R host flags.  d_cw: R rows of
 * cw_stride >= S*n1 bytes (rows of erased packets are never read); d_frames: R rows of frame_bytes;
 * d_out: R rows of S*k bytes (data_with_header of source packet seq - delay); d_flag: R bytes (may be
 * NULL), 1 when the row's window held n-k+1 or more erasures.  Per stream, the rows of all calls
 * together equal fec_swdf_relay_batch / fec_swdf_destination_batch over the stream's whole sequence
 * from seq 0, row for row; one-packet calls and bursts continue each other.
 * No pointer or row needs any alignment (frame rows are 431 bytes at (10,3,10,3)).
 * Calls on different HIP streams are ordered by the group.  FEC_ERR_ARG (a repeated or out-of-range
 * id, a count < 1, a null pointer, cw_stride < S*n1; at create a geometry whose smallest chunk does
 * not fit a CU's LDS) leaves the group unchanged; any later failure poisons it (every further call
 * returns FEC_ERR_HIP). */
typedef struct fec_relay_streams fec_relay_streams;
int fec_relay_streams_create(int max_payload, int T1, int N1, int T2, int N2, int nstreams,
                             fec_relay_streams **out);
int fec_relay_streams_destroy(fec_relay_streams *group);
/* Mixed groups: every stream has its own (T1, N1, T2, N2), and one call serves streams of different
 * codes in one launch per side -- the relay or destination node of many flows under variable rate,
 * each on the code its own loss calls for.  tuples: ncodes x {T1, N1, T2, N2} (1 <= ncodes <= 64,
 * equal tuples may repeat), code_of: nstreams indices into it.  FEC_ERR_ARG, nothing created: a tuple
 * fec_relay_streams_create refuses at this max_payload, a tuple of which either side's smallest chunk
 * does not fit a CU's LDS (fec_relay_streams_mixed_fit), a code index outside [0, ncodes), a null
 * pointer.  The result is an ordinary group: fec_relay_streams_relay / _destination / _state /
 * _destroy take it unchanged, with this row layout: each row array has one stride for the whole group
 * (fec_relay_streams_codes).  d_cw rows: cw_stride >= the largest S*n1 of the group's codes; a
 * stream's codeword is the first S*n1 bytes of its own code, the rest of the row is never read.
 * d_frames rows: frame_stride = the largest frame size 2 + (S+1)*n2; the relay writes the stream's
 * frame into the first bytes and zero behind it, the destination reads the stream's own frame bytes
 * only.  d_out rows: out_stride = the largest S*k; the stream's data_with_header row, then zero.
 * Per stream, the rows of all calls together equal fec_swdf_relay_batch / _destination_batch of its
 * own tuple over its sequence from seq 0, whatever the cutting and whichever streams shared its
 * calls.  Both sides run the table-driven kernels (fec_relay_streams.hip: the one-code kernels' chunk
 * body with the code's geometry from a table in device memory); a call cuts a stream's burst into
 * chunks of min(the call's longest burst, its code's chunk size) packets, and a launch takes the LDS
 * of the largest chunk among the codes present in that call.  Device state per stream: a relay ring
 * slot of max_c((n1_c+n2_c-2) S_c n1_c) bytes and a destination ring slot of max_c((n2_c-1) S_c n2_c). */
int fec_relay_streams_create_mixed(int max_payload, const int32_t *tuples, int ncodes,
                                   const int32_t *code_of, int nstreams, fec_relay_streams **out);
/* The number of codes of a group (1 for fec_relay_streams_create's, whose strides are its own sizes)
 * and its row strides: the least cw_stride, the frame rows' and the output rows'. */
int fec_relay_streams_codes(const fec_relay_streams *group, int *ncodes, int *cw_bytes, int *frame_stride,
                            int *out_stride);
/* Stream `id`'s code index and that code's geometry: cw_bytes = S*n1, frame_bytes = 2 + (S+1)*n2,
 * out_bytes = S*k, delay = n1 + n2 - k - 1 (any pointer may be NULL). */
int fec_relay_streams_stream_geometry(const fec_relay_streams *group, int id, int *code, int *k, int *n1,
                                      int *n2, int *S, int *cw_bytes, int *frame_bytes, int *out_bytes,
                                      int *delay);
/* Makes stream `id` a fresh relay chain and a fresh destination chain of code `code`, as the relay
 * under variable rate starts a fresh fixed-rate chain per code instance: both seq counters go to 0
 * and both flag registers to zero.  Host work only (calls already queued carry their own seqs; the
 * kernels never read a stream's device state from before seq 0).  The old chain's remaining outputs
 * are not produced: a caller that wants them through the double-coded seqs keeps the old stream id
 * alive beside a second id.  On a group made by fec_relay_streams_create only code 0 is accepted,
 * and resets the stream.  FEC_ERR_ARG (group unchanged): id or code out of range. */
int fec_relay_streams_set_code(fec_relay_streams *group, int id, int code);
/* Host only, no device call: per code the packets per chunk of a long burst and that chunk's LDS
 * bytes on the relay and on the destination side (ncodes entries each), through the routines the
 * calls use: entry c is fec_relay_streams_fit of tuple c.  FEC_ERR_ARG if any tuple is refused or
 * does not fit, ncodes is outside [1, 64] or a pointer is null. */
int fec_relay_streams_mixed_fit(int max_payload, const int32_t *tuples, int ncodes, int32_t *relay_chunk,
                                int32_t *relay_lds, int32_t *dest_chunk, int32_t *dest_lds);
/* cw_bytes = S*n1; delay = n1 + n2 - k - 1 (fec_swdf_geometry).  A group of one code; FEC_ERR_ARG
 * for a group of several (fec_relay_streams_stream_geometry answers per stream). */
int fec_relay_streams_geometry(const fec_relay_streams *group, int *k, int *n1, int *n2, int *S, int *cw_bytes,
                               int *frame_bytes, int *delay);
int fec_relay_streams_relay(fec_relay_streams *group, const int32_t *ids, const int32_t *counts, int M,
                            const uint8_t *erasure, const uint8_t *d_cw, int64_t cw_stride, uint8_t *d_frames,
                            uint8_t *d_flag, void *hip_stream);
int fec_relay_streams_destination(fec_relay_streams *group, const int32_t *ids, const int32_t *counts, int M,
                                  const uint8_t *erasure, const uint8_t *d_frames, uint8_t *d_out,
                                  uint8_t *d_flag, void *hip_stream);
/* seqs stream id has been fed so far on the relay / the destination side */
int fec_relay_streams_state(const fec_relay_streams *group, int id, int64_t *relayed, int64_t *delivered);
/* Host only, no device call.  fit: whether a side (relay != 0: the relay's) of this geometry fits a
 * CU's LDS: 1 with the packets per chunk of long bursts and that chunk's LDS bytes, 0 if not even the
 * smallest chunk fits, FEC_ERR_ARG for a tuple fec_relay_streams_create refuses.
 * plan_host: the flag half of a side for one stream from seq 0 fed in bursts of counts[]: per row the
 * n-bit window mask (bit m = flag of seq t-n+1+m, zero before seq 0: the index of the codec's
 * window-n decode rule, decodeBlock(T = n-1, t = 0), Decoder_Symbol_Wise.cpp:570-573, :640-643) and
 * the loss flag popcount(mask) >= n-k+1. */
int fec_relay_streams_fit(int relay, int max_payload, int T1, int N1, int T2, int N2, int *chunk_packets,
                          int *lds_bytes);
int fec_relay_streams_plan_host(int k, int n, const uint8_t *erasure, const int32_t *counts, int ncounts,
                                uint32_t *mask, uint8_t *flag);

/* ---- message-wise relay stream groups: hop-1 decode and hop-2 encode in one launch -------------
 * nstreams independent type-1 (message-wise decode-and-forward) relays at fixed rate, all of one
 * (max_payload, T1,B1,N1, T2,B2,N2), each flow's state on the device between calls: per flow an
 * FEC_Decoder of the hop-1 code (FEC_Decoder.cpp:38-75; its ring of received codewords :55-63,
 * Decoder::decodeStream, Decoder.cpp:72-175) feeding an FEC_Encoder of the hop-2 code
 * (FEC_Encoder.cpp:38-62; the window of Encoder.cpp:73-95, the trimmed size FEC_Encoder.cpp:55-60),
 * one packet or a burst per call.  Both tuples must be ones fec_streams_create takes at
 * max_payload.  This is the fixed-rate relay of the per-packet contract; the reference's adaptive
 * message-wise session (Variable_Rate_FEC_Decoder's stored messages, the 12-byte relay header,
 * T2_ack) is not built here.  The destination is an ordinary (T2,B2,N2) decoder:
 * fec_streams_decode_burst of a fec_streams group serves it, and there is no destination entry.
 *
 * Rows as in fec_relay_streams_relay: ids M distinct flow ids (host); counts M burst sizes >= 1
 * (host; NULL: one packet of each); R = the sum of the counts; erasure R host flags; d_cw1 R rows of
 * cw1_stride >= cw1_bytes = S1*n1 bytes, the flow's next hop-1 codewords untrimmed (rows of erased
 * packets are never read); d_cw2 R rows of cw2_bytes = S2*n2; d_cw2_len R trimmed wire sizes (as
 * fec_streams_encode_burst's); d_fate R bytes (may be NULL): 0 none, 1 copied, 2 recovered, 3 lost
 * (fec_plan_host's encoding).  For hop-1 seq t of a flow: t < T1 gives a zero row, size 0, fate 0,
 * and the hop-2 encoder does not advance; t >= T1 gives the hop-2 codeword number t - T1 of the
 * message the hop-1 decoder outputs at seq t, its length clipped to [0, max_payload]; a message the
 * relay loses is forwarded as the empty message, so relay seq and source seq stay equal.
 * Per flow the rows of all calls together equal fec_streams_decode_burst over the flow's hop-1
 * sequence, the first T1 rows dropped, then fec_streams_encode_burst over the rest -- byte for byte
 * with the zero pad, sizes and fates too, whatever the cutting into calls and whichever flows share
 * a call.  No pointer or row needs any alignment.  Calls on different HIP streams are ordered by
 * the group.
 * One workgroup per chunk of at most 32 packets decodes its messages straight into the encoder's
 * position planes in LDS and encodes them: no payload row is written or read.  A chunk behind a
 * burst's first decodes the n2-1 messages in front of it again, so a burst cut in several has
 * chunks of at least T1+k1-1 + n2-1 packets (fec_mw_relay_streams_fit).
 * FEC_ERR_ARG (group unchanged): a repeated or out-of-range id, a count < 1, a null pointer,
 * cw1_stride < cw1_bytes; at create a tuple fec_streams_create refuses, or a pair whose smallest
 * chunk T1+k1-1 + n2-1 exceeds 32 packets or a CU's 160 KB of LDS ((24,12,12) -> (24,12,12)).  Any
 * later failure poisons the group (every further call returns FEC_ERR_HIP). */
typedef struct fec_mw_relay_streams fec_mw_relay_streams;
int fec_mw_relay_streams_create(int max_payload, int T1, int B1, int N1, int T2, int B2, int N2, int nstreams,
                                fec_mw_relay_streams **out);
int fec_mw_relay_streams_destroy(fec_mw_relay_streams *group);
/* Mixed groups: every flow has its own pair of codes (T1,B1,N1) -> (T2,B2,N2), and one call serves
 * flows of different pairs in one launch -- the relay node of many flows under the adaptive loop, each
 * hop of each flow on the code its own loss calls for.  This replaces one fec_mw_relay_streams_create
 * group and one call per pair.  pairs: ncodes x {T1,B1,N1,T2,B2,N2} (1 <= ncodes <= 64, equal pairs
 * may repeat), code_of: nstreams indices into it.  FEC_ERR_ARG, nothing created: a pair
 * fec_mw_relay_streams_create refuses at this max_payload (a tuple fec_streams_create refuses, or a
 * smallest chunk T1+k1-1 + n2-1 over 32 packets or over a CU's LDS; fec_mw_relay_streams_mixed_fit), a
 * code index outside [0, ncodes), ncodes out of range, a null pointer.  The result is an ordinary
 * group: fec_mw_relay_streams_relay / _state / _destroy take it unchanged, with this row layout: each
 * row array has one stride for the whole group (fec_mw_relay_streams_codes).  d_cw1 rows: cw1_stride >=
 * the largest S1*n1 of the group's pairs; a flow's codeword is the first S1*n1 bytes of its own code,
 * the rest of the row and rows of erased packets are never read.  d_cw2 rows: cw2_stride = the largest
 * S2*n2; the flow's hop-2 codeword, then zeros up to the stride (a row of hop-1 seq < T1 is zero
 * across the whole stride); nothing outside a row is written.  d_cw2_len, d_fate: as in a one-code
 * group.  Per flow, the rows of all calls together equal the one-code contract of the flow's own pair
 * (fec_streams_decode_burst over its hop-1 sequence, the first T1 rows dropped, then
 * fec_streams_encode_burst with lengths clipped to [0, max_payload]) byte for byte, sizes and fates
 * too, whatever the cutting into one-packet calls and bursts and whichever flows share a call.  No
 * pointer or row needs any alignment.
 * The table-driven kernel runs the one-code kernel's chunk body with the pair's geometry from a table
 * in device memory; a call cuts a flow's burst into chunks of min(the call's longest burst, its pair's
 * chunk size) packets, and a launch takes the LDS of the largest such chunk among the pairs present in
 * that call.  Device state per flow: a codeword ring slot of 64 x max_c(S1_c n1_c) bytes and a window
 * slot of max_c(max(n2_c - 1, 1) S2_c k2_c) bytes rounded up to 16; one codec per distinct hop code. */
int fec_mw_relay_streams_create_mixed(int max_payload, const int32_t *pairs, int ncodes,
                                      const int32_t *code_of, int nstreams, fec_mw_relay_streams **out);
/* The number of pairs of a group (1 for fec_mw_relay_streams_create's, whose strides are its own
 * sizes) and its row strides: the least cw1_stride and the output rows' (any pointer may be NULL). */
int fec_mw_relay_streams_codes(const fec_mw_relay_streams *group, int *ncodes, int *cw1_bytes, int *cw2_stride);
/* Flow `id`'s pair index and that pair's sizes: cw1_bytes = S1*n1, cw2_bytes = S2*n2, delay = T1 (any
 * pointer may be NULL). */
int fec_mw_relay_streams_stream_geometry(const fec_mw_relay_streams *group, int id, int *code, int *k1, int *n1,
                                         int *k2, int *n2, int *cw1_bytes, int *cw2_bytes, int *delay);
/* Makes flow `id` a fresh hop-1 decoder and a fresh hop-2 encoder of pair `code`: seq 0 and a new
 * symbolic decoder on that pair's decode rules.  Host work only (calls already queued carry their own
 * seqs and pairs; the slot's device bytes are not cleared, and the kernels never read a flow's device
 * state from before seq 0).  The old pair's last T1 messages are never forwarded: a caller that wants
 * them keeps the old id alive beside a second id.  On a group made by fec_mw_relay_streams_create only
 * code 0 is accepted, and resets the flow.  FEC_ERR_ARG (group unchanged): id or code out of range. */
int fec_mw_relay_streams_set_code(fec_mw_relay_streams *group, int id, int code);
/* Host only, no device call: per pair the packets per chunk of a burst cut in several and that
 * chunk's LDS bytes (ncodes entries each): entry c is fec_mw_relay_streams_fit of pair c, through the
 * routine create uses.  FEC_ERR_ARG if any pair is refused, ncodes is outside [1, 64] or a pointer is
 * null. */
int fec_mw_relay_streams_mixed_fit(int max_payload, const int32_t *pairs, int ncodes, int32_t *chunk,
                                   int32_t *lds);
/* cw1_bytes = S1*n1, cw2_bytes = S2*n2, delay = T1 (any pointer may be NULL).  A group of one pair;
 * FEC_ERR_ARG for a group of several (fec_mw_relay_streams_stream_geometry answers per flow). */
int fec_mw_relay_streams_geometry(const fec_mw_relay_streams *group, int *cw1_bytes, int *cw2_bytes, int *delay);
int fec_mw_relay_streams_relay(fec_mw_relay_streams *group, const int32_t *ids, const int32_t *counts, int M,
                               const uint8_t *erasure, const uint8_t *d_cw1, int64_t cw1_stride, uint8_t *d_cw2,
                               int32_t *d_cw2_len, uint8_t *d_fate, void *hip_stream);
/* hop-1 packets flow id has been fed so far, and messages forwarded (= max(received - T1, 0), T1 the
 * flow's own) */
int fec_mw_relay_streams_state(const fec_mw_relay_streams *group, int id, int64_t *received, int64_t *forwarded);
/* Host only, no device call: the packets per chunk of a burst cut in several and that chunk's LDS
 * bytes, through the routine create uses.  FEC_ERR_ARG where create would refuse the pair. */
int fec_mw_relay_streams_fit(int max_payload, int T1, int B1, int N1, int T2, int B2, int N2, int *chunk_packets,
                             int *lds_bytes);

/* ---- relay: state-dependent symbol-wise decode-and-forward (SD-SWDF, RELAYING_TYPE 3) --------
 * Decoder_Symbol_Wise::symbol_wise_encode_state_dependent (src/Decoder_Symbol_Wise.cpp:178-432) at
 * the relay and symbol_wise_decode_state_dependent + extract_data (:487-546, :653-661) at the
 * destination, as Variable_Rate_FEC_Decoder drives them with one relay frame per seq
 * (src/Variable_Rate_FEC_Decoder.cpp:636-675, 1458-1493 relay; :1703-1721, 1798-1815 destination),
 * fixed rate, k = T1-N1+1 = T2-N2+1, T2 <= T1 <= T_TOT = 10; sdbo = FLAG_FOR_SDBO (FEC_Macro.h:50
 * ships 0).  The control flow depends only on erasure flags and headers: a host planner replays it
 * per packet (serial, like the reference) and the GPU applies the per-packet plans to the bytes.
 * A batch runs a fresh relay / destination over seqs 0..P-1; both calls return when done.
 *   fec_sdswdf_relay_batch: d_cw P rows of cw_stride bytes (source codewords zero-padded to >= S*n1;
 *     erased rows are never read), h_erasure P hop-1 flags (host) -> d_frames P rows of frame_bytes:
 *     [size BE16][header 11 bytes][codeword_new_vector[n2-1][0..size)], size = (S+1)*n2.
 *   fec_sdswdf_destination_batch: d_frames (rows of frame_bytes; the 11 header bytes of every
 *     received frame steer the decode), h_erasure P hop-2 flags (host) -> d_out P rows of S*k
 *     bytes: row t = data_with_header of source packet t - delay (blocks*k decoded, rest zero);
 *     h_flag (host, may be NULL): 1 when a diagonal had too many erasures (the loss counter).
 *   fec_sdswdf_relay_plan / fec_sdswdf_dest_plan: the host plans alone (tests): per seq a record id,
 *     and the distinct records: relay = header[11] + n2 rows of n1 coefficients (frame symbol i of
 *     block j = sum_p coef[i][p] * symbol (j, p) of source packet t-(n1-1)+p+(k-1-i)); destination
 *     = k rows of n2 coefficients (data symbol s of block j = sum_q coef[s][q] * frame symbol
 *     (j, q) of frame t-s-(n2-1-q)). */
typedef struct fec_sdswdf fec_sdswdf;
int fec_sdswdf_create(int max_payload, int T1, int N1, int T2, int N2, int sdbo, fec_sdswdf **out);
int fec_sdswdf_destroy(fec_sdswdf *w);
/* Host-only (no device call): whether a type-3 batch of this geometry runs on the tile kernel
 * (1) or the per-(packet, block) kernel (0), the tile's packets and its dynamic LDS bytes; stride <=
 * 0 = the default row pitch (relay: S*n1, destination: the frame bytes). */
int fec_sdswdf_tile_geometry(int relay, int max_payload, int T1, int N1, int T2, int N2, int64_t stride,
                             int *tile_packets, int *lds_bytes);
int fec_sdswdf_geometry(const fec_sdswdf *w, int *k, int *n1, int *n2, int *S, int *blocks,
                        int *frame_bytes, int *delay);
int fec_sdswdf_relay_batch(fec_sdswdf *w, const uint8_t *d_cw, int64_t cw_stride, const uint8_t *h_erasure,
                           int64_t P, uint8_t *d_frames, void *hip_stream);
int fec_sdswdf_destination_batch(fec_sdswdf *w, const uint8_t *d_frames, const uint8_t *h_erasure, int64_t P,
                                 uint8_t *d_out, uint8_t *h_flag, void *hip_stream);
/* The same over several independent streams laid end to end (fec_relay_vr): a fresh relay /
 * destination takes over at each row of h_starts (sorted); the rows in front of a start that its
 * plans reach must be zero codewords / frames on received (0) flags, as before a stream's seq 0. */
int fec_sdswdf_relay_batch_starts(fec_sdswdf *w, const uint8_t *d_cw, int64_t cw_stride, const uint8_t *h_erasure,
                                  int64_t P, const int64_t *h_starts, int nstarts, uint8_t *d_frames,
                                  void *hip_stream);
int fec_sdswdf_destination_batch_starts(fec_sdswdf *w, const uint8_t *d_frames, const uint8_t *h_erasure,
                                        int64_t P, const int64_t *h_starts, int nstarts, uint8_t *d_out,
                                        uint8_t *h_flag, void *hip_stream);
int fec_sdswdf_relay_plan(fec_sdswdf *w, const uint8_t *h_erasure, int64_t P, int32_t *h_plan,
                          uint8_t *h_records, int64_t records_cap, int64_t *n_records, int *record_bytes);
int fec_sdswdf_dest_plan(fec_sdswdf *w, const uint8_t *h_erasure, const uint8_t *h_headers, int64_t P,
                         int32_t *h_plan, uint8_t *h_flag, uint8_t *h_records, int64_t records_cap,
                         int64_t *n_records, int *record_bytes);

/* ---- relay under variable rate: RELAYING_TYPE 2 / 3 through code switches ---------------------
 * The relay chain of Variable_Rate_FEC_Decoder under a schedule of source codes (:600-740 relay,
 * :1423-1600 and :1772-1873 destination): at a switch to (T, N) at seq s the relay and the
 * destination create fresh Decoder_Symbol_Wise objects for it; for the T_TOT + 1 double-coded seqs
 * s .. s + T_TOT (Variable_Rate_FEC_Encoder.cpp:74-235) the old objects take the old code's
 * codewords and the new ones the new code's, the relay sends [BE16 size_cur][new part][old part]
 * (part = [header 11 bytes, type 3][codeword_new_vector row of size = (S+1)*n2 bytes]), the
 * destination's old object reports; at s + T_TOT + 1 the new objects take over (copy_elements).
 * Hop 1 carries FEC_Encoder(max_payload, T, N, N) codewords, hop 2 the relay's (T, N) re-encoding
 * (T2 = T: the relay-mode estimator fixes T = T_TOT, Parameter_Estimator.cpp:72-75).
 *   fec_relay_vr_create: type 2 or 3; sched = nsw entries (seq, T, N), the first at seq 0, each at
 *     least T_TOT + 1 = 11 after the previous, 1 <= T <= 10, N <= T; P seqs.
 *   fec_relay_vr_run: d_payload P rows of max_payload bytes (source packet t), h_e1 / h_e2 P hop-1 /
 *     hop-2 erasure flags (host) -> d_frames P rows of frame_stride bytes and d_frame_len P sizes
 *     (the relay's frame per seq), d_out P rows of out_stride bytes (what the reporting destination
 *     object's extract_data wrote at seq t: blocks*k bytes of its code, zero after), h_flag P (host,
 *     may be NULL): the reporting object's loss flag.  Returns when done. */
typedef struct fec_relay_vr fec_relay_vr;
int fec_relay_vr_create(int type, int max_payload, const int32_t *sched, int nsw, int64_t P, fec_relay_vr **out);
int fec_relay_vr_destroy(fec_relay_vr *r);
int fec_relay_vr_geometry(const fec_relay_vr *r, int *frame_stride, int *out_stride, int *codes);
int fec_relay_vr_run(fec_relay_vr *r, const uint8_t *d_payload, const uint8_t *h_e1, const uint8_t *h_e2,
                     uint8_t *d_frames, int32_t *d_frame_len, uint8_t *d_out, uint8_t *h_flag, void *hip_stream);

/* ---- the two-hop adaptive relay session (RELAYING_TYPE 2 / 3, N_INITIAL = N_INITIAL_2 = -1) -------
 * application_local_simulation.cpp:71-593 with FLAG_FOR_CONSTANT_TRANS = 1, replacing the loop of
 * Application_Layer_Sender::generate_message_and_encode (:64-282: the 12-byte feedback, the split
 * T = T_TOT - N2, T2 = T_TOT - N), Variable_Rate_FEC_Encoder::encode in relay mode
 * (Variable_Rate_FEC_Encoder.cpp:74-235), Application_Layer_Receiver::receive_message_and_symbol_
 * wise_encode / _decode (Application_Layer_Receiver.cpp:56-319, the relay-mode estimators,
 * Parameter_Estimator.cpp:72-75), Variable_Rate_FEC_Decoder's relay and destination paths
 * (Variable_Rate_FEC_Decoder.cpp:542-1879) and send_sym_wise_message (Application_Layer_Sender.cpp:
 * 284-346).  The control flow runs on the host at create (it depends on the hop erasure patterns
 * only); run does the byte work of the whole session on the GPU.
 *   fec_relay_session_create: relay_type 2 or 3, Q seqs (the reference's loop runs to seq
 *     NUMBER_OF_ITERATIONS + T_TOT + T2 - 1), hop patterns e1 / e2 (received past their end; e1[0]
 *     must be 0).
 *   fec_relay_session_info: stats[16] = {Q, relay_bytes, source switches, relay switches,
 *     destination switches, destination flags, relay calls, lineages, destination outputs,
 *     processed seqs, symbol bytes, encoder instances, longest lineage, relay flags, rate1 count,
 *     rate2 count}; rates[4] = {sum of first-hop rates, of second-hop rates, of min rates, control
 *     plane ms} (the reference's float sums, in its order).
 *   fec_relay_session_relay_offsets: off[Q+1], relay packet t at d_relay[off[t], off[t+1]).
 *   fec_relay_session_hop1_headers: hdr[Q][16], the source's packet headers (:222-244).
 *   fec_relay_session_dest_meta: proc[Q] (1 = the destination's main object extracted an output at
 *     seq t), flag[Q] (its decode flag).
 *   fec_relay_session_run: d_payload Q rows of max_payload bytes (source packet t) -> d_relay
 *     (relay_bytes: every relay packet, 8-byte header + word), d_dest_out Q rows of 320 bytes (the
 *     extracted data_with_header of packet t - T_TOT, zero where not processed), d_dest_lost Q
 *     (calc_missed_chars, Variable_Rate_FEC_Decoder.cpp:2698-2792), *d_lost their count; async on
 *     the stream.
 *   fec_relay_session_hop1: after a run, the source's wire packets (16-byte header + VR frame) at
 *     `stride`, zero padded, sizes in d_len. */
typedef struct fec_relay_session fec_relay_session;
int fec_relay_session_create(int relay_type, int max_payload, int64_t Q, const uint8_t *e1, int64_t n_e1,
                             const uint8_t *e2, int64_t n_e2, fec_relay_session **out);
int fec_relay_session_destroy(fec_relay_session *h);
int fec_relay_session_info(const fec_relay_session *h, int64_t *stats, double *rates);
int fec_relay_session_relay_offsets(const fec_relay_session *h, int64_t *off);
int fec_relay_session_hop1_headers(const fec_relay_session *h, uint8_t *hdr);
int fec_relay_session_dest_meta(const fec_relay_session *h, uint8_t *proc, uint8_t *flag);
int fec_relay_session_run(fec_relay_session *h, const uint8_t *d_payload, uint8_t *d_relay, uint8_t *d_dest_out,
                          uint8_t *d_dest_lost, int64_t *d_lost, void *hip_stream);
int fec_relay_session_hop1(fec_relay_session *h, uint8_t *d_packets, int64_t stride, int32_t *d_len,
                           void *hip_stream);

/* ---- relay per call: the Decoder_Symbol_Wise methods on caller-held state ---------------------
 * What siphon::Decoder_Symbol_Wise (fec_amd_dropin.h) calls: one reference method call each, on
 * the arrays the reference's callers fill (Variable_Rate_FEC_Decoder.cpp:950-1879).  The control
 * flow runs on the host over the flags and headers; the GF work of all the packet's code blocks is
 * one GPU launch (its inputs packed into pinned staging, results back), then the call returns.
 *   fec_sw_state_encode  = symbol_wise_encode_state_dependent (Decoder_Symbol_Wise.cpp:178-432):
 *     slots = codeword_vector_state_dependent [30] (packet at offset 2), er = its flags [30],
 *     header [30] rows of 11 ints (row n2-1 written), cnv = codeword_new_vector[n2-1], cnsw =
 *     codeword_new_symbol_wise;
 *   fec_sw_state_decode  = symbol_wise_decode_state_dependent (:487-546) into buffer, *flag;
 *   fec_sw_encode_1      = symbol_wise_encode_1 (:547-619): cv = codeword_vector [T_TOT+1], er =
 *     temp_erasure_vector, cnv = codeword_new_vector [T_TOT+1] (row n2-1 written);
 *   fec_sw_decode_1      = symbol_wise_decode_1 (:621-651) into buffer, *flag.
 * k2 == k; n <= 11 (types 3) / n <= 17 (type 2); sdbo = FLAG_FOR_SDBO. */
int fec_sw_state_encode(int max_payload, int k, int n, int k2, int n2, int sdbo, uint8_t *const *slots,
                        const uint8_t *er, int *const *header, uint8_t *cnv, uint8_t *cnsw);
int fec_sw_state_decode(int max_payload, int k, int n, uint8_t *const *slots, int *const *header, uint8_t *buffer,
                        int *flag);
int fec_sw_encode_1(int max_payload, int k, int n, int k2, int n2, uint8_t *const *cv, const uint8_t *er,
                    uint8_t *const *cnv, uint8_t *cnsw, int *flag);
int fec_sw_decode_1(int max_payload, int k, int n, uint8_t *const *cv, const uint8_t *er, uint8_t *buffer,
                    int *flag);

/* ---- erasure patterns (inputs of the decode path; host only, no device needed) ---------------
 * Byte-exact restatements of Erasure_File_Generator (src/Erasure_File_Generator.cpp:25-287): out[i]
 * = 1 if packet i is erased.  Same engine (mt19937), same draw order and the same libstdc++
 * uniform_real_distribution<double> arithmetic as the reference; probabilities are float as in
 * its signatures.  The reference writes these bytes to erasure.bin (read back by
 * Erasure_Simulator, src/Erasure_Simulator.cpp:13-30). */
/* generate_IID (:25-63); seed 0 = SEED_ARTIFICIAL_ERASURE */
int fec_erasure_iid(uint8_t *out, int count, float erasure_prob, int seed);
/* generate_three_sections_IID (:65-121) */
int fec_erasure_three_sections_iid(uint8_t *out, int count1, float prob1, int count2, float prob2,
                                   int count3, float prob3, int seed);
/* generate_GE (:123-170) / generate_GE_varying (:172-213); good_state: the generator object's
 * state carried across calls (in/out, NULL = a fresh object, i.e. good) */
int fec_erasure_ge(uint8_t *out, int count, float alpha, float beta, float erasure_prob, int seed,
                   int *good_state);
int fec_erasure_ge_varying(uint8_t *out, int count, float alpha, float beta, float erasure_prob,
                           int seed, int *good_state);
/* generate_Fritchman_varying (:215-264) */
int fec_erasure_fritchman_varying(uint8_t *out, int count, float alpha, float beta,
                                  float erasure_prob, int number_of_states, int seed);
/* generate_periodic (:266-287) */
int fec_erasure_periodic(uint8_t *out, int count, int T, int B, int N);

/* ---- utility (tests / bench only, not on the coding path) ---------------------------------
 * Synthetic payloads: byte b of packet t0+p = low 8 bits of splitmix64(seed ^ ((t0+p)*L + b)). */
int fec_util_fill_payload(uint8_t *d_out, int64_t t0, int64_t count, int L, uint64_t seed,
                          void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
