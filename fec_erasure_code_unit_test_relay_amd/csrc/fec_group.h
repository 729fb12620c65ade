// fec_group.h -- what a stream group's call does around its launch, the same for every group
// (fec_streams.hip, fec_relay_streams.hip, fec_mw_relay_streams.hip): the staging ring of a call's
// records with the ordering rule of a call (GroupStage, StageGuard), the kernels' dynamic-LDS limit
// (lds_allow) and the checks and constants the groups share.  Host code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "fec_amd.h"
#include "fec_status.h"

namespace fec {

constexpr int kCuLds = 160 * 1024;  // dynamic LDS a group's kernel may take (a CU's whole LDS)
constexpr int kChunkTP = 32;        // packets per chunk, LDS permitting (at least the packets a chunk needs in front)
constexpr size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

// A call's records (chunks, row flags or masks, coefficient blocks) go through a ring of kBufs pinned,
// mapped staging buffers that the kernels read in place, so the host prepares a call (the decoders'
// symbolic steps) while the GPU still runs the ones before it.  A call goes
//     check (arguments; check_ids) -> begin -> StageGuard -> reserve, fill -> launch -> commit
// and the group's per-stream counters advance after commit.
struct GroupStage {
    static constexpr int kBufs = 4;
    void* h_buf[kBufs] = {};         // pinned records
    void* d_buf[kBufs] = {};         // their device addresses
    size_t cap[kBufs] = {};          // bytes of h_buf[b] (a large call grows its buffer to its records)
    hipEvent_t staged[kBufs] = {};   // the last kernel that read h_buf[b]
    hipEvent_t done = nullptr;       // the last call's kernel (the group's windows and rings)
    int buf = 0;                     // the next call's buffer
    bool open = false;               // between begin and commit
    bool poisoned = false;           // a failed call left host and device state apart: every later call is refused
    std::vector<uint32_t> mark;      // duplicate-id check (call stamp per stream)
    uint32_t stamp = 0;

    GroupStage() = default;
    GroupStage(const GroupStage&) = delete;
    GroupStage& operator=(const GroupStage&) = delete;
    ~GroupStage() {
        for (hipEvent_t e : staged)
            if (e) (void)hipEventDestroy(e);
        if (done) (void)hipEventDestroy(done);
        for (void* p : h_buf)
            if (p) (void)hipHostFree(p);
    }

    // Buffers of `bytes` each for a group of nstreams streams; the events start out recorded.
    int init(int nstreams, size_t bytes) {
        mark.assign(nstreams, 0);
        for (int b = 0; b < kBufs; ++b) {
            if (int st = grow(b, bytes)) return st;
            FEC_HIP(hipEventCreateWithFlags(&staged[b], hipEventDisableTiming));
            FEC_HIP(hipEventRecord(staged[b], nullptr));
        }
        FEC_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
        FEC_HIP(hipEventRecord(done, nullptr));
        return FEC_OK;
    }

    // ids distinct and in range (an argument check: it changes nothing but the stamp)
    int check_ids(const int32_t* ids, int M) {
        if (++stamp == 0) {
            std::fill(mark.begin(), mark.end(), 0u);
            stamp = 1;
        }
        const int nstreams = static_cast<int>(mark.size());
        for (int m = 0; m < M; ++m) {
            const int id = ids[m];
            if (id < 0 || id >= nstreams || mark[id] == stamp) return FEC_ERR_ARG;
            mark[id] = stamp;
        }
        return FEC_OK;
    }

    // This call's staging buffer, h_buf[buf]: a buffer is rewritten only after the kernel that read it
    // (host wait on that call's kernel, kBufs calls back), and the previous call's kernel -- which read
    // and wrote the windows and rings, after every older kernel -- comes before anything this call
    // enqueues on `s`, whichever stream the previous call used (device-side wait).
    int begin(hipStream_t s) {
        if (poisoned) return FEC_ERR_HIP;
        FEC_HIP(hipEventSynchronize(staged[buf]));
        FEC_HIP(hipStreamWaitEvent(s, done, 0));
        open = true;
        return FEC_OK;
    }

    // The call's buffer holds at least `bytes` (its old contents are not kept).
    int reserve(size_t bytes) { return bytes <= cap[buf] ? FEC_OK : grow(buf, std::max(bytes, 2 * cap[buf])); }
    uint8_t* host() const { return static_cast<uint8_t*>(h_buf[buf]); }
    const uint8_t* device() const { return static_cast<const uint8_t*>(d_buf[buf]); }

    // After the launch on `s`: the call's kernel is the group's last and its buffer's last reader.
    int commit(hipStream_t s) {
        FEC_HIP(hipGetLastError());
        FEC_HIP(hipEventRecord(done, s));
        FEC_HIP(hipEventRecord(staged[buf], s));
        buf = (buf + 1) % kBufs;
        open = false;
        return FEC_OK;
    }

private:
    int grow(int b, size_t bytes) {
        if (h_buf[b]) FEC_HIP(hipHostFree(h_buf[b]));
        h_buf[b] = nullptr;
        d_buf[b] = nullptr;
        cap[b] = 0;
        FEC_HIP(hipHostMalloc(&h_buf[b], bytes, hipHostMallocMapped));
        FEC_HIP(hipHostGetDevicePointer(&d_buf[b], h_buf[b], 0));
        cap[b] = bytes;
        return FEC_OK;
    }
};

// Declared right after begin: a call that leaves before commit (a failed HIP call, a failed symbolic
// step) may have its host state ahead of the device's, its buffer gone or its events unrecorded, so
// the group is poisoned.
struct StageGuard {
    GroupStage& st;
    ~StageGuard() {
        if (st.open) st.poisoned = true;
        st.open = false;
    }
};

// A launch with more than 64 KB of dynamic LDS needs the kernel's limit raised first, once per size:
// *raised is the kernel's high-water mark, one per kernel and process (a static of the caller).
inline int lds_allow(const void* kernel, int lds, int* raised) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (lds <= 64 * 1024 || lds <= *raised) return FEC_OK;
    FEC_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    *raised = lds;
    return FEC_OK;
}

// counts all >= 1 (null: M counts of 1); their sum and largest
inline int check_counts(const int32_t* counts, int M, int64_t* R, int* maxc) {
    *R = counts ? 0 : M;
    *maxc = counts ? 0 : 1;
    for (int m = 0; counts && m < M; ++m) {
        if (counts[m] < 1) return FEC_ERR_ARG;
        *R += counts[m];
        *maxc = std::max(*maxc, counts[m]);
    }
    return FEC_OK;
}

}  // namespace fec
