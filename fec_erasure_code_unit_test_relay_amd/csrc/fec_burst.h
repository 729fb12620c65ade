// fec_burst.h -- what the burst kernels of the stream groups share (fec_streams.hip, fec_mw_relay_streams.hip):
// a chunk's unit record, the decode row flags, exact division by a multiply, the tuples the stream
// kernels take (stream_tuple), the fork-join pool for the symbolic steps of a large call, the symbolic
// half of a burst (plan_burst_rows) and of a whole decode call (DecodePlan).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

#include "fec_group.h"
#include "fec_host.h"

namespace fec {
namespace {

constexpr int kRR = 64;  // decoder ring rows per stream (>= T + k, the per-packet decoder's)

__device__ __forceinline__ uint8_t gmul(const uint8_t* gexp, const uint8_t* glog, uint8_t a, uint8_t b) {
    return (a && b) ? gexp[glog[a] + glog[b]] : 0;
}

struct FastDiv {  // x / d by one multiply, exact while x * d < 2^32
    uint32_t m, d;
};
inline FastDiv fast_div(int d) {
    return FastDiv{d > 1 ? static_cast<uint32_t>(((1ull << 32) + d - 1) / d) : 0u, static_cast<uint32_t>(d)};
}
__device__ __forceinline__ int fdiv(FastDiv f, int x) {
    return f.d == 1 ? x : static_cast<int>(__umulhi(static_cast<uint32_t>(x), f.m));
}

struct BurstUnit {   // one chunk = one workgroup
    int64_t row0;    // its first row in the call's row arrays
    int64_t seq0;    // that row's sequence number in its stream
    int64_t coef;    // decode: byte offset of the chunk's first coefficient block (its recovered rows, in row order)
    int32_t id;
    int32_t cnt;     // rows of the chunk (<= the code's TP)
    int32_t lead;    // rows of the burst in front of the chunk (0: the first chunk)
    int32_t total;   // rows of the burst
    int32_t code;    // index in the mixed kernels' table (0 in a one-code group)
    int32_t pad;
};
constexpr uint8_t kRowClamp = 4, kRowErased = 8;  // decode row flags: fate | clamp | erased

// One code (T,B,N) of a stream group at payload size L: false for a tuple that fec_codec_create or the
// stream kernels (ring rows, registers, LDS tables) refuse.
inline bool stream_tuple(int L, int T, int B, int N, Geometry* g) {
    try {
        *g = Geometry::make(L, T, B, N);
    } catch (const std::invalid_argument&) {
        return false;
    }
    if (g->L > 1500 || g->B < g->N || g->n > kMaxN - 1) return false;
    return g->T + g->k <= kRR && g->k <= 16 && g->k * g->n <= 16 * 32;
}

}  // namespace
}  // namespace fec

namespace {
// Fork-join pool for the decoders' symbolic steps of one call: the streams are independent, so the
// call's items are cut into contiguous parts, one per thread (the calling thread takes part 0).  A
// worker polls for the next job for a while (calls come back to back) before it sleeps: a sleeping
// thread's wake-up costs tens of microseconds, as much as its share of the steps.
// The workers run on the 8 CPUs of the creating thread's aligned group (within the allowed set):
// on a two-socket box the scheduler otherwise spreads them over both sockets (FEC_STREAMS_PIN=0:
// unplaced).
// A group with fewer than 4 allowed CPUs (a sparse cpuset: taskset, cgroup) is left alone: spin-
// polling workers crowded on one or two CPUs stall each other for milliseconds.
void place_near(int home) {
    if (home < 0) return;
    cpu_set_t allowed, set;
    CPU_ZERO(&set);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return;
    const int base = home & ~7;
    for (int c = base; c < base + 8 && c < CPU_SETSIZE; ++c)
        if (CPU_ISSET(c, &allowed)) CPU_SET(c, &set);
    if (CPU_COUNT(&set) >= 4) (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
}
// CPUs this process may run on (its affinity mask), at least 1.
int allowed_cpus() {
    cpu_set_t allowed;
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return static_cast<int>(std::thread::hardware_concurrency());
    return std::max(1, CPU_COUNT(&allowed));
}

class StepPool {
public:
    explicit StepPool(int threads) {
        const char* pin = std::getenv("FEC_STREAMS_PIN");
        const int home = (pin && std::atoi(pin) == 0) ? -1 : sched_getcpu();
        for (int i = 1; i < threads; ++i) th_.emplace_back([this, i, home] {
            place_near(home);
            loop(i);
        });
    }
    ~StepPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_.store(true);
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    int parts() const { return static_cast<int>(th_.size()) + 1; }
    // f(part) for every part; returns after all of them
    void run(const std::function<void(int)>& f) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f;
            left_.store(static_cast<int>(th_.size()), std::memory_order_relaxed);
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        f(0);
        while (left_.load(std::memory_order_acquire) > 0) __builtin_ia32_pause();
    }

private:
    void loop(int i) {
        uint64_t seen = 0;
        for (;;) {
            // poll up to ~0.2 ms for the next job, then sleep
            const auto t0 = std::chrono::steady_clock::now();
            for (int spin = 0; gen_.load(std::memory_order_acquire) == seen && !stop_.load(); ++spin) {
                __builtin_ia32_pause();
                if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
            }
            const std::function<void(int)>* f;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_.load() || gen_.load() != seen; });
                if (stop_.load()) return;
                seen = gen_.load();
                f = job_;
            }
            (*f)(i);
            left_.fetch_sub(1, std::memory_order_release);
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_;
    const std::function<void(int)>* job_ = nullptr;
    std::atomic<uint64_t> gen_{0};
    std::atomic<bool> stop_{false};
    std::atomic<int> left_{0};
};

constexpr int kPoolMinItems = 1024;  // items per part below which a call steps on one thread

// A group's pool (FEC_STREAMS_THREADS threads, default min(allowed CPUs - 1, 8)); null for a group too
// small to ever fill two parts, or with one thread.
std::unique_ptr<StepPool> make_step_pool(int nstreams) {
    const int hw = allowed_cpus();  // not hardware_concurrency: the process's cpuset may be smaller
    int nth = std::max(1, std::min(hw > 1 ? hw - 1 : 1, 8));
    if (const char* e = std::getenv("FEC_STREAMS_THREADS")) nth = std::max(1, std::atoi(e));
    return std::unique_ptr<StepPool>(nth > 1 && nstreams >= 2 * kPoolMinItems ? new StepPool(nth) : nullptr);
}

// The symbolic half of a burst for one stream: packets seq0 .. seq0 + count - 1 with erasure flags
// er[]; one flag byte per row (the fate of packet seq - T | kRowClamp | kRowErased) and the k x n
// blocks of the recovered rows, appended in row order.  A run of received packets on the fast path
// is one skip_received, not a step each.
void plan_burst_rows(fec::StreamPlanner& pl, int T, int kn, int64_t seq0, const uint8_t* er, int64_t count,
                          uint8_t* flags, std::vector<uint8_t>& coefs) {
    int64_t t = 0;
    while (t < count) {
        const int64_t seq = seq0 + t;
        if (!er[t] && pl.fast_at(seq)) {
            int64_t e = t + 1;
            while (e < count && !er[e]) ++e;
            pl.skip_received(seq, e - t);
            for (int64_t i = t; i < e; ++i) flags[i] = seq0 + i >= T ? fec::kCopy : fec::kNone;
            t = e;
            continue;
        }
        const fec::StepResult r = pl.step(seq, er[t] != 0);
        flags[t] = static_cast<uint8_t>(r.fate | (r.slow ? fec::kRowClamp : 0) | (er[t] ? fec::kRowErased : 0));
        if (r.fate == fec::kRecovered) coefs.insert(coefs.end(), r.coef, r.coef + kn);
        ++t;
    }
}

// The symbolic half of a decode call of M streams with R rows in all, and its records as the kernels
// read them.  Streams are independent: contiguous parts of them, one per thread of the pool (a call of
// fewer than 2 * kPoolMinItems rows: one part); a part's recovered rows keep their coefficient blocks
// in row order, and a part's blocks follow those of the parts before it.
template <class Unit>
struct DecodePlan {
    std::vector<Unit> units;
    std::vector<uint8_t> flags;
    std::vector<std::vector<uint8_t>> coefs;  // per part
    size_t off_flags = 0, off_coef = 0, bytes = 0;  // staging: units | row flags | coefficient blocks

    // tp(m): the chunk size of the call's m-th stream.  stream(m, row0, cnt, units, flags, coefs) plans
    // that stream's cnt rows (plan_burst_rows), which start at row row0 of the call, appending to coefs,
    // and fills its (cnt + tp - 1) / tp units, their coefficient offsets counted in coefs.
    // rebase(unit, by) moves a unit's coefficient offsets by `by` bytes.  False: a step failed.
    template <class Tp, class Stream, class Rebase>
    bool plan(StepPool* pool, const int32_t* counts, int M, int64_t R, Tp tp, Stream stream, Rebase rebase) {
        // (the pool calls every one of its parts: a call with fewer streams than parts leaves some empty)
        const int np = (pool && R >= 2 * kPoolMinItems) ? pool->parts() : 1;
        std::vector<int64_t> row_at(M + 1, 0), unit_at(M + 1, 0);
        for (int m = 0; m < M; ++m) {
            const int cnt = counts ? counts[m] : 1, t = tp(m);
            row_at[m + 1] = row_at[m] + cnt;
            unit_at[m + 1] = unit_at[m] + (cnt + t - 1) / t;
        }
        flags.resize(static_cast<size_t>(R));
        units.resize(static_cast<size_t>(unit_at[M]));
        coefs.resize(np);
        auto first = [&](int p) { return static_cast<int>(static_cast<int64_t>(M) * p / np); };
        std::atomic<bool> failed{false};
        auto part = [&](int p) {
            if (p < 0 || p >= np) return;
            try {
                for (int m = first(p); m < first(p + 1); ++m)
                    stream(m, row_at[m], counts ? counts[m] : 1, units.data() + unit_at[m], flags.data() + row_at[m],
                           coefs[p]);
            } catch (...) {
                failed.store(true);
            }
        };
        if (np > 1)
            pool->run(part);
        else
            part(0);
        if (failed.load()) return false;
        int64_t cbase = 0;
        for (int p = 0; p < np; ++p) {
            if (cbase)
                for (int64_t ui = unit_at[first(p)]; ui < unit_at[first(p + 1)]; ++ui) rebase(units[ui], cbase);
            cbase += static_cast<int64_t>(coefs[p].size());
        }
        off_flags = fec::align16(units.size() * sizeof(Unit));
        off_coef = fec::align16(off_flags + flags.size());
        bytes = off_coef + static_cast<size_t>(cbase) + 16;
        return true;
    }

    // The records into a staging buffer of at least `bytes`.
    void write(uint8_t* hs) const {
        std::memcpy(hs, units.data(), units.size() * sizeof(Unit));
        std::memcpy(hs + off_flags, flags.data(), flags.size());
        uint8_t* c = hs + off_coef;
        for (const auto& part : coefs) {
            if (!part.empty()) std::memcpy(c, part.data(), part.size());
            c += part.size();
        }
    }
};

}  // namespace
