// fec_burst.h -- what the burst kernels of the stream groups share (fec_streams.hip, fec_mw_relay_streams.hip):
// a chunk's unit record, the decode row flags, exact division by a multiply, the fork-join pool for
// the symbolic steps of a large call and the symbolic half of a burst (plan_burst_rows).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

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

}  // namespace
