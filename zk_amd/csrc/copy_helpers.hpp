// copy_helpers.hpp -- the few host threads that copy a serialised table out of pinned staging (zk_mle_to_bytes, zk_cmle_to_bytes,
// zk_mle_upload_shard).
#pragma once
#include <sched.h>
#include <stdint.h>

#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "env.hpp"

// chunk -> caller's buffer on a few host threads: a fresh destination (a new Vec<u8>) is page-fault bound, and faults parallelise.
// The helpers live for ONE zk_mle_to_bytes call (started once, handed every chunk, joined at its end), never more than three of
// them; their number follows the CPUs this process may run on (sched_getaffinity, so cgroup / taskset limits count), and
// ZK_TO_BYTES_THREADS (1..4; 1 = the caller's thread only) overrides it.  zk_mle_upload_shard gathers its shard with the same
// helpers (stride > 1: destination element i is source element i * stride).
class CopyHelpers {
  public:
    explicit CopyHelpers(size_t total_bytes) {
        static const unsigned from_env = (unsigned)env_u64("ZK_TO_BYTES_THREADS", 0, 1, 4);   // 0: not set
        unsigned nt = from_env;
        if (!nt) {
            cpu_set_t set;
            CPU_ZERO(&set);
            nt = sched_getaffinity(0, sizeof set, &set) == 0 ? (unsigned)CPU_COUNT(&set) : 1u;
            if (nt > 4) nt = 4;
        }
        if (nt < 2 || total_bytes < 2 * kMinPerThread) return;
        for (unsigned i = 1; i < nt; ++i) {
            try {
                th_.emplace_back([this, i] { work(i); });
            } catch (...) {
                break;   // no thread to be had: the ones that started (perhaps none) share the work
            }
        }
    }
    ~CopyHelpers() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    CopyHelpers(const CopyHelpers &) = delete;
    CopyHelpers &operator=(const CopyHelpers &) = delete;
    // bytes of the destination (a multiple of 32 when stride > 1)
    void copy(uint8_t *dst, const uint8_t *src, size_t bytes, size_t stride = 1) {
        const unsigned parts = (unsigned)th_.size() + 1;
        if (parts < 2 || bytes < 2 * kMinPerThread) {
            copy_part(dst, src, bytes, stride);
            return;
        }
        const size_t per = (bytes / parts + 4095) & ~(size_t)4095;
        {
            std::lock_guard<std::mutex> lk(mu_);
            dst_ = dst, src_ = src, bytes_ = bytes, per_ = per, stride_ = stride;
            pending_ = parts - 1;
            ++generation_;
        }
        cv_.notify_all();
        copy_part(dst, src, per < bytes ? per : bytes, stride);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
    }

  private:
    static constexpr size_t kMinPerThread = (size_t)2 << 20;
    static void copy_part(uint8_t *dst, const uint8_t *src, size_t bytes, size_t stride) {
        if (stride == 1) {
            memcpy(dst, src, bytes);
            return;
        }
        for (size_t i = 0; i < bytes; i += 32) memcpy(dst + i, src + i * stride, 32);
    }
    void work(unsigned part) {
        uint64_t seen = 0;
        for (;;) {
            uint8_t *dst;
            const uint8_t *src;
            size_t bytes, per, stride;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                dst = dst_, src = src_, bytes = bytes_, per = per_, stride = stride_;
            }
            const size_t off = per * part;
            if (off < bytes) copy_part(dst + off, src + off * stride, bytes - off < per ? bytes - off : per, stride);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    uint8_t *dst_ = nullptr;
    const uint8_t *src_ = nullptr;
    size_t bytes_ = 0, per_ = 0, stride_ = 1;
    unsigned pending_ = 0;
    uint64_t generation_ = 0;
    bool stop_ = false;
};
