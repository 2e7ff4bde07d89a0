// The host thread pool of the batched front end and the plan that shares a
// node's CPUs among its ranks. Pure host code (no HIP): tools/pool_check.cpp
// builds it stand-alone, under a sanitizer.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace svo {

// SVO_POOL_SPIN_US (default 400 us)
double pool_spin_env();

// Persistent pool for the per-sequence host work (RANSAC hypotheses, pose fits).
// It runs a couple of times per step, microseconds apart: workers busy-poll a
// generation counter for a while after each job (spin_us, SVO_POOL_SPIN_US)
// before sleeping on a condition variable, so a dispatch normally costs no
// futex wake-up. The caller works too and spins on a counter of finished TASKS
// (a worker that wakes late with nothing left to take is not waited for).
// Tasks are claimed by CAS on one word holding (generation, task count, next
// index): a worker still holding a word of an older job -- generation AND count
// -- can never take (or skip) a task of a newer one, whatever the sizes of the
// two jobs (the count is not read from a second variable that a newer job may
// already have rewritten).
// Workers are pinned to `cpus` (the rank's share of the node, svo_host_cpu_plan)
// when it is non-empty. The spin is bounded below one step (SVO_POOL_SPIN_US,
// default 400 us): between the step's two pool jobs the workers stay hot, across
// an idle caller they sleep, so a rank does not burn its cores between steps.
class Pool {
   public:
    explicit Pool(int n, const std::vector<int>& cpus = {}, double spin_us = pool_spin_env());
    ~Pool();
    int size() const { return (int)th_.size(); }
    // a job without tasks: sleeping workers wake and every worker starts a new
    // spin window, so a job expected shortly finds them hot (no futex wake-up)
    void prime() {
        if (th_.empty()) return;
        publish(0);
    }
    void run(int n, const std::function<void(int)>& fn);

   private:
    // job word: generation (24 bits) | task count (20) | next index (20)
    static constexpr int kFieldBits = 20;
    static constexpr uint64_t kFieldMask = (1ull << kFieldBits) - 1;
    static constexpr uint64_t kGenMask = (1ull << (64 - 2 * kFieldBits)) - 1;
    static uint64_t gen_of(uint64_t v) { return v >> (2 * kFieldBits); }
    static uint64_t cnt_of(uint64_t v) { return (v >> kFieldBits) & kFieldMask; }
    static uint64_t idx_of(uint64_t v) { return v & kFieldMask; }
    uint64_t publish(int n);
    void work(uint64_t g);
    void loop();
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_;
    const std::function<void(int)>* fn_ = nullptr;
    std::atomic<uint64_t> next_{0}, gen_{0};
    std::atomic<int> done_{0}, sleeping_{0};
    std::atomic<bool> stop_{false};
    double spin_us_ = 400.0;
};

// This rank's share of the CPUs the process may run on (svo_host_cpu_plan):
// the CPUs of its GPU's NUMA node split among the ranks on that node when
// gpu_node[world] is given and the node has enough of them, an even split of
// all allowed CPUs otherwise.
std::vector<int> host_cpu_plan(int rank, int world, const int* gpu_node);

}  // namespace svo
