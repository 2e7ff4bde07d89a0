// Host thread pool + host core plan (host_pool.hpp); svo_pool_selftest and
// svo_host_cpu_plan of the C ABI.
#include "host_pool.hpp"

#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "svo_gpu.h"

namespace svo {

double pool_spin_env() {
    const char* e = std::getenv("SVO_POOL_SPIN_US");
    return e ? std::atof(e) : 400.0;
}

Pool::Pool(int n, const std::vector<int>& cpus, double spin_us) : spin_us_(spin_us) {
    for (int i = 0; i < n; i++) {
        th_.emplace_back([this] { loop(); });
        if (!cpus.empty()) {
            cpu_set_t set;
            CPU_ZERO(&set);
            for (int c : cpus)
                if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &set);
            (void)pthread_setaffinity_np(th_.back().native_handle(), sizeof(set), &set);
        }
    }
}

Pool::~Pool() {
    {
        std::lock_guard<std::mutex> g(mu_);
        stop_.store(true);
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
}

static void pause() {
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
}

void Pool::run(int n, const std::function<void(int)>& fn) {
    if (th_.empty() || n <= 1 || n > (int)kFieldMask) {
        for (int i = 0; i < n; i++) fn(i);
        return;
    }
    fn_ = &fn;
    done_.store(0, std::memory_order_relaxed);
    const uint64_t g = publish(n);  // the release store of the job word publishes fn_ / done_
    work(g);
    while (done_.load(std::memory_order_acquire) < n) pause();
}

// a new job of n tasks: its word replaces the old one in a single store, so a
// stale CAS (old generation and count) fails from here on
uint64_t Pool::publish(int n) {
    const uint64_t g = (gen_.load(std::memory_order_relaxed) + 1) & kGenMask;
    next_.store((g << (2 * kFieldBits)) | ((uint64_t)n << kFieldBits), std::memory_order_release);
    {
        std::lock_guard<std::mutex> lk(mu_);
        gen_.store(g, std::memory_order_release);
    }
    if (sleeping_.load(std::memory_order_acquire) > 0) cv_.notify_all();
    return g;
}

void Pool::work(uint64_t g) {
    for (;;) {
        uint64_t v = next_.load(std::memory_order_acquire);
        if (gen_of(v) != g || idx_of(v) >= cnt_of(v)) return;
        if (!next_.compare_exchange_weak(v, v + 1, std::memory_order_acq_rel)) continue;
        (*fn_)((int)idx_of(v));
        done_.fetch_add(1, std::memory_order_acq_rel);
    }
}

void Pool::loop() {
    uint64_t seen = 0;
    for (;;) {
        const auto t0 = std::chrono::steady_clock::now();
        int k = 0;
        while (gen_.load(std::memory_order_acquire) == seen && !stop_.load(std::memory_order_relaxed)) {
            pause();
            if (++k == 256) {
                k = 0;
                if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() >
                    spin_us_)
                    break;
            }
        }
        if (gen_.load(std::memory_order_acquire) == seen && !stop_.load()) {
            std::unique_lock<std::mutex> lk(mu_);
            sleeping_.fetch_add(1);
            cv_.wait(lk, [&] { return stop_.load() || gen_.load() != seen; });
            sleeping_.fetch_sub(1);
        }
        if (stop_.load()) return;
        seen = gen_.load(std::memory_order_acquire);
        work(seen);
    }
}

// ---- host core plan (svo_host_cpu_plan) ----
static std::vector<int> parse_cpulist(const std::string& txt) {  // "0-3,8,10-11"
    std::vector<int> out;
    std::stringstream ss(txt);
    std::string tok;
    while (std::getline(ss, tok, ',')) {
        if (tok.empty() || tok[0] == '\n') continue;
        const size_t dash = tok.find('-');
        const int a = std::atoi(tok.c_str());
        const int b = dash == std::string::npos ? a : std::atoi(tok.c_str() + dash + 1);
        for (int c = a; c <= b; c++) out.push_back(c);
    }
    return out;
}

// NUMA node of every CPU id (-1: unknown), from /sys/devices/system/node
static std::vector<int> cpu_nodes(int max_cpu) {
    std::vector<int> node((size_t)max_cpu + 1, -1);
    for (int m = 0; m < 64; m++) {
        std::ifstream f("/sys/devices/system/node/node" + std::to_string(m) + "/cpulist");
        if (!f) continue;
        std::string txt;
        std::getline(f, txt);
        for (int c : parse_cpulist(txt))
            if (c >= 0 && c <= max_cpu) node[c] = m;
    }
    return node;
}

std::vector<int> host_cpu_plan(int rank, int world, const int* gpu_node) {
    cpu_set_t set;
    CPU_ZERO(&set);
    std::vector<int> allowed;
    if (sched_getaffinity(0, sizeof(set), &set) == 0)
        for (int c = 0; c < CPU_SETSIZE; c++)
            if (CPU_ISSET(c, &set)) allowed.push_back(c);
    if (allowed.empty() || world <= 0 || rank < 0 || rank >= world) return {};
    const std::vector<int> node = cpu_nodes(allowed.back());
    std::stable_sort(allowed.begin(), allowed.end(), [&](int a, int b) { return node[a] < node[b]; });
    auto split = [](const std::vector<int>& cpus, int idx, int k) {
        std::vector<int> out;
        const int m = (int)cpus.size();
        if (m == 0 || k <= 0) return out;
        if (m < k) {  // fewer CPUs than ranks: shared, one each
            out.push_back(cpus[idx % m]);
            return out;
        }
        const int lo = (int)((int64_t)m * idx / k), hi = (int)((int64_t)m * (idx + 1) / k);
        out.assign(cpus.begin() + lo, cpus.begin() + hi);
        return out;
    };
    if (gpu_node && gpu_node[rank] >= 0) {
        // the ranks whose GPUs sit on this rank's node share that node's CPUs
        const int my = gpu_node[rank];
        int idx = 0, k = 0;
        for (int r = 0; r < world; r++)
            if (gpu_node[r] == my) {
                if (r < rank) idx++;
                k++;
            }
        std::vector<int> local;
        for (int c : allowed)
            if (node[c] == my) local.push_back(c);
        if ((int)local.size() >= k) return split(local, idx, k);
    }
    return split(allowed, rank, world);
}

}  // namespace svo

using namespace svo;

extern "C" {

int svo_host_cpu_plan(int local_rank, int local_world, const int* gpu_node, int* cpus, int cap, int* n) {
    if (local_world <= 0 || local_rank < 0 || local_rank >= local_world || cap < 0 || (cap > 0 && !cpus))
        return SVO_ERR_ARG;
    const std::vector<int> v = host_cpu_plan(local_rank, local_world, gpu_node);
    for (int i = 0; i < (int)v.size() && i < cap; i++) cpus[i] = v[i];
    if (n) *n = (int)v.size();
    return SVO_OK;
}

int svo_pool_selftest(int threads, int jobs, int64_t* bad) {
    if (threads < 1 || jobs < 1 || !bad) return SVO_ERR_ARG;
    // jobs of alternating, growing and shrinking sizes with primes between them
    // (the front end's pattern: per-hypothesis jobs whose size changes every
    // round): every task of every job must run exactly once, and no task of an
    // older job may run after its job returned
    Pool pool(threads - 1);
    std::vector<std::atomic<int>> hits(4096);
    std::atomic<int64_t> errors{0};
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    for (int j = 0; j < jobs; j++) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        const int n = (j & 1) ? 1 + (int)((rng >> 33) % 4096) : 1 + (int)((rng >> 33) % 8);
        for (int i = 0; i < n; i++) hits[i].store(0, std::memory_order_relaxed);
        const int tag = j;
        std::atomic<int> live{1};
        pool.run(n, [&, tag](int i) {
            if (i < 0 || i >= n || !live.load(std::memory_order_acquire) || tag != j) errors.fetch_add(1);
            if (i >= 0 && i < n) hits[i].fetch_add(1, std::memory_order_relaxed);
        });
        live.store(0, std::memory_order_release);
        for (int i = 0; i < n; i++)
            if (hits[i].load(std::memory_order_relaxed) != 1) errors.fetch_add(1);
        if ((rng >> 20) & 1) pool.prime();
    }
    *bad = errors.load();
    return SVO_OK;
}

}  // extern "C"
