// Stand-alone host check of the front end's thread pool and CPU plan
// (svo_amd/csrc/host_pool.cpp), meant for a sanitizer build on the build machine:
//   clang++ -std=c++17 -O1 -g -fsanitize=thread -pthread -Iinclude -Isvo_amd/csrc \
//       tools/pool_check.cpp svo_amd/csrc/host_pool.cpp -o tools/bin/pool_check
//   tools/bin/pool_check 2 8 16          (or -fsanitize=address,undefined)
// Runs svo_pool_selftest (4000 jobs) for every thread count given, and
// svo_host_cpu_plan for a few (rank, world) pairs with and without GPU nodes.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "svo_gpu.h"

int main(int argc, char** argv) {
    int64_t total = 0;
    for (int a = 1; a < argc; a++) {
        int64_t bad = -1;
        const int rc = svo_pool_selftest(std::atoi(argv[a]), 4000, &bad);
        std::printf("selftest threads=%s rc=%d bad=%lld\n", argv[a], rc, (long long)bad);
        total += rc ? 1 : bad;
    }
    const int nodes[4] = {0, 0, 1, -1};
    for (int world : {1, 2, 4})
        for (int rank = 0; rank < world; rank++)
            for (const int* gn : {(const int*)nullptr, nodes}) {
                int cpus[4096], n = -1;
                const int rc = svo_host_cpu_plan(rank, world, gn, cpus, 4096, &n);
                std::printf("plan rank=%d/%d nodes=%d rc=%d n=%d first=%d\n", rank, world, gn != nullptr, rc, n,
                            n > 0 ? cpus[0] : -1);
                total += rc ? 1 : 0;
            }
    std::printf("bad == %lld\n", (long long)total);
    return total ? 1 : 0;
}
