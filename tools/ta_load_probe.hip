// Probe: what does a per-lane global load cost the texture addresser (TA) by
// width and by active lanes? LK's level setup is TA-bound (profiles/r06/
// r_lk_mem_pipeline.txt) and issues only 2- and 8-byte loads; this measures the
// forms a paired strip map would use instead, at LK's address shape: four 16-lane
// groups per wave, each at its own window of an image that stays in L2, lanes
// STRIDE bytes apart, 8 rows one pitch apart in flight together.
//
//   form      bytes  lane stride
//   u16       2      1 B   (prev pixel pair, any byte address)
//   u32       4      1 B   (prev pixels x .. x + 3, any byte address)
//   u32x2     8      4 B   (derivative records x, x + 1)
//   u32x3     12     4 B   (records x .. x + 2)
//   u32x4     16     4 B   (records x .. x + 3; 4-byte aligned only)
//
// each with all 64 lanes and with 4 (the last lane of every group) under EXEC.
// Wall time per wave-instruction from events; TA_TA_BUSY from a counters-only
// pass of its own over the same binary (tools/gpu.sh taprobe).
//
//   hipcc --offload-arch=gfx950 -O3 tools/ta_load_probe.hip -o tools/bin/ta_load_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

typedef const __attribute__((address_space(1))) uint8_t* gu8;
typedef uint16_t u16a1 __attribute__((aligned(1)));
typedef uint32_t u32a1 __attribute__((aligned(1)));
typedef uint32_t u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x3a4 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kW = 1241, kH = 376, kPitch = 1312;  // a KITTI level 0 with its padding
constexpr int kRows = 8, kIters = 64, kBlocks = 4096;
constexpr size_t kBytes = (size_t)(kH + 2 * kRows) * kPitch * 4 + 64;

__device__ __forceinline__ unsigned fold(uint16_t v) { return v; }
__device__ __forceinline__ unsigned fold(uint32_t v) { return v; }
__device__ __forceinline__ unsigned fold(u32x2a4 v) { return v.x ^ v.y; }
__device__ __forceinline__ unsigned fold(u32x3a4 v) { return v.x ^ v.y ^ v.z; }
__device__ __forceinline__ unsigned fold(u32x4a4 v) { return v.x ^ v.y ^ v.z ^ v.w; }

// T: the load form; STRIDE: bytes between neighbouring lanes (and per pixel of
// the plane: the pitch is kPitch * STRIDE bytes); FEW: only lane 15 of each group
template <typename T, int STRIDE, bool FEW>
__global__ __launch_bounds__(256) void ta_probe_kernel(const uint8_t* src, unsigned* out, unsigned key) {
    const gu8 b = (gu8)src;
    const unsigned lane = threadIdx.x & 63, l = lane & 15;
    const unsigned grp = (blockIdx.x * 256u + threadIdx.x) >> 4;
    unsigned acc = 0;
    unsigned h = grp * 2654435761u + 12345u;
    for (int it = 0; it < kIters; it++) {
        h = h * 1664525u + 1013904223u;
        const unsigned x = (h >> 8) % (unsigned)(kW - 24), y = (h >> 20) % (unsigned)(kH - kRows);
        const unsigned off = (y * kPitch + x + l) * STRIDE;
        if (!FEW || l == 15) {
            T v[kRows];
#pragma unroll
            for (int r = 0; r < kRows; r++)
                v[r] = *(const __attribute__((address_space(1))) T*)(b + (size_t)r * kPitch * STRIDE + off);
#pragma unroll
            for (int r = 0; r < kRows; r++) acc += fold(v[r]);
        }
    }
    if (acc == key) out[0] = acc;  // (never, in effect: the loads must stay)
}

typedef void (*probe_t)(const uint8_t*, unsigned*, unsigned);

int main() {
    struct {
        const char* name;
        int bytes, stride, lanes;
        probe_t fn;
    } P[] = {
        {"u16   2 B  stride 1", 2, 1, 64, ta_probe_kernel<u16a1, 1, false>},
        {"u32   4 B  stride 1", 4, 1, 64, ta_probe_kernel<u32a1, 1, false>},
        {"u32x2 8 B  stride 4", 8, 4, 64, ta_probe_kernel<u32x2a4, 4, false>},
        {"u32x3 12 B stride 4", 12, 4, 64, ta_probe_kernel<u32x3a4, 4, false>},
        {"u32x4 16 B stride 4", 16, 4, 64, ta_probe_kernel<u32x4a4, 4, false>},
        {"u16   2 B  stride 1", 2, 1, 4, ta_probe_kernel<u16a1, 1, true>},
        {"u32   4 B  stride 1", 4, 1, 4, ta_probe_kernel<u32a1, 1, true>},
        {"u32x2 8 B  stride 4", 8, 4, 4, ta_probe_kernel<u32x2a4, 4, true>},
        {"u32x3 12 B stride 4", 12, 4, 4, ta_probe_kernel<u32x3a4, 4, true>},
        {"u32x4 16 B stride 4", 16, 4, 4, ta_probe_kernel<u32x4a4, 4, true>},
    };
    uint8_t* d;
    unsigned* out;
    if (hipMalloc(&d, kBytes) != hipSuccess || hipMalloc(&out, 4) != hipSuccess) {
        fprintf(stderr, "no device memory\n");
        return 1;
    }
    std::vector<uint8_t> hbuf(kBytes);
    for (size_t i = 0; i < kBytes; i++) hbuf[i] = (uint8_t)(i * 37 + (i >> 8));
    (void)hipMemcpy(d, hbuf.data(), kBytes, hipMemcpyHostToDevice);
    hipDeviceProp_t prop;
    (void)hipGetDeviceProperties(&prop, 0);
    const double cus = prop.multiProcessorCount, mhz = prop.clockRate / 1e3;
    printf("%d CUs at %.0f MHz; %d blocks x 4 waves, %d x %d loads per wave\n", (int)cus, mhz, kBlocks, kIters, kRows);
    printf("form                 lanes   us     ns/wave-inst/CU  cycles/wave-inst/CU\n");
    for (auto& p : P) {
        hipLaunchKernelGGL(p.fn, dim3(kBlocks), dim3(256), 0, 0, d, out, 0x12345679u);  // warm: code object, L2
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0);
        (void)hipEventCreate(&e1);
        float best = 1e30f;
        for (int rep = 0; rep < 3; rep++) {
            (void)hipEventRecord(e0, 0);
            hipLaunchKernelGGL(p.fn, dim3(kBlocks), dim3(256), 0, 0, d, out, 0x12345679u);
            (void)hipEventRecord(e1, 0);
            if (hipEventSynchronize(e1) != hipSuccess) {
                fprintf(stderr, "kernel failed\n");
                return 1;
            }
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            best = ms < best ? ms : best;
        }
        const double inst_per_cu = (double)kBlocks * 4 * kIters * kRows / cus;
        const double ns = best * 1e6 / inst_per_cu;
        printf("%-20s %5d %7.1f %10.3f %16.2f\n", p.name, p.lanes, best * 1e3, ns, ns * mhz / 1e3);
    }
    return 0;
}
