// Device staging of the windowed bundle adjustment (DESIGN.md section 10,
// "Staging on the device"). A problem's observations arrive as W lists, one per
// camera, each with strictly increasing point ids (the front end's feature lists:
// DESIGN.md section 3). The BA wants them sorted by (point, camera) with index
// lists per point and per camera (ba.hpp). That order is a merge of the W sorted
// lists, so for observation k of camera j with id m
//   staged position = sum over cameras j' of lower_bound(ids_j', m)
//                     + the cameras j' < j whose list holds m
//   first of its point <=> no camera j' < j holds m
// -- W binary searches per observation, each on its own. An inclusive scan of the
// "first" flags in staged order numbers the points (ascending id), and because a
// camera's ids ascend, its k-th observation is its k-th staged position:
// cam_idx[cam_off[j] + k] is the staged position itself. No sort, no atomics;
// every sum is an integer sum in a fixed order, so two runs give the same bits.
//   place  grid (blocks over W cap, P) x 256: positions, "first" counts per workgroup
//   count  one thread per problem: n_obs, n_points (the host sizes the LM's block
//          from these)
//   fill   the same grid: ocam, oxy, cam_idx, flags and ids in staged order
//   points one workgroup of 1024 per problem, looping over its observations: the
//          scan, pt_off, pt_id, the compact points gathered from the map, cam_off,
//          then cam_pt through the scanned flags
#include "ba.hpp"

namespace svo {

namespace {

constexpr int kMaxCams = SVO_BA_MAX_CAMS;
constexpr int kPlaceBlock = 256;
constexpr int kScanBlock = 1024;
constexpr unsigned kFirstBit = 0x80000000u;

// first index of a[0, n) (ascending) whose value is not below m
__device__ __forceinline__ int lower_bound(const int* __restrict__ a, int n, int m) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < m) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the problem's cameras into LDS: counts, list bases (in entries), offsets
__device__ __forceinline__ void load_cams(const BaLists& L, int p, int* cnt, int* base, int* off) {
    if (threadIdx.x < kMaxCams) {
        const int j = threadIdx.x;
        int c = 0, l = 0;
        if (j < L.W) {
            c = min(max(L.counts[p * L.W + j], 0), L.cap);
            l = L.slot ? min(max(L.slot[p * L.W + j], 0), L.W - 1) : j;
        }
        cnt[j] = c;
        base[j] = l * L.cap;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0;
        for (int j = 0; j < kMaxCams; j++) {
            off[j] = o;
            o += cnt[j];
        }
        off[kMaxCams] = o;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kPlaceBlock) void ba_stage_place_kernel(BaLists L, BaStageWork Wk) {
    __shared__ int cnt[kMaxCams], base[kMaxCams], off[kMaxCams + 1];
    const int p = blockIdx.y, WC = L.W * L.cap;
    load_cams(L, p, cnt, base, off);
    const int f = blockIdx.x * kPlaceBlock + threadIdx.x;
    const int j = f / L.cap, k = f - j * L.cap;
    const bool live = f < WC && k < cnt[j];
    bool first = false;
    if (live) {
        const int* __restrict__ ids = L.ids + (size_t)p * WC;
        const int m = ids[base[j] + k];
        int pos = k;
        first = true;
        for (int q = 0; q < L.W; q++) {
            if (q == j || cnt[q] == 0) continue;
            const int* a = ids + base[q];
            const int lb = lower_bound(a, cnt[q], m);
            pos += lb;
            if (q < j && lb < cnt[q] && a[lb] == m) {
                pos++;
                first = false;
            }
        }
        Wk.pos[(size_t)p * WC + f] = (int)((unsigned)pos | (first ? kFirstBit : 0u));
    }
    const int nfirst = __syncthreads_count(live && first);
    if (threadIdx.x == 0) Wk.part[p * gridDim.x + blockIdx.x] = nfirst;
}

__global__ __launch_bounds__(64) void ba_stage_count_kernel(BaLists L, BaStageWork Wk, int nblk) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= L.P) return;
    int o = 0, m = 0;
    for (int j = 0; j < L.W; j++) o += min(max(L.counts[p * L.W + j], 0), L.cap);
    for (int b = 0; b < nblk; b++) m += Wk.part[p * nblk + b];
    Wk.n_obs[p] = o;
    Wk.n_points[p] = m;
}

__global__ __launch_bounds__(kPlaceBlock) void ba_stage_fill_kernel(BaLists L, BaStageWork Wk, BaStageOut O) {
    __shared__ int cnt[kMaxCams], base[kMaxCams], off[kMaxCams + 1];
    const int p = blockIdx.y, WC = L.W * L.cap;
    load_cams(L, p, cnt, base, off);
    const int f = blockIdx.x * kPlaceBlock + threadIdx.x;
    const int j = f / L.cap, k = f - j * L.cap;
    if (f >= WC || k >= cnt[j]) return;
    const unsigned v = (unsigned)Wk.pos[(size_t)p * WC + f];
    const int pos = (int)(v & ~kFirstBit);
    // (a list that is not strictly increasing could place past the end: the
    // callers check or guarantee the order, this is the bounds guard)
    if (pos >= O.maxO || off[j] + k >= O.maxO) return;
    const size_t src = (size_t)p * WC + base[j] + k, dst = (size_t)p * O.maxO + pos;
    O.ocam[dst] = j;
    O.oxy[2 * dst] = L.xy[2 * src];
    O.oxy[2 * dst + 1] = L.xy[2 * src + 1];
    if (L.ur && O.our) O.our[dst] = L.ur[src];
    O.cam_idx[(size_t)p * O.maxO + off[j] + k] = pos;
    Wk.flag[(size_t)p * WC + pos] = (int)(v >> 31);
    Wk.smid[(size_t)p * WC + pos] = L.ids[src];
}

__device__ __forceinline__ int wave_scan_incl(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

__global__ __launch_bounds__(kScanBlock) void ba_stage_points_kernel(BaLists L, BaStageWork Wk, BaStageOut O) {
    __shared__ int cnt[kMaxCams], base[kMaxCams], off[kMaxCams + 1];
    __shared__ int wsum[kScanBlock / 64];
    const int p = blockIdx.x, WC = L.W * L.cap;
    load_cams(L, p, cnt, base, off);
    const int nobs = min(off[kMaxCams], O.maxO);
    int* __restrict__ flag = Wk.flag + (size_t)p * WC;
    const int* __restrict__ smid = Wk.smid + (size_t)p * WC;
    int* pt_off = O.pt_off + (size_t)p * (O.maxM + 1);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int carry = 0;  // points before this chunk (uniform)
    for (int c0 = 0; c0 < nobs; c0 += kScanBlock) {
        const int i = c0 + threadIdx.x;
        const int f = i < nobs ? flag[i] : 0;
        const int incl = wave_scan_incl(f);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanBlock / 64; w++) {
            const int s = wsum[w];
            before += w < wave ? s : 0;
            total += s;
        }
        const int idx = carry + before + incl - 1;  // the observation's point
        if (i < nobs) {
            flag[i] = idx;
            if (f && idx < O.maxM) {
                const int m = smid[i];
                pt_off[idx] = i;
                if (O.pt_id) O.pt_id[(size_t)p * O.maxM + idx] = m;
                if (O.points) {
                    const double* X = O.map + 3 * ((size_t)p * O.map_cap + m);
                    double* Y = O.points + 3 * ((size_t)p * O.maxM + idx);
                    Y[0] = X[0];
                    Y[1] = X[1];
                    Y[2] = X[2];
                }
            }
        }
        carry += total;
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    const int M = min(carry, O.maxM);
    for (int i = M + threadIdx.x; i <= O.maxM; i += kScanBlock) pt_off[i] = nobs;
    if (threadIdx.x <= L.W) O.cam_off[(size_t)p * (L.W + 1) + threadIdx.x] = min(off[threadIdx.x], nobs);
    if (threadIdx.x == 0 && O.n_points) O.n_points[p] = M;
    __syncthreads();  // every flag[] now holds its point index
    // camera lists: entry c names staged position cam_idx[c]
    const int* cam_idx = O.cam_idx + (size_t)p * O.maxO;
    int* cam_pt = O.cam_pt + (size_t)p * O.maxO;
    for (int c = threadIdx.x; c < nobs; c += kScanBlock) cam_pt[c] = flag[cam_idx[c]];
}

__global__ __launch_bounds__(kMaxCams * 12) void ba_stage_cams_kernel(BaLists L, const int* __restrict__ n_cams,
                                                                      const double* __restrict__ ring, int n_fixed,
                                                                      double* __restrict__ poses,
                                                                      uint8_t* __restrict__ fixed) {
    const int p = blockIdx.x, j = threadIdx.x / 12, q = threadIdx.x - 12 * j;
    if (j >= L.W) return;
    const int V = min(max(n_cams[p], 0), L.W);
    const int l = L.slot ? min(max(L.slot[p * L.W + j], 0), L.W - 1) : j;
    poses[12 * ((size_t)p * L.W + j) + q] = j < V ? ring[12 * ((size_t)p * L.W + l) + q] : 0.0;
    if (q == 0) fixed[(size_t)p * L.W + j] = (j < n_fixed || j >= V) ? 1 : 0;
}

__global__ __launch_bounds__(kPlaceBlock) void ba_stage_unstage_kernel(BaLists L, const int* __restrict__ n_cams,
                                                                       const int* __restrict__ n_points,
                                                                       const int* __restrict__ pt_id, int maxM,
                                                                       const double* __restrict__ points,
                                                                       const double* __restrict__ poses,
                                                                       const uint8_t* __restrict__ fixed,
                                                                       double* __restrict__ map, int map_cap,
                                                                       double* __restrict__ ring) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * kPlaceBlock + threadIdx.x;
    if (i < min(n_points[p], maxM)) {
        const int m = pt_id[(size_t)p * maxM + i];
        if (m >= 0 && m < map_cap) {
            const double* X = points + 3 * ((size_t)p * maxM + i);
            double* Y = map + 3 * ((size_t)p * map_cap + m);
            Y[0] = X[0];
            Y[1] = X[1];
            Y[2] = X[2];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < L.W * 12) {
        const int j = threadIdx.x / 12, q = threadIdx.x - 12 * j;
        const int V = min(max(n_cams[p], 0), L.W);
        if (j < V && !fixed[(size_t)p * L.W + j]) {
            const int l = L.slot ? min(max(L.slot[p * L.W + j], 0), L.W - 1) : j;
            ring[12 * ((size_t)p * L.W + l) + q] = poses[12 * ((size_t)p * L.W + j) + q];
        }
    }
}

bool lists_ok(const BaLists& l) { return l.P > 0 && l.W > 0 && l.W <= kMaxCams && l.cap > 0; }

}  // namespace

int ba_stage_blocks(int W, int cap) { return (W * cap + kPlaceBlock - 1) / kPlaceBlock; }

void ba_stage_layout(Carver& c, int P, int W, int cap, BaStageWork& w) {
    const size_t n = (size_t)P * W * cap;
    w.pos = c.take<int>(n);
    w.flag = c.take<int>(n);
    w.smid = c.take<int>(n);
    w.part = c.take<int>((size_t)P * ba_stage_blocks(W, cap));
    w.n_points = c.take<int>(P);
    w.n_obs = c.take<int>(P);
}

hipError_t launch_ba_stage_place(const BaLists& l, const BaStageWork& w, hipStream_t st) {
    if (!lists_ok(l)) return hipErrorInvalidValue;
    const int nb = ba_stage_blocks(l.W, l.cap);
    hipLaunchKernelGGL(ba_stage_place_kernel, dim3(nb, l.P), dim3(kPlaceBlock), 0, st, l, w);
    hipLaunchKernelGGL(ba_stage_count_kernel, dim3((l.P + 63) / 64), dim3(64), 0, st, l, w, nb);
    return hipGetLastError();
}

hipError_t launch_ba_stage_fill(const BaLists& l, const BaStageWork& w, const BaStageOut& o, hipStream_t st) {
    if (!lists_ok(l) || o.maxM < 0 || o.maxO < 0 || (o.points && !o.map)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ba_stage_fill_kernel, dim3(ba_stage_blocks(l.W, l.cap), l.P), dim3(kPlaceBlock), 0, st, l, w, o);
    hipLaunchKernelGGL(ba_stage_points_kernel, dim3(l.P), dim3(kScanBlock), 0, st, l, w, o);
    return hipGetLastError();
}

hipError_t launch_ba_stage_cams(const BaLists& l, const int* n_cams, const double* ring, int n_fixed, double* poses,
                                uint8_t* fixed, hipStream_t st) {
    if (!lists_ok(l)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ba_stage_cams_kernel, dim3(l.P), dim3(kMaxCams * 12), 0, st, l, n_cams, ring, n_fixed, poses,
                       fixed);
    return hipGetLastError();
}

hipError_t launch_ba_stage_unstage(const BaLists& l, const int* n_cams, const int* n_points, const int* pt_id,
                                   int maxM, const double* points, const double* poses, const uint8_t* fixed,
                                   double* map, int map_cap, double* ring, hipStream_t st) {
    if (!lists_ok(l)) return hipErrorInvalidValue;
    const int nb = std::max(1, (maxM + kPlaceBlock - 1) / kPlaceBlock);
    hipLaunchKernelGGL(ba_stage_unstage_kernel, dim3(nb, l.P), dim3(kPlaceBlock), 0, st, l, n_cams, n_points, pt_id,
                       maxM, points, poses, fixed, map, map_cap, ring);
    return hipGetLastError();
}

}  // namespace svo
