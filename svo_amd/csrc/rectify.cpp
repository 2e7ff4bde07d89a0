// Rectification maps (include/svo_gpu.h): a camera's fixed-point map pair on the
// device (svo_rect_maps) and cv::initUndistortRectifyMap(..., CV_16SC2, ...) on
// the host. The kernel that reads the maps is rectify.hip.
#include <climits>
#include <cmath>

#include "common.hpp"

using namespace svo;

namespace {

// cvRound(v) saturated to int32: round half to even (the default rounding mode),
// NaN -> INT_MIN (what cvtsd2si returns for it)
inline int round_sat(double v) {
    const double r = std::nearbyint(v);
    if (std::isnan(r)) return INT_MIN;
    if (r >= 2147483647.0) return INT_MAX;
    if (r <= -2147483648.0) return INT_MIN;
    return (int)r;
}

inline int16_t sat16(int v) { return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v); }

}  // namespace

extern "C" {

int svo_rect_maps_create(svo_ctx* ctx, int raw_w, int raw_h, int w, int h, const int16_t* map1, const uint16_t* map2,
                         svo_rect_maps** out) {
    if (!ctx || !map1 || !map2 || !out) return set_error(ctx, SVO_ERR_ARG, "svo_rect_maps_create: null argument");
    if (raw_w < 2 || raw_h < 2 || w < 1 || h < 1)
        return set_error(ctx, SVO_ERR_ARG, "svo_rect_maps_create: raw size below 2 x 2 or output size below 1 x 1");
    const size_t n = (size_t)w * h;
    for (size_t i = 0; i < n; i++)
        if (map2[i] >= 1024)
            return set_error(ctx, SVO_ERR_ARG, "svo_rect_maps_create: map2[%zu] = %d is no fraction pair (>= 1024)", i,
                             (int)map2[i]);
    (void)hipSetDevice(ctx->device);
    // map1, then map2 (4 n bytes in front of it: dword aligned); + 16: nothing reads
    // it, the quads' wide loads end with the arrays
    void* mem = nullptr;
    SVO_HIP(ctx, hipMalloc(&mem, 6 * n + 16));
    int16_t* d1 = (int16_t*)mem;
    uint16_t* d2 = (uint16_t*)((char*)mem + 4 * n);
    if (hipMemcpy(d1, map1, 4 * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d2, map2, 2 * n, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(mem);
        return set_error(ctx, SVO_ERR_HIP, "svo_rect_maps_create: H2D copy of the maps");
    }
    svo_rect_maps* m = new svo_rect_maps();
    m->mem = mem;
    m->dev = RectMapsDev{d1, d2, raw_w, raw_h, w, h};
    *out = m;
    return SVO_OK;
}

void svo_rect_maps_destroy(svo_ctx* ctx, svo_rect_maps* maps) {
    if (!maps) return;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    if (maps->mem) (void)hipFree(maps->mem);
    delete maps;
}

int svo_init_undistort_rectify_map(const double K[9], const double dist[8], const double R[9], const double newK[9],
                                   int w, int h, int16_t* map1, uint16_t* map2) {
    if (!K || !dist || !R || !newK || !map1 || !map2 || w < 1 || h < 1) return SVO_ERR_ARG;
    // iR = (newK R)^-1 by cofactors
    double m[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            m[3 * i + j] = (newK[3 * i] * R[j] + newK[3 * i + 1] * R[3 + j]) + newK[3 * i + 2] * R[6 + j];
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                       m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (det == 0.0 || !std::isfinite(det)) return SVO_ERR_ARG;
    const double d = 1.0 / det;
    const double ir[9] = {(m[4] * m[8] - m[5] * m[7]) * d, (m[2] * m[7] - m[1] * m[8]) * d,
                          (m[1] * m[5] - m[2] * m[4]) * d, (m[5] * m[6] - m[3] * m[8]) * d,
                          (m[0] * m[8] - m[2] * m[6]) * d, (m[2] * m[3] - m[0] * m[5]) * d,
                          (m[3] * m[7] - m[4] * m[6]) * d, (m[1] * m[6] - m[0] * m[7]) * d,
                          (m[0] * m[4] - m[1] * m[3]) * d};
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4], k4 = dist[5], k5 = dist[6],
                 k6 = dist[7];
    for (int i = 0; i < h; i++) {
        double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
        for (int j = 0; j < w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
            const double ww = 1.0 / _w, x = _x * ww, y = _y * ww;
            const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
            const double u = fx * xd + cx, v = fy * yd + cy;
            const int iu = round_sat(u * 32), iv = round_sat(v * 32);
            const size_t q = (size_t)i * w + j;
            // (the casts saturate where OpenCV's truncate: a far-out coordinate stays outside)
            map1[2 * q] = sat16(iu >> 5);
            map1[2 * q + 1] = sat16(iv >> 5);
            map2[q] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    }
    return SVO_OK;
}

}  // extern "C"
