// Map::localBundleAdjust — the optimisation R:src/map.cpp's Map::run leaves as a
// TODO, on the GPU (svo_bundle_adjust) and as an explicit call: nothing in
// Tracking's loop calls it.
#include <algorithm>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "svo/frame.hpp"
#include "svo/map.hpp"
#include "svo/map_point.hpp"
#include "svo_gpu.h"

namespace svo {

Frame* Map::frameAt(long index) const {
    std::shared_lock lock(mMapMutex);
    const long n = (long)mAllFrames.size();
    if (index < 0) index += n;
    return index >= 0 && index < n ? mAllFrames[(size_t)index] : nullptr;
}

Map::BundleResult Map::localBundleAdjust(svo_ctx* ctx, const double K[9], int window, int n_fixed,
                                         double huber_delta, int max_iterations) {
    std::unique_lock lock(mMapMutex);
    if (!ctx || !K) throw std::invalid_argument("localBundleAdjust: no context or intrinsics");
    if (window <= 0 || window > SVO_BA_MAX_CAMS)
        throw std::invalid_argument("localBundleAdjust: window must be 1 .. SVO_BA_MAX_CAMS");
    if (n_fixed < 0 || max_iterations < 0) throw std::invalid_argument("localBundleAdjust: negative argument");
    BundleResult res;
    const size_t C = std::min((size_t)window, mAllFrames.size());
    if (C == 0) return res;
    Frame* const* frames = mAllFrames.data() + (mAllFrames.size() - C);
    // frame poses are camera -> world; the solver's are world -> camera
    std::vector<double> poses(12 * C);
    std::vector<uint8_t> fixed(C);
    for (size_t j = 0; j < C; j++) {
        const SE3d T = frames[j]->pose().inverse();
        for (int k = 0; k < 9; k++) poses[12 * j + k] = T.R[k];
        for (int k = 0; k < 3; k++) poses[12 * j + 9 + k] = T.t[k];
        fixed[j] = j < (size_t)n_fixed;
    }
    std::vector<MapPoint*> pts;
    std::vector<double> xyz;
    std::vector<int> ocam, opt;
    std::vector<float> oxy;
    for (MapPoint* mp : mMapPoints) {
        bool seen = false;
        for (size_t j = 0; j < C; j++) {
            const auto it = mp->mObservations.find(frames[j]->ID);
            if (it == mp->mObservations.end() || it->second->isOutlier) continue;
            if (!seen) {
                seen = true;
                pts.push_back(mp);
                xyz.insert(xyz.end(), {mp->mWorldPos.x, mp->mWorldPos.y, mp->mWorldPos.z});
            }
            ocam.push_back((int)j);
            opt.push_back((int)pts.size() - 1);
            oxy.push_back(it->second->pos.x);
            oxy.push_back(it->second->pos.y);
        }
    }
    res.frames = C;
    res.points = pts.size();
    res.observations = ocam.size();
    double costs[2] = {0, 0};
    if (svo_bundle_adjust(ctx, 1, (int)C, (int)pts.size(), (int)ocam.size(), nullptr, nullptr, nullptr, poses.data(),
                          fixed.data(), xyz.data(), ocam.data(), opt.data(), oxy.data(), K, huber_delta,
                          max_iterations, costs, &res.iterations) != SVO_OK)
        throw std::runtime_error(std::string("svo_bundle_adjust: ") + svo_last_error(ctx));
    res.initialCost = costs[0];
    res.finalCost = costs[1];
    for (size_t j = 0; j < C; j++) {
        if (fixed[j]) continue;  // untouched, bit for bit
        frames[j]->pose() = SE3d(&poses[12 * j], &poses[12 * j + 9]).inverse();
    }
    for (size_t i = 0; i < pts.size(); i++) pts[i]->mWorldPos = Point3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    return res;
}

}  // namespace svo
