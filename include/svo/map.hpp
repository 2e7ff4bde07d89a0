// Map — the parts of R:include/map.h / R:src/map.cpp the tracking path uses
// (frame and map-point ownership). The viewer thread, drawer and ground-truth
// parsing are UI and out of scope.
#pragma once

#include <shared_mutex>
#include <unordered_map>
#include <vector>

#include "svo/types.hpp"

namespace svo {

class Frame;
class MapPoint;

class Map {
public:
    Map() = default;
    ~Map();
    Map(const Map&) = delete;
    Map& operator=(const Map&) = delete;

    void addFrame(Frame* frame);
    MapPoint* createMapPoint(const Point3d& position);
    [[nodiscard]] size_t mapPointsSize() const;
    [[nodiscard]] size_t framesSize() const;
    // frame `index` in insertion order; negative counts from the newest (-1)
    [[nodiscard]] Frame* frameAt(long index) const;

    struct BundleResult {
        double initialCost = 0, finalCost = 0;
        int iterations = 0;
        size_t frames = 0, points = 0, observations = 0;
    };
    // The body R:src/map.cpp's Map::run leaves as "TODO optimization part here", as
    // an explicit call: windowed bundle adjustment (svo_bundle_adjust) of the last
    // `window` frames the map holds (at most SVO_BA_MAX_CAMS), the oldest n_fixed
    // of them held constant, and of every map point with an observation in them
    // that is not flagged isOutlier (MapPoint::mObservations). K: row-major 3x3.
    // Writes back the free frames' poses and the points' mWorldPos. Throws
    // std::invalid_argument for a bad window, std::runtime_error if the GPU call fails.
    BundleResult localBundleAdjust(svo_ctx* ctx, const double K[9], int window, int n_fixed, double huber_delta,
                                   int max_iterations);

private:
    std::vector<Frame*> mAllFrames;
    std::unordered_map<size_t, Frame*> mKeyFrames;
    std::vector<MapPoint*> mMapPoints;
    mutable std::shared_mutex mMapMutex;
};

}  // namespace svo
