// The batched front end's place memory (svo_frontend_places_enable; the rules:
// DESIGN.md section 3e): kernels that describe every sequence's feature list on
// its own frame, compact the valid entries in order into a record, and gather a
// chosen record's matched pairs for the pose solver (places.hip).
#pragma once

#include "orb.hpp"

namespace svo {

// Level 0 of frames[s] (s < nseq) blurred by the descriptors' 7-tap kernel into
// out + s * seq_stride (rows `pitch` apart); w x h: the frames' size.
hipError_t launch_places_blur(const PyrDesc* frames, int nseq, int w, int h, uint8_t* out, size_t seq_stride,
                              int pitch, hipStream_t st);

// Section 3d's descriptor of every feature (xy [s][cap][2], n[s] of them) at octave
// 0 of its sequence's frame: the level pixel is (rint(x), rint(y)) (f32, half to
// even), valid iff it lies `reach` inside the frame; moments on frames[s].lv[0],
// samples on blurred + s * seq_stride. desc [s][cap][32] (zero where invalid),
// valid [s][cap]. hp: the half patch, umax: its hp + 1 half row widths (host),
// pattern: 512 (x, y) int8 on the device.
hipError_t launch_places_describe(const PyrDesc* frames, const uint8_t* blurred, size_t seq_stride, int pitch,
                                  const float* xy, const int* n, int cap, int nseq, int hp, const int* umax,
                                  int reach, const int8_t* pattern, uint8_t* desc, uint8_t* valid,
                                  hipStream_t st);

// The valid entries of every sequence's list in list order: descriptors, pixels
// and (mid non-null) map ids into desc_out / xy_out / mid_out + s * out_stride
// entries, their count into n_out[s * n_stride].
struct PlacesCompact {
    const int* n;          // [s]
    const uint8_t* valid;  // [s][cap]
    const uint8_t* desc;   // [s][cap][32]
    const float* xy;       // [s][cap][2]
    const int* mid;        // [s][cap], nullable
    int cap;
    uint8_t* desc_out;
    float* xy_out;
    int* mid_out;  // [s][cap], nullable with mid
    size_t out_stride;
    int* n_out;
    int n_stride;
};
hipError_t launch_places_compact(const PlacesCompact& c, int nseq, hipStream_t st);

// A record's map points: xyz_out[s * out_stride + i] = map[s][mid[s][i]] (three f64,
// copied bit for bit) for i < n[s * n_stride]; an id outside [0, map_cap) reads nothing.
hipError_t launch_places_gather_xyz(const int* mid, int cap, const int* n, int n_stride, const double* map,
                                    int map_cap, double* xyz_out, size_t out_stride, int nseq, hipStream_t st);

// The solver's inputs of chosen problem k < n_sel: for pair i < n_pairs[prob[k]] of
// pairs [problem][cap][2] = (query index, record index): obj[k][i] = the record's
// xyz (set rec_set[k] of rec_xyz, `cap` entries per set), img[k][i] = the query's
// xy (set q_set[k] of q_xy). prob / q_set / rec_set: device, [n_sel].
hipError_t launch_places_gather_pairs(const int* pairs, const int* n_pairs, const int* prob, const int* q_set,
                                      const int* rec_set, int n_sel, int cap, const float* q_xy,
                                      const double* rec_xyz, double* obj, float* img, hipStream_t st);

}  // namespace svo
