// The ground-plane camera model's device side (include/avhot.h: av_ground_cfg): the projection of an image point onto the road,
// shared by the ground forms of av_track_obstacles (obstacles.hip) and av_lane_paths (bridge.hip).  float64, every operation
// rounded on its own, in the order the header states.
#pragma once
#include "common.h"

namespace grounddev {

struct RoadPoint {
    double f, l, D;     // forward, lateral (metres), and the homogeneous divisor: D > 0 = below the horizon, in front of the camera
    bool on_road;       // D > 0 && 0 <= f <= max_range  (a NaN fails)
};

// g: the nine entries of av_ground_cfg.g (any address space; a wave-uniform table entry is read through scalar loads)
__device__ __forceinline__ RoadPoint project(const double* __restrict__ g, double max_range, double u, double v) {
    RoadPoint p;
    const double F = (g[0] * u + g[1] * v) + g[2], L = (g[3] * u + g[4] * v) + g[5];
    p.D = (g[6] * u + g[7] * v) + g[8];
    p.f = F / p.D, p.l = L / p.D;
    p.on_road = p.D > 0.0 && p.f >= 0.0 && p.f <= max_range;
    return p;
}

// the projection's Jacobian at p: metres per pixel
struct RoadJac {
    double dfu, dfv, dlu, dlv;
};
__device__ __forceinline__ RoadJac jacobian(const double* __restrict__ g, const RoadPoint& p) {
    RoadJac j;
    j.dfu = (g[0] - p.f * g[6]) / p.D, j.dfv = (g[1] - p.f * g[7]) / p.D;
    j.dlu = (g[3] - p.l * g[6]) / p.D, j.dlv = (g[4] - p.l * g[7]) / p.D;
    return j;
}

}  // namespace grounddev
