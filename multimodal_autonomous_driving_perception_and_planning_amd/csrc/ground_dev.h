// The ground-plane camera model's device side (include/avhot.h: av_ground_cfg): the projection of an image point onto the road,
// shared by the ground forms of av_track_obstacles (obstacles.hip) and av_lane_paths (bridge.hip), and the way back, a road point's
// place in the frame and the picture there (resample_dev.h's sample), shared by av_ground_warp (ground.hip), av_rig_surround
// (surround.hip) and the odometry's patch stage (egoflow.hip).  float64, every operation rounded on its own, in the header's order.
#pragma once
#include "common.h"
#include "resample_dev.h"

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

// the frame position of road point (f, l) through q = av_ground_cfg.ginv, in 1/65536 pixels (av_ground_warp's tu, tv): false where
// the point is at or above the horizon, behind the camera or outside the h x w frame (a NaN fails); inside, both are exact integers
// below 2^47
__device__ __forceinline__ bool warp_position(const double* __restrict__ q, int h, int w, double f, double l, long long& iu,
                                              long long& iv) {
    const double U = (q[0] * f + q[1] * l) + q[2], V = (q[3] * f + q[4] * l) + q[5], D = (q[6] * f + q[7] * l) + q[8];
    if (!(D > 0.0)) return false;
    const double u = U / D, v = V / D;
    const double tu = floor(u * 65536.0 + 0.5), tv = floor(v * 65536.0 + 0.5);
    if (!(tu >= 0.0 && tu <= (double)(w - 1) * 65536.0 && tv >= 0.0 && tv <= (double)(h - 1) * 65536.0)) return false;
    iu = (long long)tu, iv = (long long)tv;
    return true;
}

// the picture at such a position as b | g << 8 | r << 16: resample_dev.h's bilinear sample (WIDE: its packed form, needs w >= 2)
template <bool WIDE>
__device__ __forceinline__ unsigned warp_sample(const uint8_t* __restrict__ src, int h, int w, long long iu, long long iv) {
    return resample::bilinear_bgr<WIDE>(src, h, w, iu, iv);
}

}  // namespace grounddev
