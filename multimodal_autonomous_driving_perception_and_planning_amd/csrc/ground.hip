// The camera model: a ground-plane homography per camera (av_ground_cfg), made on the host (av_ground_make), and the bird's-eye
// warp of the frames through it (av_ground_warp).
//
// The reference has no camera: BEVRenderer draws a track at forward = 50 - cy * 0.1, lateral = (cx - 320) * 0.03
// (bev_renderer.py:207-208), the map av_obstacle_cfg carries.  A flat road seen by a pinhole camera is a plane-to-plane
// projection, so image (u, v, 1) and road (forward, lateral, 1) are related by a 3 x 3 matrix up to scale; av_ground_cfg holds it
// and its true inverse, so that one sign convention (D > 0: below the horizon, in front of the camera) holds in both directions.
// The projection of image points is in ground_dev.h (obstacles.hip, bridge.hip use it), and so is a panel pixel's sampling, which
// surround.hip shares; this file has the pixel kernel.
//
// av_ground_warp: resample_dev.h's tile, store and bilinear sample.  Per pixel: the road point of the pixel's centre through ginv in
// float64 (header's operation order), the source position rounded to 1/65536 pixel, then the sample.
#include "common.h"
#include "ground_dev.h"

#include <cmath>
#include <cstring>

namespace {

template <bool WIDE>        // the frames are at least two pixels wide: the sample's packed form
__global__ void __launch_bounds__(256) ground_warp_kernel(const av_ground_cfg* __restrict__ ground, int h, int w,
                                                          const uint8_t* __restrict__ bgr, int gh, int gw, double f_far,
                                                          double m_per_px, unsigned fill, uint8_t* __restrict__ out) {
    const int cam = blockIdx.z;
    int r, c0, npx;
    if (!resample::tile_thread(gh, gw, r, c0, npx)) return;
    const double* q = ground[cam].ginv;                             // the same for the whole grid slice: scalar loads
    const uint8_t* src = bgr + (size_t)cam * h * w * 3;
    const double f = f_far - ((double)r + 0.5) * m_per_px;
    unsigned px[resample::PX];
#pragma unroll
    for (int j = 0; j < resample::PX; ++j) {                        // (a column past the row's end is not computed)
        const double l = (((double)(c0 + j) + 0.5) - (double)gw / 2.0) * m_per_px;
        long long iu, iv;
        // `fill` where the road point is at or above the horizon, behind the camera or outside the frame
        px[j] = j < npx && grounddev::warp_position(q, h, w, f, l, iu, iv) ? grounddev::warp_sample<WIDE>(src, h, w, iu, iv) : fill;
    }
    resample::store_px4(out + (((size_t)cam * gh + r) * gw + c0) * 3, px, npx);      // r < gh, c0 + npx <= gw
}

}  // namespace

extern "C" int av_ground_make(const double g[9], double max_range, int anchor, av_ground_cfg* out) {
    AV_REQUIRE(g && out, AV_EINVAL, "av_ground_make: null argument");
    for (int i = 0; i < 9; ++i) AV_REQUIRE(std::isfinite(g[i]), AV_EINVAL, "av_ground_make: g[%d] is not finite", i);
    AV_REQUIRE(max_range > 0.0 && std::isfinite(max_range), AV_EINVAL, "av_ground_make: max_range must be > 0 and finite");
    AV_REQUIRE(anchor == 0 || anchor == 1, AV_EINVAL, "av_ground_make: anchor %d is neither 0 (centre) nor 1 (bottom centre)", anchor);
    // adj(g) / det(g)
    const double a[9] = {g[4] * g[8] - g[5] * g[7], g[2] * g[7] - g[1] * g[8], g[1] * g[5] - g[2] * g[4],
                         g[5] * g[6] - g[3] * g[8], g[0] * g[8] - g[2] * g[6], g[2] * g[3] - g[0] * g[5],
                         g[3] * g[7] - g[4] * g[6], g[1] * g[6] - g[0] * g[7], g[0] * g[4] - g[1] * g[3]};
    const double det = (g[0] * a[0] + g[1] * a[3]) + g[2] * a[6];
    AV_REQUIRE(det != 0.0 && std::isfinite(det), AV_EINVAL, "av_ground_make: g is singular");
    double inv[9];
    for (int i = 0; i < 9; ++i) {
        inv[i] = a[i] / det;
        AV_REQUIRE(std::isfinite(inv[i]), AV_EINVAL, "av_ground_make: the inverse of g is not finite");
    }
    std::memcpy(out->g, g, sizeof out->g);
    std::memcpy(out->ginv, inv, sizeof out->ginv);
    out->max_range = max_range, out->anchor = anchor, out->reserved = 0;
    return AV_OK;
}

extern "C" int av_ground_warp(av_ctx* ctx, av_stream_t stream, const av_ground_cfg* ground, int n_cams, int h, int w,
                              const uint8_t* bgr, int gh, int gw, double f_far, double m_per_px, const uint8_t fill[3],
                              uint8_t* out) {
    AV_REQUIRE(ctx && ground && bgr && fill && out, AV_EINVAL, "av_ground_warp: null argument");
    AV_REQUIRE(n_cams >= 1 && h >= 1 && w >= 1 && gh >= 1 && gw >= 1, AV_EINVAL, "av_ground_warp: n_cams, h, w, gh and gw must be >= 1");
    AV_REQUIRE(m_per_px > 0.0 && std::isfinite(m_per_px) && std::isfinite(f_far), AV_EINVAL,
               "av_ground_warp: m_per_px must be > 0 and finite, f_far finite");
    dim3 grid;
    if (int rc = resample::tile_grid(gw, gh, n_cams, "av_ground_warp", "cameras", &grid)) return rc;
    const auto kernel = w >= 2 ? ground_warp_kernel<true> : ground_warp_kernel<false>;      // a source one pixel wide: tap by tap
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), ground, h, w, bgr, gh, gw, f_far, m_per_px, resample::pack_bgr(fill), out);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
