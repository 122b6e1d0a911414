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
// av_ground_warp, mapping: a thread makes four adjacent pixels of one panel row and stores them as 12 bytes at once (tail of a
// row: byte by byte); a 256-thread workgroup covers a tile of 64 columns x 16 rows, because vertically adjacent panel pixels read
// adjacent source rows (the lower tap row of one is the upper of the next) and horizontally adjacent ones adjacent source pixels:
// a tile's taps share cache lines in both directions.  Per pixel: the road point of the pixel's centre through ginv in float64
// (header's operation order), the source position rounded to 1/65536 pixel, then rasterdev::resize_channel's bilinear rule.
#include "common.h"
#include "ground_dev.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int TILE_W = 64, TILE_H = 16, PX = 4;     // pixels per tile row, rows per tile, pixels per thread

// one panel pixel as b | g << 8 | r << 16; `fill` where the road point is at or above the horizon, behind the camera or outside the frame
__device__ __forceinline__ unsigned warp_pixel(const double* __restrict__ q, const uint8_t* __restrict__ src, int h, int w, double f,
                                               double l, unsigned fill) {
    long long iu, iv;
    return grounddev::warp_position(q, h, w, f, l, iu, iv) ? grounddev::warp_sample(src, h, w, iu, iv) : fill;
}

__global__ void __launch_bounds__(256) ground_warp_kernel(const av_ground_cfg* __restrict__ ground, int h, int w,
                                                          const uint8_t* __restrict__ bgr, int gh, int gw, double f_far,
                                                          double m_per_px, unsigned fill, uint8_t* __restrict__ out) {
    const int cam = blockIdx.z;
    const int r = blockIdx.y * TILE_H + (int)(threadIdx.x / (TILE_W / PX));
    const long long c0l = (long long)blockIdx.x * TILE_W + (int)(threadIdx.x % (TILE_W / PX)) * PX;
    if (r >= gh || c0l >= gw) return;
    const int c0 = (int)c0l;
    const double* q = ground[cam].ginv;                             // the same for the whole grid slice: scalar loads
    const uint8_t* src = bgr + (size_t)cam * h * w * 3;
    const double f = f_far - ((double)r + 0.5) * m_per_px;
    const int npx = min(PX, gw - c0);
    unsigned px[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {                                  // (a column past the row's end is not computed)
        const double l = (((double)(c0 + j) + 0.5) - (double)gw / 2.0) * m_per_px;
        px[j] = j < npx ? warp_pixel(q, src, h, w, f, l, fill) : fill;
    }
    uint8_t* o = out + (((size_t)cam * gh + r) * gw + c0) * 3;      // r < gh, c0 + npx <= gw
    if (npx == PX) {
        const unsigned words[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
        __builtin_memcpy(o, words, 12);                             // one 12-byte store, at any alignment
    } else {
#pragma unroll
        for (int j = 0; j < PX - 1; ++j)
            if (j < npx) o[j * 3] = (uint8_t)px[j], o[j * 3 + 1] = (uint8_t)(px[j] >> 8), o[j * 3 + 2] = (uint8_t)(px[j] >> 16);
    }
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
    const long long tiles_y = ((long long)gh + TILE_H - 1) / TILE_H;
    AV_REQUIRE(n_cams <= 65535 && tiles_y <= 65535, AV_EINVAL, "av_ground_warp: more than 65535 cameras or tile rows");
    const unsigned fc = (unsigned)fill[0] | ((unsigned)fill[1] << 8) | ((unsigned)fill[2] << 16);
    const dim3 grid((unsigned)(((long long)gw + TILE_W - 1) / TILE_W), (unsigned)tiles_y, (unsigned)n_cams);
    hipLaunchKernelGGL(ground_warp_kernel, grid, dim3(256), 0, as_stream(stream), ground, h, w, bgr, gh, gw, f_far, m_per_px, fc, out);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
