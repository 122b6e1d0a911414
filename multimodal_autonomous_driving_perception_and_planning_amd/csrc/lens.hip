// Lens distortion (av_lens_cfg, made on the host by av_lens_make): the tables that rectify a frame (av_lens_map_rectify) or
// take the bird's-eye view straight from raw frames (av_lens_map_ground), and the kernel that applies such a table (av_remap).
//
// Undistorting costs about twice the float64 operations per pixel of av_ground_warp, which is already bound by the issue of
// float64 instructions.  The float64 work is therefore done once per lens, into a table of source positions in
// 1/65536 pixels, and the per-frame kernel is integer only: 8 bytes of table in, four taps, 3 bytes out per pixel.  The tables
// need the FORWARD model only (rectified pixel -> raw position); the Newton inverse of lens_dev.h serves points (obstacles.hip).
//
// av_remap: resample_dev.h's tile, store and bilinear sample (its packed form: the two taps of a source row fetched together).  A
// thread makes four adjacent pixels of one output row from 32 contiguous table bytes (tail of a row: entry by entry).  Every source
// index is derived from an entry that has passed the range check against (sw, sh): a foreign table cannot make the kernel read
// outside bgr.  The table builders use the tile's constants with a rule of their own: one column and four rows per thread.
#include "common.h"
#include "lens_dev.h"
#include "resample_dev.h"

#include <cmath>
#include <cstring>

namespace {

using resample::PX, resample::TILE_H, resample::TILE_W;
constexpr int MAX_SIDE = 32768;                     // (side - 1) * 65536 fits an int32

// rectified pixel (u, v) of lens L -> the map entry of the raw position
__host__ __device__ __forceinline__ void raw_entry(const av_lens_cfg* __restrict__ L, double u, double v, int32_t* o) {
    const double x = (u - L->ncx) / L->nfx, y = (v - L->ncy) / L->nfy;
    double xd, yd;
    lensdev::distort(&L->k1, x, y, &xd, &yd);
    lensdev::map_entry(L->fx * xd + L->cx, L->fy * yd + L->cy, L->w, L->h, o, o + 1);
}

// one thread per map entry (cold path: once per lens)
__global__ void __launch_bounds__(256) lens_map_rectify_kernel(const av_lens_cfg* __restrict__ lens, int h, int w,
                                                               int32_t* __restrict__ map) {
    const int k = blockIdx.z;
    const int r = blockIdx.y * TILE_H + (int)(threadIdx.x / TILE_W);
    const long long cl = (long long)blockIdx.x * TILE_W + (int)(threadIdx.x % TILE_W);
    if (cl >= w) return;
    const av_lens_cfg* L = lens + k;
    const bool same = L->w == w && L->h == h;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int rr = r + j * (TILE_H / PX);                       // four rows per thread: 64 columns x 16 rows per workgroup
        if (rr >= h) break;
        int32_t e[2] = {-1, -1};
        if (same) raw_entry(L, (double)(int)cl, (double)rr, e);
        int32_t* o = map + (((size_t)k * h + rr) * w + (size_t)cl) * 2;
        o[0] = e[0], o[1] = e[1];
    }
}

__global__ void __launch_bounds__(256) lens_map_ground_kernel(const av_lens_cfg* __restrict__ lens,
                                                              const av_ground_cfg* __restrict__ ground, int gh, int gw, double f_far,
                                                              double m_per_px, int32_t* __restrict__ map) {
    const int k = blockIdx.z;
    const int r = blockIdx.y * TILE_H + (int)(threadIdx.x / TILE_W);
    const long long cl = (long long)blockIdx.x * TILE_W + (int)(threadIdx.x % TILE_W);
    if (cl >= gw) return;
    const av_lens_cfg* L = lens + k;
    const double* q = ground[k].ginv;
    const double l = (((double)(int)cl + 0.5) - (double)gw / 2.0) * m_per_px;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int rr = r + j * (TILE_H / PX);
        if (rr >= gh) break;
        const double f = f_far - ((double)rr + 0.5) * m_per_px;
        const double U = (q[0] * f + q[1] * l) + q[2], V = (q[3] * f + q[4] * l) + q[5], D = (q[6] * f + q[7] * l) + q[8];
        int32_t e[2] = {-1, -1};
        if (D > 0.0) raw_entry(L, U / D, V / D, e);
        int32_t* o = map + (((size_t)k * gh + rr) * gw + (size_t)cl) * 2;
        o[0] = e[0], o[1] = e[1];
    }
}

// one output pixel as b | g << 8 | r << 16 from a table entry; lim = ((sw - 1) << 16, (sh - 1) << 16).  WIDE: sw >= 2
template <bool WIDE>
__device__ __forceinline__ unsigned remap_pixel(const uint8_t* __restrict__ src, int sh, int sw, unsigned lim_u, unsigned lim_v,
                                                int32_t tu, int32_t tv, unsigned fill) {
    if ((unsigned)tu > lim_u || (unsigned)tv > lim_v) return fill;      // (a negative entry is a large unsigned)
    return resample::bilinear_bgr<WIDE>(src, sh, sw, tu, tv);
}

template <bool WIDE>
__global__ void __launch_bounds__(256) remap_kernel(const int32_t* __restrict__ map, int cam_stride, int sh, int sw,
                                                    const uint8_t* __restrict__ bgr, int dh, int dw, unsigned fill,
                                                    uint8_t* __restrict__ out) {
    const int cam = blockIdx.z;
    int r, c0, npx;
    if (!resample::tile_thread(dh, dw, r, c0, npx)) return;
    const uint8_t* src = bgr + (size_t)cam * sh * sw * 3;
    const size_t px0 = (size_t)r * dw + c0;                          // r < dh, c0 < dw
    const int32_t* mp = map + ((size_t)(cam / cam_stride) * dh * dw + px0) * 2;
    const unsigned lim_u = (unsigned)(sw - 1) << 16, lim_v = (unsigned)(sh - 1) << 16;      // sw, sh <= 32768
    uint8_t* o = out + ((size_t)cam * dh * dw + px0) * 3;
    if (npx == PX) {
        int32_t e[2 * PX];
        __builtin_memcpy(e, mp, sizeof e);                          // the four entries: 32 contiguous bytes
        unsigned px[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) px[j] = remap_pixel<WIDE>(src, sh, sw, lim_u, lim_v, e[2 * j], e[2 * j + 1], fill);
        resample::store_px4(o, px, PX);
    } else {
        for (int j = 0; j < npx; ++j)                               // c0 + j < dw: nothing past the row's end is read or written
            resample::store_px1(o + j * 3, remap_pixel<WIDE>(src, sh, sw, lim_u, lim_v, mp[2 * j], mp[2 * j + 1], fill));
    }
}

bool finite4(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3]); }

}  // namespace

extern "C" int av_lens_make(const double K[4], const double dist[5], const double new_K[4], int w, int h, av_lens_cfg* out) {
    AV_REQUIRE(K && dist && out, AV_EINVAL, "av_lens_make: null argument");
    const double* N = new_K ? new_K : K;
    AV_REQUIRE(finite4(K) && finite4(N), AV_EINVAL, "av_lens_make: an intrinsic is not finite");
    for (int i = 0; i < 5; ++i) AV_REQUIRE(std::isfinite(dist[i]), AV_EINVAL, "av_lens_make: dist[%d] is not finite", i);
    AV_REQUIRE(K[0] > 0.0 && K[1] > 0.0 && N[0] > 0.0 && N[1] > 0.0, AV_EINVAL, "av_lens_make: focal lengths must be > 0");
    AV_REQUIRE(w >= 1 && h >= 1 && w <= MAX_SIDE && h <= MAX_SIDE, AV_EINVAL, "av_lens_make: frame size %d x %d not in 1 .. %d", w, h,
               MAX_SIDE);
    // the radial map r -> r rad(r^2) must be increasing out to the farthest corner of the rectified frame
    double rmax = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double x = ((i & 1 ? (double)(w - 1) : 0.0) - N[2]) / N[0], y = ((i & 2 ? (double)(h - 1) : 0.0) - N[3]) / N[1];
        rmax = std::fmax(rmax, std::sqrt(x * x + y * y));
    }
    AV_REQUIRE(std::isfinite(rmax), AV_EINVAL, "av_lens_make: the rectified frame's corners are not finite");
    const double k1 = dist[0], k2 = dist[1], k3 = dist[4];
    for (int i = 1; i <= 1024; ++i) {
        const double r = rmax * (double)i / 1024.0, r2 = r * r;
        const double q = 1 + r2 * (3 * k1 + r2 * (5 * k2 + r2 * (7 * k3)));
        AV_REQUIRE(q > 0.0, AV_EINVAL,
                   "av_lens_make: the model folds over inside the rectified frame (radial derivative %.3g at normalised radius %.4g of %.4g)",
                   q, r, rmax);
    }
    out->fx = K[0], out->fy = K[1], out->cx = K[2], out->cy = K[3];
    out->k1 = dist[0], out->k2 = dist[1], out->p1 = dist[2], out->p2 = dist[3], out->k3 = dist[4];
    out->nfx = N[0], out->nfy = N[1], out->ncx = N[2], out->ncy = N[3];
    out->w = w, out->h = h;
    return AV_OK;
}

extern "C" int av_lens_map_rectify(av_ctx* ctx, av_stream_t stream, const av_lens_cfg* lens, int n_maps, int h, int w, int32_t* map) {
    AV_REQUIRE(ctx && lens && map, AV_EINVAL, "av_lens_map_rectify: null argument");
    AV_REQUIRE(n_maps >= 1 && h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE, AV_EINVAL,
               "av_lens_map_rectify: n_maps must be >= 1, h and w in 1 .. %d", MAX_SIDE);
    dim3 grid;
    if (int rc = resample::tile_grid(w, h, n_maps, "av_lens_map_rectify", "maps", &grid)) return rc;
    hipLaunchKernelGGL(lens_map_rectify_kernel, grid, dim3(256), 0, as_stream(stream), lens, h, w, map);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_lens_map_ground(av_ctx* ctx, av_stream_t stream, const av_lens_cfg* lens, const av_ground_cfg* ground, int n_maps,
                                  int gh, int gw, double f_far, double m_per_px, int32_t* map) {
    AV_REQUIRE(ctx && lens && ground && map, AV_EINVAL, "av_lens_map_ground: null argument");
    AV_REQUIRE(n_maps >= 1 && gh >= 1 && gw >= 1, AV_EINVAL, "av_lens_map_ground: n_maps, gh and gw must be >= 1");
    AV_REQUIRE(m_per_px > 0.0 && std::isfinite(m_per_px) && std::isfinite(f_far), AV_EINVAL,
               "av_lens_map_ground: m_per_px must be > 0 and finite, f_far finite");
    dim3 grid;
    if (int rc = resample::tile_grid(gw, gh, n_maps, "av_lens_map_ground", "maps", &grid)) return rc;
    hipLaunchKernelGGL(lens_map_ground_kernel, grid, dim3(256), 0, as_stream(stream), lens, ground, gh, gw, f_far, m_per_px, map);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_remap(av_ctx* ctx, av_stream_t stream, const int32_t* map, int n_cams, int cam_stride, int sh, int sw,
                        const uint8_t* bgr, int dh, int dw, const uint8_t fill[3], uint8_t* out) {
    AV_REQUIRE(ctx && map && bgr && fill && out, AV_EINVAL, "av_remap: null argument");
    AV_REQUIRE(n_cams >= 1 && dh >= 1 && dw >= 1, AV_EINVAL, "av_remap: n_cams, dh and dw must be >= 1");
    AV_REQUIRE(sh >= 1 && sw >= 1 && sh <= MAX_SIDE && sw <= MAX_SIDE, AV_EINVAL, "av_remap: sh and sw must be in 1 .. %d", MAX_SIDE);
    AV_REQUIRE(cam_stride >= 1, AV_EINVAL, "av_remap: cam_stride must be >= 1");
    dim3 grid;
    if (int rc = resample::tile_grid(dw, dh, n_cams, "av_remap", "cameras", &grid)) return rc;
    const size_t out_bytes = (size_t)n_cams * dh * dw * 3, n_maps = ((size_t)n_cams + cam_stride - 1) / cam_stride;
    AV_REQUIRE(!resample::overlap(out, out_bytes, bgr, (size_t)n_cams * sh * sw * 3), AV_EINVAL, "av_remap: out overlaps bgr");
    AV_REQUIRE(!resample::overlap(out, out_bytes, map, n_maps * dh * dw * 8), AV_EINVAL, "av_remap: out overlaps map");
    const unsigned fc = resample::pack_bgr(fill);
    const auto kernel = sw >= 2 ? remap_kernel<true> : remap_kernel<false>;      // a source one pixel wide: tap by tap
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), map, cam_stride, sh, sw, bgr, dh, dw, fc, out);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
