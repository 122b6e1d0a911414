// The rig's surround view: the rectified frames of a vehicle's K cameras stitched into one top-down panel in the VEHICLE's road
// frame (av_rig_surround, include/avhot.h).  av_ground_warp makes one panel per camera, each in its own camera's road frame; here
// a panel pixel's road point goes through every camera's mount (rig.hip's table, the other way round: CameraRig.from_vehicle) and
// ginv, and the cameras that see it are blended (feather: weights that fall to one at the frame's border, so a seam fades instead
// of cutting) or the nearest one is taken.
//
// resample_dev.h's tile and store: a thread makes four adjacent pixels of one panel row, and stores their cover bytes as 4 at once
// when the rows are a multiple of four wide; neighbouring panel pixels read neighbouring source pixels of whichever camera sees
// them.  grid.z is the vehicle; the loop over the K cameras runs inside the thread, with the four pixels' running sums in
// registers, and a camera's mount, ginv and max_range are the same for the whole workgroup: scalar loads.  No LDS.  The per-pixel
// position and sample are ground_dev.h's, which av_ground_warp uses too.
#include "common.h"
#include "ground_dev.h"

#include <cmath>

namespace {

using resample::PX;
constexpr int MAX_CAMS = 8, MAX_SIDE = 32768;

// the four pixels and their cover bytes
__device__ __forceinline__ void store_pixels(uint8_t* __restrict__ o, uint8_t* __restrict__ cv, const unsigned (&px)[PX],
                                             const unsigned (&mask)[PX], int npx, bool cover4) {
    resample::store_px4(o, px, npx);
    if (!cv) return;
    if (cover4) {                                                   // gw % 4 == 0: every thread has four pixels
        const unsigned word = mask[0] | (mask[1] << 8) | (mask[2] << 16) | (mask[3] << 24);
        __builtin_memcpy(cv, &word, 4);
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j)
            if (j < npx) cv[j] = (uint8_t)mask[j];
    }
}

template <bool NEAREST, bool WIDE>        // WIDE: the frames are at least two pixels wide, the sample's packed form
__global__ void __launch_bounds__(256) rig_surround_kernel(int n_cams, const av_rig_mount* __restrict__ mounts,
                                                           const av_ground_cfg* __restrict__ ground, int h, int w,
                                                           const uint8_t* __restrict__ bgr, int gh, int gw, double x_far, double m_per_px,
                                                           unsigned fill, uint8_t* __restrict__ out, uint8_t* __restrict__ cover) {
    const int veh = blockIdx.z;
    int r, c0, npx;
    if (!resample::tile_thread(gh, gw, r, c0, npx)) return;
    const size_t frame = (size_t)h * w * 3;
    const double X = x_far - ((double)r + 0.5) * m_per_px;
    double Y[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) Y[j] = (((double)(c0 + j) + 0.5) - (double)gw / 2.0) * m_per_px;
    const long long lim_u = (long long)(w - 1) << 16, lim_v = (long long)(h - 1) << 16;
    unsigned mask[PX] = {0u, 0u, 0u, 0u}, px[PX];
    // feather: the sums of the weights and of weight x channel; nearest: the winner's distance, camera and frame position
    unsigned sw[PX] = {0u, 0u, 0u, 0u}, sp[PX][3] = {}, last[PX] = {0u, 0u, 0u, 0u};
    double best[PX];
    long long bu[PX], bv[PX];
    int bk[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) best[j] = 0.0, bu[j] = bv[j] = 0, bk[j] = 0;
    for (int k = 0; k < n_cams; ++k) {
        // the same for the whole workgroup: scalar loads
        const av_rig_mount m = mounts[(size_t)veh * n_cams + k];
        const av_ground_cfg& g = ground[(size_t)veh * n_cams + k];
        const double* q = g.ginv;
        const double max_range = g.max_range;
        const uint8_t* src = bgr + ((size_t)veh * n_cams + k) * frame;
        const double dx = X - m.x;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            if (j >= npx) continue;                                 // (a column past the row's end is not computed)
            const double dy = Y[j] - m.y;
            const double f = m.c * dx + m.s * dy, l = m.c * dy - m.s * dx;
            if (!(f >= 0.0 && f <= max_range)) continue;
            {
                // most cameras do not see the pixel: a point more than a whole pixel outside the frame is refused before the two
                // divisions (with D > 0, U < -D is u < -1 and U > w D is u > w - 1 + 1/2, whatever the quotient's rounding; a NaN
                // passes on to the full test); the sums are warp_position's own, which the compiler computes once
                const double U = (q[0] * f + q[1] * l) + q[2], V = (q[3] * f + q[4] * l) + q[5], D = (q[6] * f + q[7] * l) + q[8];
                if (!(D > 0.0) || U < -D || U > (double)w * D || V < -D || V > (double)h * D) continue;
            }
            long long iu, iv;
            if (!grounddev::warp_position(q, h, w, f, l, iu, iv)) continue;
            if constexpr (NEAREST) {
                const double d2 = f * f + l * l;
                if (mask[j] == 0u || d2 < best[j]) best[j] = d2, bu[j] = iu, bv[j] = iv, bk[j] = k;    // equal d2: the smaller k stays
            } else {
                const unsigned p = grounddev::warp_sample<WIDE>(src, h, w, iu, iv);
                const long long eu = min(iu, lim_u - iu), ev = min(iv, lim_v - iv);
                const unsigned wt = (unsigned)(min(eu, ev) >> 16) + 1u;                    // 1 .. 16384
                sw[j] += wt, last[j] = p;
                sp[j][0] += wt * (p & 255u), sp[j][1] += wt * ((p >> 8) & 255u), sp[j][2] += wt * (p >> 16);
            }
            mask[j] |= 1u << k;
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        px[j] = fill;
        if (mask[j] == 0u) continue;
        if constexpr (NEAREST) {
            px[j] = grounddev::warp_sample<WIDE>(bgr + ((size_t)veh * n_cams + bk[j]) * frame, h, w, bu[j], bv[j]);
        } else {
            const unsigned d = 2u * sw[j];                                                  // <= 2 x 8 x 16384
            // one camera alone (most of a panel): (2 wt p + wt) / (2 wt) is p itself, without the three divisions
            px[j] = (mask[j] & (mask[j] - 1u)) == 0u
                        ? last[j]
                        : ((2u * sp[j][0] + sw[j]) / d) | (((2u * sp[j][1] + sw[j]) / d) << 8) | (((2u * sp[j][2] + sw[j]) / d) << 16);
        }
    }
    const size_t at = ((size_t)veh * gh + r) * gw + c0;              // r < gh, c0 + npx <= gw
    store_pixels(out + at * 3, cover ? cover + at : nullptr, px, mask, npx, gw % PX == 0);
}

}  // namespace

extern "C" int av_rig_surround(av_ctx* ctx, av_stream_t stream, const av_surround_cfg* cfg, int n_vehicles, int n_cams,
                               const av_rig_mount* mounts, const av_ground_cfg* ground, int h, int w, const uint8_t* bgr, int gh, int gw,
                               uint8_t* out, uint8_t* cover) {
    static_assert(sizeof(av_surround_cfg) == 24, "av_surround_cfg layout");
    AV_REQUIRE(n_vehicles >= 1, AV_EINVAL, "av_rig_surround: n_vehicles must be >= 1");
    AV_REQUIRE(n_cams >= 1 && n_cams <= MAX_CAMS, AV_EINVAL, "av_rig_surround: n_cams %d not in 1..%d", n_cams, MAX_CAMS);
    AV_REQUIRE(h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE, AV_EINVAL, "av_rig_surround: frame size h %d, w %d not in 1..%d", h, w,
               MAX_SIDE);
    AV_REQUIRE(gh >= 1 && gw >= 1, AV_EINVAL, "av_rig_surround: panel size gh and gw must be >= 1");
    dim3 grid;
    if (int rc = resample::tile_grid(gw, gh, n_vehicles, "av_rig_surround", "vehicles", &grid)) return rc;
    AV_REQUIRE(cfg, AV_EINVAL, "av_rig_surround: null cfg");
    AV_REQUIRE(cfg->m_per_px > 0.0 && std::isfinite(cfg->m_per_px), AV_EINVAL, "av_rig_surround: cfg m_per_px must be > 0 and finite");
    AV_REQUIRE(std::isfinite(cfg->x_far), AV_EINVAL, "av_rig_surround: cfg x_far must be finite");
    AV_REQUIRE(cfg->blend == 0 || cfg->blend == 1, AV_EINVAL, "av_rig_surround: cfg blend %d is neither 0 (feather) nor 1 (nearest)",
               cfg->blend);
    AV_REQUIRE(cfg->reserved == 0, AV_EINVAL, "av_rig_surround: cfg reserved must be 0");
    AV_REQUIRE(ctx && mounts && ground && bgr && out, AV_EINVAL, "av_rig_surround: null argument");
    {
        const unsigned __int128 panel = (unsigned __int128)n_vehicles * gh * gw, frames = (unsigned __int128)n_vehicles * n_cams * h * w * 3;
        AV_REQUIRE(!resample::overlap(out, panel * 3, bgr, frames), AV_EINVAL, "av_rig_surround: out overlaps bgr");
        AV_REQUIRE(!cover || !resample::overlap(cover, panel, bgr, frames), AV_EINVAL, "av_rig_surround: cover overlaps bgr");
    }
    const auto kernel = cfg->blend == 1 ? (w >= 2 ? rig_surround_kernel<true, true> : rig_surround_kernel<true, false>)
                                        : (w >= 2 ? rig_surround_kernel<false, true> : rig_surround_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), n_cams, mounts, ground, h, w, bgr, gh, gw,
                       cfg->x_far, cfg->m_per_px, resample::pack_bgr(cfg->fill), out, cover);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
