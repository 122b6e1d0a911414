// Road memory (include/avhot.h: av_roadmem_*): a world-anchored rolling canvas per vehicle that takes every frame's seen pixels of
// the surround panel through the pose the odometry measured, and gives the panel's unseen pixels back out of it.  The header
// states every stage's arithmetic; DESIGN.md 7u has the layout and the measurements.
//
//   pose    one thread per vehicle: the odometry's (x, y, psi) and mode -> (x, y, cos, sin, reset)
//   update  one thread per canvas cell, a workgroup 16 x 16 STORAGE cells: the thread at [a][b] finds the one world cell of the new
//           window that lives there, so the stores are in storage order and no tile meets the torus seam.  A cell that neither
//           entered nor is seen leaves without a load or a store; one that entered unseen stores its stamp and loads nothing.
//           A seen cell gathers four cover bytes and its panel taps (resample_dev.h's sample) and stores two words.
//           A second, one-wave launch writes the new state behind it: every workgroup of the first reads the old one.
//   fill    resample_dev.h's tile (four adjacent panel pixels a thread); a thread whose pixels are all covered writes their ages
//           and leaves, the others read four stamps and, where remembered, four cells per uncovered pixel.
// What is the same for a vehicle (pose, origins, F) is read through scalar loads.  No LDS.
#include "common.h"
#include "resample_dev.h"

#include <cmath>

namespace {

using resample::PX;
constexpr int CELL_TILE = 16;
constexpr double POSE_LIMIT = 1073741824.0;     // 2^30 cells

// i mod n, non-negative
__host__ __device__ __forceinline__ int pmod(int i, int n) {
    const int r = i % n;
    return r < 0 ? r + n : r;
}

struct Window {
    int i0, j0;
    bool bad;       // the pose is out of range (a NaN among them)
};
__device__ __forceinline__ Window window_of(double x, double y, double m, int n) {
    const double qx = x / m, qy = y / m;
    Window w;
    w.bad = !(fabs(qx) <= POSE_LIMIT && fabs(qy) <= POSE_LIMIT);
    w.i0 = w.bad ? 0 : (int)floor(qx) - n / 2;
    w.j0 = w.bad ? 0 : (int)floor(qy) - n / 2;
    return w;
}

// ---- stage 1: pose -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) roadmem_pose_kernel(int n_vehicles, const av_egoflow_state* __restrict__ state,
                                                          const uint8_t* __restrict__ mode, av_roadmem_pose* __restrict__ pose) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= n_vehicles) return;
    const av_egoflow_state s = state[v];
    av_roadmem_pose p;
    p.x = s.x, p.y = s.y, p.cs = cos(s.psi), p.sn = sin(s.psi);
    p.reset = mode != nullptr && mode[v] == 2, p.reserved = 0;
    pose[v] = p;
}

// ---- stage 2: update -----------------------------------------------------------------------------------------------------------
template <bool WIDE>        // WIDE: the panel is at least two pixels wide, the sample's packed form
__global__ void __launch_bounds__(256) roadmem_update_kernel(int n, double m, int gh, int gw, double x_far, double pm,
                                                             const av_roadmem_pose* __restrict__ pose, const uint8_t* __restrict__ panel,
                                                             const uint8_t* __restrict__ cover, const av_roadmem_state* __restrict__ state,
                                                             uint32_t* __restrict__ canvas, uint32_t* __restrict__ stamp) {
    const int veh = blockIdx.z;
    // the same for the whole workgroup: scalar loads
    const av_roadmem_pose p = pose[veh];
    const av_roadmem_state s = state[veh];
    const Window w = window_of(p.x, p.y, m, n);
    if (w.bad) return;
    const bool fresh = p.reset != 0 || s.frames == 0;
    const unsigned F = fresh ? 1u : (unsigned)s.frames + 1u;
    const int ra = pmod(w.i0, n), rb = pmod(w.j0, n);
    // the world cell of the new window that lives at [a][b]
    const int a = blockIdx.y * CELL_TILE + (int)(threadIdx.x / CELL_TILE), b = blockIdx.x * CELL_TILE + (int)(threadIdx.x % CELL_TILE);
    const int i = w.i0 + (a - ra) + (a < ra ? n : 0), j = w.j0 + (b - rb) + (b < rb ? n : 0);
    const bool entered = fresh || i < s.i0 || (long long)i >= (long long)s.i0 + n || j < s.j0 || (long long)j >= (long long)s.j0 + n;
    const double xc = ((double)i + 0.5) * m, yc = ((double)j + 0.5) * m;
    const double dx = xc - p.x, dy = yc - p.y;
    const double X = p.cs * dx + p.sn * dy, Y = p.cs * dy - p.sn * dx;
    const double pr = (x_far - X) / pm - 0.5, pc = Y / pm + (double)gw / 2.0 - 0.5;
    const double tr = floor(pr * 65536.0 + 0.5), tc = floor(pc * 65536.0 + 0.5);
    const size_t at = ((size_t)veh * n + a) * n + b;                // a, b < n: n is a multiple of the tile
    if (tr >= 0.0 && tr <= (double)(gh - 1) * 65536.0 && tc >= 0.0 && tc <= (double)(gw - 1) * 65536.0) {
        const long long itr = (long long)tr, itc = (long long)tc;
        const int r0 = (int)(itr >> 16), c0 = (int)(itc >> 16), r1 = min(r0 + 1, gh - 1), c1 = min(c0 + 1, gw - 1);
        const uint8_t* cv = cover + (size_t)veh * gh * gw;
        const unsigned c00 = cv[(size_t)r0 * gw + c0], c01 = cv[(size_t)r0 * gw + c1], c10 = cv[(size_t)r1 * gw + c0],
                       c11 = cv[(size_t)r1 * gw + c1];
        if (c00 != 0u && c01 != 0u && c10 != 0u && c11 != 0u) {
            canvas[at] = resample::bilinear_bgr<WIDE>(panel + (size_t)veh * gh * gw * 3, gh, gw, itc, itr);
            stamp[at] = F;
            return;
        }
    }
    if (entered) stamp[at] = 0u;
}

// the new state, behind the cells
__global__ void __launch_bounds__(64) roadmem_commit_kernel(int n_vehicles, int n, double m, const av_roadmem_pose* __restrict__ pose,
                                                            av_roadmem_state* __restrict__ state) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= n_vehicles) return;
    const av_roadmem_pose p = pose[v];
    const av_roadmem_state s = state[v];
    const Window w = window_of(p.x, p.y, m, n);
    av_roadmem_state o;
    o.i0 = w.i0, o.j0 = w.j0, o.status = w.bad ? 1 : 0;
    o.frames = w.bad ? 0 : (p.reset != 0 || s.frames == 0) ? 1 : s.frames + 1;
    state[v] = o;
}

// ---- stage 3: fill -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) roadmem_fill_kernel(int n, int max_age, double m, int gh, int gw, double x_far, double pm,
                                                           unsigned fill, const av_roadmem_pose* __restrict__ pose,
                                                           const av_roadmem_state* __restrict__ state, const uint32_t* __restrict__ canvas,
                                                           const uint32_t* __restrict__ stamp, const uint8_t* __restrict__ cover,
                                                           uint8_t* __restrict__ panel, uint8_t* __restrict__ age) {
    const int veh = blockIdx.z;
    int r, c0, npx;
    if (!resample::tile_thread(gh, gw, r, c0, npx)) return;
    const size_t at = ((size_t)veh * gh + r) * gw + c0;             // r < gh, c0 + npx <= gw
    const bool four = gw % PX == 0;                                 // every thread has four pixels, 4-byte aligned
    unsigned cv[PX] = {1u, 1u, 1u, 1u};
    if (four) {
        unsigned word;
        __builtin_memcpy(&word, cover + at, 4);
#pragma unroll
        for (int k = 0; k < PX; ++k) cv[k] = (word >> (8 * k)) & 255u;
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k)
            if (k < npx) cv[k] = cover[at + k];
    }
    unsigned ag[PX] = {0u, 0u, 0u, 0u}, px[PX] = {0u, 0u, 0u, 0u};
    if (cv[0] == 0u || cv[1] == 0u || cv[2] == 0u || cv[3] == 0u) {
        // the same for the whole workgroup: scalar loads
        const av_roadmem_pose p = pose[veh];
        const av_roadmem_state s = state[veh];
        const unsigned F = (unsigned)s.frames;
        const int ra = pmod(s.i0, n), rb = pmod(s.j0, n);
        const double lo_i = (double)s.i0 * 65536.0, hi_i = ((double)s.i0 + (double)(n - 1)) * 65536.0;
        const double lo_j = (double)s.j0 * 65536.0, hi_j = ((double)s.j0 + (double)(n - 1)) * 65536.0;
        const uint32_t* cnv = canvas + (size_t)veh * n * n;
        const uint32_t* stp = stamp + (size_t)veh * n * n;
        const double X = x_far - ((double)r + 0.5) * pm;
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            if (cv[k] != 0u) continue;                              // (a column past the row's end counts as covered)
            px[k] = fill, ag[k] = 255u;
            const double Y = (((double)(c0 + k) + 0.5) - (double)gw / 2.0) * pm;
            const double xw = (p.x + p.cs * X) - p.sn * Y, yw = (p.y + p.sn * X) + p.cs * Y;
            const double ti = floor((xw / m - 0.5) * 65536.0 + 0.5), tj = floor((yw / m - 0.5) * 65536.0 + 0.5);
            if (!(F != 0u && ti >= lo_i && ti < hi_i && tj >= lo_j && tj < hi_j)) continue;
            const long long iti = (long long)ti, itj = (long long)tj;           // within the window: below 2^47
            const unsigned wi = (unsigned)(iti & 65535), wj = (unsigned)(itj & 65535);
            int sa = ra + (int)((iti >> 16) - s.i0), sb = rb + (int)((itj >> 16) - s.j0);       // 0 .. 2 n - 3
            sa = sa >= n ? sa - n : sa, sb = sb >= n ? sb - n : sb;
            const int sa1 = sa + 1 >= n ? 0 : sa + 1, sb1 = sb + 1 >= n ? 0 : sb + 1;
            const size_t q00 = (size_t)sa * n + sb, q01 = (size_t)sa * n + sb1, q10 = (size_t)sa1 * n + sb, q11 = (size_t)sa1 * n + sb1;
            const unsigned s00 = stp[q00], s01 = stp[q01], s10 = stp[q10], s11 = stp[q11];
            const unsigned old = F - min(min(s00, s01), min(s10, s11));
            if (s00 == 0u || s01 == 0u || s10 == 0u || s11 == 0u || old > (unsigned)max_age) continue;
            const unsigned p00 = cnv[q00], p01 = cnv[q01], p10 = cnv[q10], p11 = cnv[q11];
            unsigned out = 0u;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                out |= resample::blend((p00 >> (8 * ch)) & 255u, (p01 >> (8 * ch)) & 255u, (p10 >> (8 * ch)) & 255u,
                                       (p11 >> (8 * ch)) & 255u, wj, wi) << (8 * ch);
            px[k] = out, ag[k] = min(old, 254u);
        }
        uint8_t* o = panel + at * 3;
        if (four && (cv[0] | cv[1] | cv[2] | cv[3]) == 0u) {
            resample::store_px4(o, px, PX);
        } else {
#pragma unroll
            for (int k = 0; k < PX; ++k)
                if (cv[k] == 0u) resample::store_px1(o + k * 3, px[k]);
        }
    }
    if (four) {
        const unsigned word = ag[0] | (ag[1] << 8) | (ag[2] << 16) | (ag[3] << 24);
        __builtin_memcpy(age + at, &word, 4);
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k)
            if (k < npx) age[at + k] = (uint8_t)ag[k];
    }
}

// ---- checks and launches -------------------------------------------------------------------------------------------------------
int check_cfg(const av_roadmem_cfg* c, const char* who) {
    static_assert(sizeof(av_roadmem_cfg) == 48 && sizeof(av_roadmem_state) == 16 && sizeof(av_roadmem_pose) == 40, "av_roadmem layouts");
    AV_REQUIRE(c, AV_EINVAL, "%s: null cfg", who);
    AV_REQUIRE(c->n >= 16 && c->n <= 4096 && c->n % CELL_TILE == 0, AV_EINVAL, "%s: cfg n %d is not a multiple of 16 in 16..4096", who, c->n);
    AV_REQUIRE(c->max_age >= 0, AV_EINVAL, "%s: cfg max_age must be >= 0", who);
    AV_REQUIRE(c->m_per_px > 0.0 && std::isfinite(c->m_per_px), AV_EINVAL, "%s: cfg m_per_px must be > 0 and finite", who);
    AV_REQUIRE(c->panel_m_per_px > 0.0 && std::isfinite(c->panel_m_per_px), AV_EINVAL, "%s: cfg panel_m_per_px must be > 0 and finite", who);
    AV_REQUIRE(std::isfinite(c->x_far), AV_EINVAL, "%s: cfg x_far must be finite", who);
    AV_REQUIRE(c->gh >= 1 && c->gw >= 1, AV_EINVAL, "%s: cfg gh and gw must be >= 1", who);
    for (int k = 0; k < 5; ++k) AV_REQUIRE(c->reserved[k] == 0, AV_EINVAL, "%s: cfg reserved must be 0", who);
    return AV_OK;
}

int check_vehicles(int n_vehicles, const char* who) {
    AV_REQUIRE(n_vehicles >= 1 && n_vehicles <= 65535, AV_EINVAL, "%s: n_vehicles %d not in 1..65535", who, n_vehicles);
    return AV_OK;
}

// does the panel share a byte with the canvas or the stamps?
int check_apart(const av_roadmem_cfg* c, int n_vehicles, const void* panel, const void* canvas, const void* stamp, const char* who) {
    const unsigned __int128 pb = (unsigned __int128)n_vehicles * c->gh * c->gw * 3, cb = (unsigned __int128)n_vehicles * c->n * c->n * 4;
    AV_REQUIRE(!resample::overlap(panel, pb, canvas, cb), AV_EINVAL, "%s: panel overlaps canvas", who);
    AV_REQUIRE(!resample::overlap(panel, pb, stamp, cb), AV_EINVAL, "%s: panel overlaps stamp", who);
    return AV_OK;
}

int launch_pose(av_stream_t stream, int n_vehicles, const av_egoflow_state* state, const uint8_t* mode, av_roadmem_pose* pose) {
    hipLaunchKernelGGL(roadmem_pose_kernel, dim3((unsigned)((n_vehicles + 63) / 64)), dim3(64), 0, as_stream(stream), n_vehicles, state,
                       mode, pose);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int launch_update(av_stream_t stream, const av_roadmem_cfg* c, int n_vehicles, const av_roadmem_pose* pose, const uint8_t* panel,
                  const uint8_t* cover, av_roadmem_state* state, uint8_t* canvas, uint32_t* stamp) {
    const dim3 grid((unsigned)(c->n / CELL_TILE), (unsigned)(c->n / CELL_TILE), (unsigned)n_vehicles);
    hipLaunchKernelGGL(c->gw >= 2 ? roadmem_update_kernel<true> : roadmem_update_kernel<false>, grid, dim3(256), 0, as_stream(stream),
                       c->n, c->m_per_px, c->gh, c->gw, c->x_far, c->panel_m_per_px, pose, panel, cover, state,
                       reinterpret_cast<uint32_t*>(canvas), stamp);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(roadmem_commit_kernel, dim3((unsigned)((n_vehicles + 63) / 64)), dim3(64), 0, as_stream(stream), n_vehicles, c->n,
                       c->m_per_px, pose, state);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int launch_fill(av_stream_t stream, const av_roadmem_cfg* c, const dim3& grid, const av_roadmem_pose* pose, const av_roadmem_state* state,
                const uint8_t* canvas, const uint32_t* stamp, const uint8_t* cover, uint8_t* panel, uint8_t* age) {
    hipLaunchKernelGGL(roadmem_fill_kernel, grid, dim3(256), 0, as_stream(stream), c->n, c->max_age, c->m_per_px, c->gh, c->gw, c->x_far,
                       c->panel_m_per_px, resample::pack_bgr(c->fill), pose, state, reinterpret_cast<const uint32_t*>(canvas), stamp,
                       cover, panel, age);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // namespace

extern "C" int av_roadmem_check(const av_roadmem_cfg* cfg) { return check_cfg(cfg, "av_roadmem_check"); }

extern "C" int av_roadmem_pose_from(av_ctx* ctx, av_stream_t stream, int n_vehicles, const av_egoflow_state* state, const uint8_t* mode,
                                    av_roadmem_pose* pose) {
    if (int rc = check_vehicles(n_vehicles, "av_roadmem_pose_from")) return rc;
    AV_REQUIRE(ctx && state && pose, AV_EINVAL, "av_roadmem_pose_from: null argument");
    return launch_pose(stream, n_vehicles, state, mode, pose);
}

extern "C" int av_roadmem_update(av_ctx* ctx, av_stream_t stream, const av_roadmem_cfg* cfg, int n_vehicles, const av_roadmem_pose* pose,
                                 const uint8_t* panel, const uint8_t* cover, av_roadmem_state* state, uint8_t* canvas, uint32_t* stamp) {
    if (int rc = check_cfg(cfg, "av_roadmem_update")) return rc;
    if (int rc = check_vehicles(n_vehicles, "av_roadmem_update")) return rc;
    AV_REQUIRE(ctx && pose && panel && cover && state && canvas && stamp, AV_EINVAL, "av_roadmem_update: null argument");
    if (int rc = check_apart(cfg, n_vehicles, panel, canvas, stamp, "av_roadmem_update")) return rc;
    return launch_update(stream, cfg, n_vehicles, pose, panel, cover, state, canvas, stamp);
}

extern "C" int av_roadmem_fill(av_ctx* ctx, av_stream_t stream, const av_roadmem_cfg* cfg, int n_vehicles, const av_roadmem_pose* pose,
                               const av_roadmem_state* state, const uint8_t* canvas, const uint32_t* stamp, const uint8_t* cover,
                               uint8_t* panel, uint8_t* age) {
    if (int rc = check_cfg(cfg, "av_roadmem_fill")) return rc;
    if (int rc = check_vehicles(n_vehicles, "av_roadmem_fill")) return rc;
    dim3 grid;
    if (int rc = resample::tile_grid(cfg->gw, cfg->gh, n_vehicles, "av_roadmem_fill", "vehicles", &grid)) return rc;
    AV_REQUIRE(ctx && pose && state && canvas && stamp && cover && panel && age, AV_EINVAL, "av_roadmem_fill: null argument");
    if (int rc = check_apart(cfg, n_vehicles, panel, canvas, stamp, "av_roadmem_fill")) return rc;
    return launch_fill(stream, cfg, grid, pose, state, canvas, stamp, cover, panel, age);
}

extern "C" int av_roadmem_step(av_ctx* ctx, av_stream_t stream, const av_roadmem_cfg* cfg, int n_vehicles, const av_egoflow_state* ego_state,
                               const uint8_t* mode, av_roadmem_pose* pose, uint8_t* panel, const uint8_t* cover, av_roadmem_state* state,
                               uint8_t* canvas, uint32_t* stamp, uint8_t* age) {
    if (int rc = check_cfg(cfg, "av_roadmem_step")) return rc;
    if (int rc = check_vehicles(n_vehicles, "av_roadmem_step")) return rc;
    dim3 grid;
    if (int rc = resample::tile_grid(cfg->gw, cfg->gh, n_vehicles, "av_roadmem_step", "vehicles", &grid)) return rc;
    AV_REQUIRE(ctx && ego_state && pose && panel && cover && state && canvas && stamp && age, AV_EINVAL, "av_roadmem_step: null argument");
    if (int rc = check_apart(cfg, n_vehicles, panel, canvas, stamp, "av_roadmem_step")) return rc;
    if (int rc = launch_pose(stream, n_vehicles, ego_state, mode, pose)) return rc;
    if (int rc = launch_update(stream, cfg, n_vehicles, pose, panel, cover, state, canvas, stamp)) return rc;
    return launch_fill(stream, cfg, grid, pose, state, canvas, stamp, cover, panel, age);
}

extern "C" int av_roadmem_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int vehicle, av_roadmem_state* state) {
    if (int rc = check_vehicles(n_vehicles, "av_roadmem_reset")) return rc;
    AV_REQUIRE(vehicle >= -1 && vehicle < n_vehicles, AV_EINVAL, "av_roadmem_reset: vehicle %d is neither -1 nor in 0..%d", vehicle,
               n_vehicles - 1);
    AV_REQUIRE(ctx && state, AV_EINVAL, "av_roadmem_reset: null argument");
    if (vehicle < 0) AV_HIP(hipMemsetAsync(state, 0, sizeof(av_roadmem_state) * (size_t)n_vehicles, as_stream(stream)));
    else AV_HIP(hipMemsetAsync(state + vehicle, 0, sizeof(av_roadmem_state), as_stream(stream)));
    return AV_OK;
}
