// Ground odometry (include/avhot.h: av_egoflow_*): the ego measurement of the Kalman stage from the road pixels of two
// consecutive frames.  The reference makes that measurement up on the host (video_loader.py:166-205); here it is measured:
//   patch    frames -> a gray bird's-eye patch per camera through the ground-plane homography (ground_dev.h's position rule and
//            bilinear sample, the lane front end's gray), with a validity bit per pixel
//   match    block matching of T x T tiles of the current patch in the previous one, sums of absolute differences over
//            (2R+1)^2 candidates per tile: the hot kernel
//   solve    vote, gate, least-squares rigid motion with one rejection round: one wave per camera
//   measure  pose integration and the (z, mode) the Kalman stage reads
// The header states every stage's arithmetic; DESIGN.md 7s has the layout and the measurements.  egoflow_dev.h declares what
// rigflow.hip (a rig's cameras fitted together) shares: the checked geometry, the patch, match and measure launches,
// and the solve's pieces.
//
// match, mapping: one wave per tile, four tiles per workgroup, each wave with its own LDS region and no data shared between waves:
//   cur  T*T bytes          the tile, packed four pixels to a word
//   win  (T+2R) rows of WP bytes (WP = T+2R rounded up to a word) + one word: the tile's neighbourhood in the previous patch
//   sad  (2R+1)^2 ints      every candidate's SAD (the sub-pixel step reads the best one's neighbours)
// Lane c, c + 64, ... takes candidate c = (dy + R) * (2R+1) + (dx + R), each with an accumulator of its own in a register (at most
// 16).  The tile's rows are the outer loop: a row's T/4 words are read once (one address for the whole wave, a broadcast) and kept
// in registers for all of the lane's candidates; per candidate the lane reads T/4 + 1 aligned words of the window row under it and
// shifts neighbouring pairs by (dx + R) & 3 bytes (v_alignbyte_b32) into the T/4 words under the tile, and v_sad_u8 adds four
// absolute differences to the candidate's accumulator.  Lanes with consecutive dx read the same or adjacent words of one window row.
// The kernel is a template over T/4 so that these loops unroll.  The argmin is a wave minimum of (SAD << 10 | c): the smallest SAD,
// and among equals the smallest c, which is the first in row-major (dy, dx) order.
#include "egoflow_dev.h"
#include "ground_dev.h"

#include <cmath>

namespace egoflow {

int geometry(const av_egoflow_cfg* c, const char* who, Geom* g) {
    AV_REQUIRE(c, AV_EINVAL, "%s: null cfg", who);
    AV_REQUIRE(c->gh >= 1 && c->gw >= 1 && c->gh <= MAX_SIDE && c->gw <= MAX_SIDE, AV_EINVAL, "%s: gh and gw must be 1 .. %d", who,
               MAX_SIDE);
    AV_REQUIRE(c->tile >= 4 && c->tile <= MAX_T && c->tile % 4 == 0, AV_EINVAL, "%s: tile %d is not a multiple of 4 in 4 .. %d", who,
               c->tile, MAX_T);
    AV_REQUIRE(c->search >= 1 && c->search <= MAX_R, AV_EINVAL, "%s: search %d is not in 1 .. %d", who, c->search, MAX_R);
    const int ty = (c->gh - 2 * c->search) / c->tile, tx = (c->gw - 2 * c->search) / c->tile;
    AV_REQUIRE(c->gh - 2 * c->search >= c->tile && c->gw - 2 * c->search >= c->tile, AV_EINVAL,
               "%s: no tile of %d px with a search range of %d px fits a %d x %d patch", who, c->tile, c->search, c->gh, c->gw);
    AV_REQUIRE((long long)ty * tx <= 65535, AV_EINVAL, "%s: more than 65535 tiles", who);
    AV_REQUIRE(c->m_per_px > 0.0 && std::isfinite(c->m_per_px) && std::isfinite(c->f_far), AV_EINVAL,
               "%s: m_per_px must be > 0 and finite, f_far finite", who);
    AV_REQUIRE(c->frame_rate > 0.0 && std::isfinite(c->frame_rate), AV_EINVAL, "%s: frame_rate must be > 0 and finite", who);
    AV_REQUIRE(c->min_texture >= 0, AV_EINVAL, "%s: min_texture must be >= 0", who);
    AV_REQUIRE(c->gate_px >= 0 && c->gate_px <= 2 * c->search, AV_EINVAL, "%s: gate_px must be 0 .. 2 * search", who);
    AV_REQUIRE(c->inlier_px > 0.0 && std::isfinite(c->inlier_px), AV_EINVAL, "%s: inlier_px must be > 0 and finite", who);
    AV_REQUIRE(c->min_inliers >= 1, AV_EINVAL, "%s: min_inliers must be >= 1", who);
    if (g) *g = Geom{c->gh, c->gw, (c->gw + 31) / 32, c->tile, c->search, ty, tx, ty * tx};
    return AV_OK;
}

}  // namespace egoflow

namespace {

using namespace egoflow;

constexpr int MATCH_WAVES = 4;                  // tiles per workgroup of the match kernel
constexpr int MATCH_K = (MAX_BINS + 63) / 64;   // candidates per lane of the match kernel, at most

// the slot of the ping-pong pair that camera `cam`'s current frame uses (0 for the stage entries, which have no state): the frame
// counter is that of state cam / per (per cameras share a state: a rig's follow their vehicle's)
__device__ __forceinline__ int slot_of(const av_egoflow_state* __restrict__ st, int cam, int per) {
    return st ? (st[cam / per].frames & 1) : 0;
}

// ---- stage 1: patch ------------------------------------------------------------------------------------------------------------
// a wave makes 64 adjacent pixels of one patch row: one byte per lane, and the wave's ballot is the row's two validity words.
// WIDE: the frames are at least two pixels wide (the bilinear sample's packed form)
template <bool WIDE>
__global__ void __launch_bounds__(256) egoflow_patch_kernel(const av_ground_cfg* __restrict__ ground, int h, int w,
                                                            const uint8_t* __restrict__ bgr, Geom g, double f_far, double m_per_px,
                                                            uint8_t* __restrict__ patch, size_t cam_stride,
                                                            const av_egoflow_state* __restrict__ st, int cams_per_state,
                                                            uint32_t* __restrict__ valid) {
    const int cam = blockIdx.z, lane = lane_id();
    const int r = blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    const int c = blockIdx.x * 64 + lane;
    if (r >= g.gh) return;                                          // (a whole wave)
    bool ok = false;
    unsigned gray = 0;
    if (c < g.gw) {
        const double f = f_far - ((double)r + 0.5) * m_per_px;
        const double l = (((double)c + 0.5) - (double)g.gw / 2.0) * m_per_px;
        long long iu, iv;
        ok = grounddev::warp_position(ground[cam].ginv, h, w, f, l, iu, iv);
        if (ok) {
            const unsigned p = grounddev::warp_sample<WIDE>(bgr + (size_t)cam * h * w * 3, h, w, iu, iv);
            gray = (1868u * (p & 255u) + 9617u * ((p >> 8) & 255u) + 4899u * ((p >> 16) & 255u) + 8192u) >> 14;
        }
    }
    const unsigned long long bits = __ballot(ok);
    if (c < g.gw) patch[(size_t)cam * cam_stride + (size_t)slot_of(st, cam, cams_per_state) * g.gh * g.gw + (size_t)r * g.gw + c] = (uint8_t)gray;
    if (valid) {
        const int w0 = (int)blockIdx.x * 2;                         // w0 < vw, since the block has a column below gw
        uint32_t* vr = valid + ((size_t)cam * g.gh + r) * g.vw;
        if (lane == 0) vr[w0] = (uint32_t)bits;
        if (lane == 32 && w0 + 1 < g.vw) vr[w0 + 1] = (uint32_t)(bits >> 32);
    }
}

// ---- stage 2: match ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int match_wave_bytes(int T, int R) {
    const int W2 = T + 2 * R, WP = (W2 + 3) & ~3, C1 = 2 * R + 1;
    return (T * T + W2 * WP + 4 + C1 * C1 * 4 + 15) & ~15;
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// TW = T / 4, the words of a tile row: the one kernel body, instantiated for every tile size so that a row stays in registers
template <int TW>
__global__ void __launch_bounds__(64 * MATCH_WAVES) egoflow_match_kernel(Geom g, int min_texture, double f_far, double m_per_px,
                                                                         const uint8_t* __restrict__ cur_base,
                                                                         const uint8_t* __restrict__ prev_base, size_t cam_stride,
                                                                         const av_egoflow_state* __restrict__ st, int cams_per_state,
                                                                         const uint32_t* __restrict__ valid,
                                                                         av_egoflow_tile* __restrict__ tiles) {
    extern __shared__ __align__(16) uint8_t lds[];
    const int cam = blockIdx.y, wave = (int)(threadIdx.x >> 6), lane = lane_id();
    const int tile = (int)blockIdx.x * MATCH_WAVES + wave;
    const bool active = tile < g.n_tiles;                           // (no early return: the workgroup's barriers are for all)
    constexpr int T = TW * 4;
    const int R = g.R, W2 = T + 2 * R, WPW = (W2 + 3) >> 2, C1 = 2 * R + 1, C = C1 * C1;
    uint8_t* mine = lds + wave * match_wave_bytes(T, R);
    uint32_t* curw = reinterpret_cast<uint32_t*>(mine);                             // [T][TW]
    uint32_t* winw = reinterpret_cast<uint32_t*>(mine + T * T);                     // [W2][WPW] + 1
    int* sadv = reinterpret_cast<int*>(mine + T * T + W2 * WPW * 4 + 4);            // [C]
    const int slot = slot_of(st, cam, cams_per_state);
    const size_t plane = (size_t)g.gh * g.gw;
    const uint8_t* cur = cur_base + (size_t)cam * cam_stride + (size_t)slot * plane;
    const uint8_t* prev = prev_base + (size_t)cam * cam_stride + (st ? (size_t)(slot ^ 1) * plane : (size_t)0);
    const int y0 = R + (active ? tile / g.tx : 0) * T, x0 = R + (active ? tile % g.tx : 0) * T;

    // live: lane i checks row y0 - R + i of the neighbourhood (W2 <= 62 rows), columns x0 - R .. x0 + T + R - 1, at most three words
    bool live = false;
    if (active) {
        bool row_ok = true;
        if (lane < W2) {
            const uint32_t* vr = valid + ((size_t)cam * g.gh + (y0 - R + lane)) * g.vw;     // y0 + T + R <= gh, x0 + T + R <= gw
            const int xa = x0 - R, xb = x0 + T + R;
            for (int wd = xa >> 5; wd <= (xb - 1) >> 5; ++wd) {
                const int lo = max(xa, wd * 32) - wd * 32, n = min(xb, wd * 32 + 32) - wd * 32 - lo;
                const uint32_t mask = n == 32 ? 0xFFFFFFFFu : (((1u << n) - 1u) << lo);
                row_ok = row_ok && (vr[wd] & mask) == mask;
            }
        }
        live = __ballot(!row_ok) == 0ull;
    }
    if (live) {                                                     // stage the tile and its neighbourhood, four pixels to a word
        for (int k = lane; k < T * TW; k += 64) {
            const uint8_t* p = cur + (size_t)(y0 + k / TW) * g.gw + x0 + (k % TW) * 4;
            curw[k] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
        }
        for (int k = lane; k < W2 * WPW; k += 64) {
            const int j0 = (k % WPW) * 4;
            const uint8_t* p = prev + (size_t)(y0 - R + k / WPW) * g.gw + (x0 - R) + j0;
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (j0 + b < W2) v |= (unsigned)p[b] << (8 * b);    // (the row's padding bytes are past the neighbourhood: not read)
            winw[k] = v;
        }
        if (lane == 0) winw[W2 * WPW] = 0;                          // the word a shift of 0 reads behind the last row and drops
    }
    __syncthreads();
    unsigned key = 0xFFFFFFFFu;
    int texture = 0;
    if (live) {
        // the lane's candidates c = lane + 64 k, k < nk <= MATCH_K: where[k] = the candidate's first window word << 2 | its byte
        // shift (a lane past the last candidate computes candidate 0 again and drops it); tile rows outermost, so that a row of the
        // tile is read once for all of the lane's candidates
        const int nk = (C + 63) >> 6;
        unsigned acc[MATCH_K], where[MATCH_K];
#pragma unroll
        for (int k = 0; k < MATCH_K; ++k) {
            const int c = lane + 64 * k, cc = c < C ? c : 0, dyi = cc / C1, dxi = cc % C1;
            where[k] = (unsigned)((dyi * WPW + (dxi >> 2)) << 2) | (unsigned)(dxi & 3), acc[k] = 0;
        }
        for (int i = 0; i < T; ++i) {
            unsigned crow[TW];
#pragma unroll
            for (int j = 0; j < TW; ++j) crow[j] = curw[i * TW + j];
            const uint32_t* wrow = winw + i * WPW;
#pragma unroll
            for (int k = 0; k < MATCH_K; ++k) {
                if (k < nk) {                                       // (uniform)
                    // words (dyi + i) * WPW + (dxi >> 2) + 0 .. TW: at most W2 * WPW, the padding word
                    const uint32_t* wr = wrow + (where[k] >> 2);
                    const unsigned sh = where[k] & 3u;
                    unsigned lo = wr[0];
#pragma unroll
                    for (int j = 0; j < TW; ++j) {
                        const unsigned hi = wr[j + 1];
                        acc[k] = __builtin_amdgcn_sad_u8(crow[j], __builtin_amdgcn_alignbyte(hi, lo, sh), acc[k]);
                        lo = hi;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < MATCH_K; ++k) {
            const int c = lane + 64 * k;
            if (c < C) {
                sadv[c] = (int)acc[k];                              // acc <= 32 * 32 * 255 < 2^18, c < 1024
                key = min(key, (acc[k] << 10) | (unsigned)c);
            }
        }
        const uint8_t* cb = reinterpret_cast<const uint8_t*>(curw);
        for (int k = lane; k < T * T; k += 64) {
            const int i = k / T, j = k % T, p = cb[k];
            if (j + 1 < T) texture += abs(p - (int)cb[k + 1]);
            if (i + 1 < T) texture += abs(p - (int)cb[k + T]);
        }
        texture = wave_sum_i(texture);
        key = wave_min_u32(key);
    }
    __syncthreads();
    if (active && lane == 0) {
        av_egoflow_tile o;
        o.flags = 0, o.dy = o.dx = o.sad = o.texture = o.reserved = 0, o.sub_dy = o.sub_dx = 0.0;
        o.f = f_far - ((double)y0 + (double)T / 2.0) * m_per_px;
        o.l = (((double)x0 + (double)T / 2.0) - (double)g.gw / 2.0) * m_per_px;
        if (live) {
            const int best = (int)(key & 1023u), s0 = (int)(key >> 10);
            o.dy = best / C1 - R, o.dx = best % C1 - R, o.sad = s0, o.texture = texture;
            const bool iy = o.dy > -R && o.dy < R, ix = o.dx > -R && o.dx < R;
            o.flags = AV_EGOFLOW_LIVE | ((texture >= min_texture && iy && ix) ? AV_EGOFLOW_ACCEPTED : 0);
            if (iy) {
                const int sm = sadv[best - C1], sp = sadv[best + C1];
                const double den = (double)(sm - 2 * s0 + sp) * 2.0;
                o.sub_dy = den > 0.0 ? (double)(sm - sp) / den : 0.0;
            }
            if (ix) {
                const int sm = sadv[best - 1], sp = sadv[best + 1];
                const double den = (double)(sm - 2 * s0 + sp) * 2.0;
                o.sub_dx = den > 0.0 ? (double)(sm - sp) / den : 0.0;
            }
        }
        tiles[(size_t)cam * g.n_tiles + tile] = o;
    }
}

// ---- stage 3: solve ------------------------------------------------------------------------------------------------------------
// (the pieces -- accepted, vote, displacement, the fit's elimination, the residual -- are egoflow_dev.h's, shared with rigflow.hip)
__global__ void __launch_bounds__(64) egoflow_solve_kernel(int n_tiles, int R, int gate, double m_per_px, double thr2, int min_inliers,
                                                           av_egoflow_tile* __restrict__ tiles, av_egoflow_motion* __restrict__ motion) {
    __shared__ int hist[MAX_BINS];
    const int cam = blockIdx.x, lane = lane_id(), C1 = 2 * R + 1;
    av_egoflow_tile* tl = tiles + (size_t)cam * n_tiles;
    int n_acc;
    const int bin = vote(hist, tl, n_tiles, R, lane, n_acc);
    const int my = bin / C1 - R, mx = bin % C1 - R;
    auto gated = [&](const av_egoflow_tile& t) { return accepted(t, R) && abs(t.dy - my) <= gate && abs(t.dx - mx) <= gate; };

    // the two fits: over the gated tiles, then over the first fit's inliers
    Fit fit[2] = {{0.0, 0.0, 0.0, 0, false}, {0.0, 0.0, 0.0, 0, false}};
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && !fit[0].ok) break;                         // (uniform)
        int n = 0;
        Sums s{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = lane; k < n_tiles; k += 64) {
            const av_egoflow_tile t = tl[k];
            if (!gated(t)) continue;
            const Disp d = displacement(t, m_per_px);
            if (pass == 1 && residual2(t.f, t.l, d, fit[0]) > thr2) continue;
            ++n, add_row(s, t.f, t.l, d);
        }
        fit[pass] = fit_of_sums(wave_sum_i(n), wave_sums(s));
    }
    // flags, and the rms of the final fit's residuals over its tiles
    int n_gated = 0;
    double ss = 0.0;
    for (int k = lane; k < n_tiles; k += 64) {
        const av_egoflow_tile t = tl[k];
        int fl = t.flags & (AV_EGOFLOW_ACCEPTED | AV_EGOFLOW_LIVE);
        if (gated(t)) {
            fl |= AV_EGOFLOW_GATED, ++n_gated;
            const Disp d = displacement(t, m_per_px);
            if (fit[0].ok && !(residual2(t.f, t.l, d, fit[0]) > thr2)) {
                fl |= AV_EGOFLOW_INLIER;
                if (fit[1].ok) ss += residual2(t.f, t.l, d, fit[1]);
            }
        }
        tl[k].flags = fl;
    }
    n_gated = wave_sum_i(n_gated);
    ss = wave_sum_dpp(ss);
    if (lane == 0) {
        av_egoflow_motion o;
        const bool have = fit[0].ok && fit[1].ok;
        o.t_f = have ? fit[1].tf : 0.0, o.t_l = have ? fit[1].tl : 0.0, o.omega = have ? fit[1].om : 0.0;
        o.rms = have ? sqrt(ss / (double)fit[1].n) : 0.0;
        o.n_accepted = n_acc, o.n_gated = n_gated, o.n_inliers = fit[0].ok ? fit[1].n : 0;
        o.valid = have && fit[1].n >= min_inliers;
        o.vote_dy = my, o.vote_dx = mx, o.reserved[0] = o.reserved[1] = 0;
        motion[cam] = o;
    }
}

// ---- stage 4: measure ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) egoflow_measure_kernel(int n_cams, double frame_rate, const av_egoflow_motion* __restrict__ motion,
                                                             av_egoflow_state* __restrict__ state, double* __restrict__ z,
                                                             uint8_t* __restrict__ mode) {
    const int cam = blockIdx.x * 64 + threadIdx.x;
    if (cam >= n_cams) return;
    av_egoflow_state s = state[cam];
    const av_egoflow_motion mo = motion[cam];
    double vx = 0.0, vy = 0.0;
    const bool use = mo.valid && s.frames >= 1;
    if (use) {
        const double c = cos(s.psi), sn = sin(s.psi);
        const double Dx = mo.t_f * c - mo.t_l * sn, Dy = mo.t_f * sn + mo.t_l * c;
        s.x += Dx, s.y += Dy, s.psi += mo.omega;
        vx = Dx * frame_rate, vy = Dy * frame_rate;
    }
    s.frames += 1;
    state[cam] = s;
    z[cam * 4 + 0] = s.x, z[cam * 4 + 1] = s.y, z[cam * 4 + 2] = vx, z[cam * 4 + 3] = vy;
    mode[cam] = use ? 1 : 2;
}

// ---- launches (arguments already checked) -----------------------------------------------------------------------------------------
int launch_solve(av_stream_t stream, const av_egoflow_cfg* c, const Geom& g, int n_cams, av_egoflow_tile* tiles,
                 av_egoflow_motion* motion) {
    const double thr = c->inlier_px * c->m_per_px;
    hipLaunchKernelGGL(egoflow_solve_kernel, dim3((unsigned)n_cams), dim3(64), 0, as_stream(stream), g.n_tiles, g.R, c->gate_px,
                       c->m_per_px, thr * thr, c->min_inliers, tiles, motion);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // namespace

namespace egoflow {

int launch_patch(av_stream_t stream, const av_egoflow_cfg* c, const Geom& g, const av_ground_cfg* ground, int n_cams, int h, int w,
                 const uint8_t* bgr, uint8_t* patch, size_t cam_stride, const av_egoflow_state* st, int cams_per_state,
                 uint32_t* valid) {
    const dim3 grid((unsigned)((g.gw + 63) / 64), (unsigned)((g.gh + 3) / 4), (unsigned)n_cams);
    const auto kernel = w >= 2 ? egoflow_patch_kernel<true> : egoflow_patch_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), ground, h, w, bgr, g, c->f_far, c->m_per_px, patch,
                       cam_stride, st, cams_per_state, valid);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
int launch_match(av_stream_t stream, const av_egoflow_cfg* c, const Geom& g, int n_cams, const uint8_t* cur, const uint8_t* prev,
                 size_t cam_stride, const av_egoflow_state* st, int cams_per_state, const uint32_t* valid,
                 av_egoflow_tile* tiles) {
    const dim3 grid((unsigned)((g.n_tiles + MATCH_WAVES - 1) / MATCH_WAVES), (unsigned)n_cams);
    const size_t lds = (size_t)MATCH_WAVES * match_wave_bytes(g.T, g.R);                  // at most 4 * 8848 bytes
#define EGO_MATCH(TW)                                                                                                             \
    case TW:                                                                                                                      \
        hipLaunchKernelGGL(egoflow_match_kernel<TW>, grid, dim3(64 * MATCH_WAVES), lds, as_stream(stream), g, c->min_texture, c->f_far, \
                           c->m_per_px, cur, prev, cam_stride, st, cams_per_state, valid, tiles);                                \
        break;
    switch (g.T / 4) {                                              // T is a multiple of 4 in 4 .. 32
        EGO_MATCH(1) EGO_MATCH(2) EGO_MATCH(3) EGO_MATCH(4) EGO_MATCH(5) EGO_MATCH(6) EGO_MATCH(7) EGO_MATCH(8)
    }
#undef EGO_MATCH
    AV_LAUNCH_CHECK();
    return AV_OK;
}
int launch_measure(av_stream_t stream, const av_egoflow_cfg* c, int n_cams, const av_egoflow_motion* motion, av_egoflow_state* state,
                   double* z, uint8_t* mode) {
    hipLaunchKernelGGL(egoflow_measure_kernel, dim3((unsigned)((n_cams + 63) / 64)), dim3(64), 0, as_stream(stream), n_cams,
                       c->frame_rate, motion, state, z, mode);
    AV_LAUNCH_CHECK();
    return AV_OK;
}


}  // namespace egoflow

#define EGO_CAMS(who) AV_REQUIRE(n_cams >= 1 && n_cams <= 65535, AV_EINVAL, who ": n_cams must be 1 .. 65535")

extern "C" int av_egoflow_tiles(const av_egoflow_cfg* cfg, int* tiles_y, int* tiles_x) {
    AV_REQUIRE(tiles_y && tiles_x, AV_EINVAL, "av_egoflow_tiles: null argument");
    Geom g;
    if (int rc = geometry(cfg, "av_egoflow_tiles", &g)) return rc;
    *tiles_y = g.ty, *tiles_x = g.tx;
    return AV_OK;
}

extern "C" int av_egoflow_patch(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, const av_ground_cfg* ground, int n_cams,
                                int h, int w, const uint8_t* bgr, uint8_t* patch, uint32_t* valid) {
    AV_REQUIRE(ctx && ground && bgr && patch && valid, AV_EINVAL, "av_egoflow_patch: null argument");
    EGO_CAMS("av_egoflow_patch");
    AV_REQUIRE(h >= 1 && w >= 1, AV_EINVAL, "av_egoflow_patch: h and w must be >= 1");
    Geom g;
    if (int rc = geometry(cfg, "av_egoflow_patch", &g)) return rc;
    return launch_patch(stream, cfg, g, ground, n_cams, h, w, bgr, patch, (size_t)g.gh * g.gw, nullptr, 1, valid);
}

extern "C" int av_egoflow_match(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_cams, const uint8_t* cur,
                                const uint8_t* prev, const uint32_t* valid, av_egoflow_tile* tiles) {
    AV_REQUIRE(ctx && cur && prev && valid && tiles, AV_EINVAL, "av_egoflow_match: null argument");
    EGO_CAMS("av_egoflow_match");
    Geom g;
    if (int rc = geometry(cfg, "av_egoflow_match", &g)) return rc;
    return launch_match(stream, cfg, g, n_cams, cur, prev, (size_t)g.gh * g.gw, nullptr, 1, valid, tiles);
}

extern "C" int av_egoflow_solve(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_cams, av_egoflow_tile* tiles,
                                av_egoflow_motion* motion) {
    AV_REQUIRE(ctx && tiles && motion, AV_EINVAL, "av_egoflow_solve: null argument");
    EGO_CAMS("av_egoflow_solve");
    Geom g;
    if (int rc = geometry(cfg, "av_egoflow_solve", &g)) return rc;
    return launch_solve(stream, cfg, g, n_cams, tiles, motion);
}

extern "C" int av_egoflow_measure(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, int n_cams, const av_egoflow_motion* motion,
                                  av_egoflow_state* state, double* z, uint8_t* mode) {
    AV_REQUIRE(ctx && motion && state && z && mode, AV_EINVAL, "av_egoflow_measure: null argument");
    EGO_CAMS("av_egoflow_measure");
    if (int rc = geometry(cfg, "av_egoflow_measure", nullptr)) return rc;
    return launch_measure(stream, cfg, n_cams, motion, state, z, mode);
}

extern "C" int av_egoflow_update(av_ctx* ctx, av_stream_t stream, const av_egoflow_cfg* cfg, const av_ground_cfg* ground, int n_cams,
                                 int h, int w, const uint8_t* bgr, uint8_t* patches, uint32_t* valid, av_egoflow_tile* tiles,
                                 av_egoflow_motion* motion, av_egoflow_state* state, double* z, uint8_t* mode) {
    AV_REQUIRE(ctx && ground && bgr && patches && valid && tiles && motion && state && z && mode, AV_EINVAL,
               "av_egoflow_update: null argument");
    EGO_CAMS("av_egoflow_update");
    AV_REQUIRE(h >= 1 && w >= 1, AV_EINVAL, "av_egoflow_update: h and w must be >= 1");
    Geom g;
    if (int rc = geometry(cfg, "av_egoflow_update", &g)) return rc;
    const size_t pair = (size_t)2 * g.gh * g.gw;
    if (int rc = launch_patch(stream, cfg, g, ground, n_cams, h, w, bgr, patches, pair, state, 1, valid)) return rc;
    if (int rc = launch_match(stream, cfg, g, n_cams, patches, patches, pair, state, 1, valid, tiles)) return rc;
    if (int rc = launch_solve(stream, cfg, g, n_cams, tiles, motion)) return rc;
    return launch_measure(stream, cfg, n_cams, motion, state, z, mode);
}
