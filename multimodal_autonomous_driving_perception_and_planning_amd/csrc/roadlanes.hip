// Road lanes (include/avhot.h: av_road_lanes*): the Hough segments of a rig's K cameras carried onto the road and into the vehicle
// frame, pooled, and the lane boundaries found there in metres -- two votes, a gated refit in three rounds, the ego lane, its
// following through the measured ego motion, the planner's reference path and the maneuver tagger's offset.
//
// Mapping (av_rig_egoflow_solve's): one workgroup per vehicle, one wave per camera.  scap <= 256, so a lane owns at most four
// segments (i = lane, lane + 64, ...): their projected end points, length, slope and weight stay in REGISTERS from the first pass
// to the last -- neither LDS (80 KB of rows would need dynamic LDS and halve the workgroups per CU) nor a second projection (two
// divisions per end point and round).  The two 64-bin histograms share one LDS array (integer atomics: order-free), wave 0 smooths
// it and picks the peaks with one lane per bin.  A round's sums are taken per boundary: per lane in row order, the wave's fixed
// tree, and thread p adds the cameras' parts in the order k = 0 .. K - 1 and solves boundary p.  Thread 0 then picks the ego lane
// and steps the state; wave 0 writes the path, one point a lane.  The header states the arithmetic; DESIGN.md 7v has the resources
// and the measurements.  float64, -ffp-contract=off: every operation rounded on its own.  Plain vector stores only.
#include "ground_dev.h"

#include <cmath>

static_assert(sizeof(av_road_lanes_cfg) == 144 && sizeof(av_road_lane_bound) == 64 && sizeof(av_road_lanes_row) == 128 &&
                  sizeof(av_road_lanes_info) == 72 && sizeof(av_road_lanes_state) == 96,
              "av_road_lanes layouts (include/avhot.h)");

namespace {

constexpr int MAX_CAMS = 8, MAXB = AV_ROAD_LANES_MAX_BOUNDS, RPL = 4, MAX_SCAP = 64 * RPL, BINS = 64, NSUM = 8;

struct Shared {
    int hist[BINS];
    int cnt[MAX_CAMS][6];                       // rows, off, short, steep, voters, over
    double part[MAX_CAMS][MAXB][NSUM];          // a camera's sums per boundary (S0..S4, T0..T2; the votes' means use [0])
    double part_min[MAX_CAMS][MAXB], part_max[MAX_CAMS][MAXB];
    int part_n[MAX_CAMS][MAXB];
    double model[MAXB][3];
    double st_xmin[MAXB], st_xmax[MAXB], st_s0[MAXB];
    int st_n[MAXB], st_views[MAXB], st_flags[MAXB];
    int peaks[MAXB];
    int nb, dir_bin, n_cand;
    double m_star;
    double centre[3], x_end;
    int n_ref;
    av_road_lane_bound out[MAXB];               // the boundaries that have members (indexed by the ego lane's choice: LDS, not scratch)
};

__device__ __forceinline__ double model_at(const double* a, double X) { return (a[0] + a[1] * X) + a[2] * (X * X); }

// h'[i] of the header for lane i of wave 0
__device__ __forceinline__ int smoothed(const int* hist, int i) {
    const int hl = i > 0 ? hist[i - 1] : 0, hr = i < BINS - 1 ? hist[i + 1] : 0;
    return hl + 2 * hist[i] + hr;
}

// the header's fit of one boundary from the vehicle's sums: false = singular
__device__ __forceinline__ bool fit_bound(const double* S, bool quad, double* a) {
    const double S0 = S[0], S1 = S[1], S2 = S[2], S3 = S[3], S4 = S[4], T0 = S[5], T1 = S[6], T2 = S[7];
    const double c11 = S2 - (S1 * S1) / S0, d1 = T1 - (S1 * T0) / S0;
    if (!(c11 > 1e-9 * S2)) return false;
    if (quad) {
        const double c12 = S3 - (S1 * S2) / S0, c22 = S4 - (S2 * S2) / S0, d2 = T2 - (S2 * T0) / S0;
        const double e22 = c22 - (c12 * c12) / c11;
        if (!(e22 > 1e-9 * S4)) return false;
        a[2] = (d2 - (c12 * d1) / c11) / e22;
        a[1] = (d1 - c12 * a[2]) / c11;
        a[0] = ((T0 - a[1] * S1) - a[2] * S2) / S0;
    } else {
        a[1] = d1 / c11;
        a[0] = (T0 - a[1] * S1) / S0;
        a[2] = 0.0;
    }
    return true;
}

// step 6 of the header for one side: a (the smoothed polynomial), xmax, has and miss are the state's; b the side's measured boundary
// or NULL.  (Called once per side with the side's own variables, so that they stay in registers.)
__device__ __forceinline__ void follow_side(const av_road_lanes_cfg& cfg, double (&a)[3], double& xmax, int32_t& has, int32_t& miss,
                                            const av_road_lane_bound* b, bool mv, double tf, double tl, double om, double one_m_alpha,
                                            int coast_bit, int& status, bool& jumped, double& jump_d) {
    double pr[3] = {a[0], a[1], a[2]}, pxmax = xmax;
    if (mv) {
        pr[0] = ((a[0] + a[1] * tf) + a[2] * (tf * tf)) - tl;
        pr[1] = (a[1] + (2.0 * a[2]) * tf) - om;
        pxmax = xmax - tf;
    }
    if (b) {
        const double nw[3] = {b->a0, b->a1, b->a2};
        bool smooth = false;
        if (has) {
            const double d = nw[0] - pr[0];
            if (fabs(d) <= cfg.jump) smooth = true;
            else jumped = true, jump_d = d;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) a[i] = smooth ? cfg.alpha * pr[i] + one_m_alpha * nw[i] : nw[i];
        xmax = b->x_max, has = 1, miss = 0;
    } else if (has) {
        miss += 1;
        if (miss > cfg.max_coast) {
            a[0] = a[1] = a[2] = 0.0, xmax = 0.0, has = 0, miss = 0;
        } else {
            a[0] = pr[0], a[1] = pr[1], a[2] = pr[2], xmax = pxmax;
            status |= coast_bit;
        }
    }
}

// steps 5 - 7 of the header but the path's points: one thread per vehicle
__device__ void finish(const av_road_lanes_cfg& cfg, Shared& sh, int K, bool no_voter, const av_egoflow_motion* motion,
                       av_road_lanes_state* state, av_road_lane_bound* bounds, av_road_lanes_info* info, av_road_lanes_row* row,
                       int32_t* n_ref, double* lane_offset) {
    // the boundaries that have members, in order
    av_road_lane_bound* B = sh.out;
    int nb = 0;
    for (int p = 0; p < sh.nb; ++p) {
        if (sh.st_n[p] == 0) continue;
        av_road_lane_bound& b = B[nb++];                                  // (field by field: no private copy of the struct)
        b.a0 = sh.model[p][0], b.a1 = sh.model[p][1], b.a2 = sh.model[p][2];
        b.x_min = sh.st_xmin[p], b.x_max = sh.st_xmax[p], b.length = sh.st_s0[p] * 0.5;
        b.n_members = sh.st_n[p], b.views = sh.st_views[p], b.flags = sh.st_flags[p], b.reserved = 0;
    }
    // 5. the ego lane
    int iL = -1, iR = -1;
    for (int p = 0; p < nb; ++p) {
        const double a0 = B[p].a0;
        if (a0 < 0.0) {
            if (iL < 0 || a0 > B[iL].a0) iL = p;
        } else if (a0 >= 0.0) {
            if (iR < 0 || a0 < B[iR].a0) iR = p;
        }
    }
    if (iL >= 0 && iR >= 0) {
        const double wd = B[iR].a0 - B[iL].a0;
        if (!(wd >= cfg.w_min && wd <= cfg.w_max)) {
            if (-B[iL].a0 <= B[iR].a0) iR = -1;
            else iL = -1;
        }
    }
    if (iL >= 0) B[iL].flags |= AV_ROAD_BOUND_LEFT;
    if (iR >= 0) B[iR].flags |= AV_ROAD_BOUND_RIGHT;
    // 6. following
    av_road_lanes_state st = *state;
    const bool mv = motion != nullptr && motion->valid != 0;
    const double tf = mv ? motion->t_f : 0.0, tl = mv ? motion->t_l : 0.0, om = mv ? motion->omega : 0.0;
    const double one_m_alpha = 1.0 - cfg.alpha;
    int status = no_voter ? AV_ROAD_NO_VOTER : 0;
    bool jumped[2] = {false, false};
    double jump_d[2] = {0.0, 0.0};
    double a_left[3] = {st.left[0], st.left[1], st.left[2]}, a_right[3] = {st.right[0], st.right[1], st.right[2]};
    follow_side(cfg, a_left, st.xmax_left, st.has_left, st.miss_left, iL >= 0 ? &B[iL] : nullptr, mv, tf, tl, om, one_m_alpha,
                AV_ROAD_COAST_LEFT, status, jumped[0], jump_d[0]);
    follow_side(cfg, a_right, st.xmax_right, st.has_right, st.miss_right, iR >= 0 ? &B[iR] : nullptr, mv, tf, tl, om, one_m_alpha,
                AV_ROAD_COAST_RIGHT, status, jumped[1], jump_d[1]);
    st.left[0] = a_left[0], st.left[1] = a_left[1], st.left[2] = a_left[2];
    st.right[0] = a_right[0], st.right[1] = a_right[1], st.right[2] = a_right[2];
    if (iL >= 0 && iR >= 0) st.width = st.right[0] - st.left[0], st.has_width = 1;
    if (jumped[0] && jumped[1]) {
        const double d0 = fabs(jump_d[0]), d1 = fabs(jump_d[1]);
        if (d0 >= cfg.w_min && d0 <= cfg.w_max && d1 >= cfg.w_min && d1 <= cfg.w_max) {
            if (jump_d[0] < 0.0 && jump_d[1] < 0.0) status |= AV_ROAD_CHANGE_LEFT;
            if (jump_d[0] > 0.0 && jump_d[1] > 0.0) status |= AV_ROAD_CHANGE_RIGHT;
        }
    }
    st.frames += 1;
    *state = st;
    // the output's sides
    double oL[3] = {st.left[0], st.left[1], st.left[2]}, oR[3] = {st.right[0], st.right[1], st.right[2]};
    double xL = st.xmax_left, xR = st.xmax_right;
    bool outL = st.has_left != 0, outR = st.has_right != 0;
    if (cfg.one_sided && ((iL >= 0) != (iR >= 0)) && !(outL && outR)) {
        const double W = st.has_width ? st.width : cfg.default_width;
        if (iL >= 0) oR[0] = oL[0] + W, oR[1] = oL[1], oR[2] = oL[2], xR = xL, outR = true;
        else oL[0] = oR[0] - W, oL[1] = oR[1], oL[2] = oR[2], xL = xR, outL = true;
        status |= AV_ROAD_ONE_SIDED;
    }
    const bool lane = outL && outR;
    if (lane) status |= AV_ROAD_LANE;
    // 7. outputs
    av_road_lanes_row r;
    for (int i = 0; i < 3; ++i) {
        r.left[i] = outL ? oL[i] : 0.0, r.right[i] = outR ? oR[i] : 0.0;
        r.centre[i] = lane ? (oL[i] + oR[i]) * 0.5 : 0.0;
    }
    r.width = lane ? oR[0] - oL[0] : 0.0;
    r.lane_offset = lane ? -r.centre[0] : __builtin_nan("");
    r.heading = lane ? -atan(r.centre[1]) : 0.0;
    const double q = 1.0 + r.centre[1] * r.centre[1];
    r.curvature = lane ? (2.0 * r.centre[2]) / (q * sqrt(q)) : 0.0;
    int nl = 0, nr = 0;
    if (lane) {
        if (iL >= 0)
            for (int j = iL - 1; j >= 0; --j) {
                const double sp = B[j + 1].a0 - B[j].a0;
                if (!(sp >= cfg.w_min && sp <= cfg.w_max)) break;
                ++nl;
            }
        if (iR >= 0)
            for (int j = iR + 1; j < nb; ++j) {
                const double sp = B[j].a0 - B[j - 1].a0;
                if (!(sp >= cfg.w_min && sp <= cfg.w_max)) break;
                ++nr;
            }
    }
    r.n_bounds = nb, r.lane_count = lane ? 1 + nl + nr : 0, r.lane_index = nl;
    r.views = (iL >= 0 ? B[iL].views : 0) | (iR >= 0 ? B[iR].views : 0);
    r.status = status, r.reserved = 0;
    *row = r;
    *lane_offset = r.lane_offset;
    for (int p = 0; p < MAXB; ++p) {
        const bool on = p < nb;
        av_road_lane_bound& o = bounds[p];
        o.a0 = on ? B[p].a0 : 0.0, o.a1 = on ? B[p].a1 : 0.0, o.a2 = on ? B[p].a2 : 0.0;
        o.x_min = on ? B[p].x_min : 0.0, o.x_max = on ? B[p].x_max : 0.0, o.length = on ? B[p].length : 0.0;
        o.n_members = on ? B[p].n_members : 0, o.views = on ? B[p].views : 0, o.flags = on ? B[p].flags : 0, o.reserved = 0;
    }
    av_road_lanes_info f;
    int n_over = 0, n_off = 0, n_short = 0, n_steep = 0, n_voters = 0;
    for (int j = 0; j < MAX_CAMS; ++j) {
        const bool on = j < K;
        f.cam_rows[j] = on ? sh.cnt[j][0] : 0;
        if (on) n_off += sh.cnt[j][1], n_short += sh.cnt[j][2], n_steep += sh.cnt[j][3], n_voters += sh.cnt[j][4], n_over += sh.cnt[j][5];
    }
    f.n_over = n_over, f.n_off = n_off, f.n_short = n_short, f.n_steep = n_steep, f.n_voters = n_voters;
    f.dir_bin = no_voter ? -1 : sh.dir_bin, f.n_cand = no_voter ? 0 : sh.n_cand, f.n_peaks = no_voter ? 0 : sh.nb;
    f.m_star = no_voter ? 0.0 : sh.m_star;
    *info = f;
    // the path's frame for wave 0
    const double x_end = fmin(cfg.path_far, fmin(xL, xR));
    const bool path = lane && x_end - cfg.path_near >= 1.0;
    sh.centre[0] = r.centre[0], sh.centre[1] = r.centre[1], sh.centre[2] = r.centre[2], sh.x_end = x_end;
    sh.n_ref = path ? cfg.n_points : 0;
    *n_ref = sh.n_ref;
}

__global__ void __launch_bounds__(64 * MAX_CAMS) road_lanes_kernel(av_road_lanes_cfg cfg, int K, const av_ground_cfg* __restrict__ ground,
                                                                    const av_rig_mount* __restrict__ mounts, int max_segments, int scap,
                                                                    const int32_t* __restrict__ segments, const int32_t* __restrict__ nseg,
                                                                    const av_egoflow_motion* __restrict__ motion,
                                                                    const double* __restrict__ plan_state, av_road_lanes_state* state,
                                                                    av_road_lane_bound* __restrict__ bounds,
                                                                    av_road_lanes_info* __restrict__ info, av_road_lanes_row* __restrict__ row,
                                                                    int rcap, double* __restrict__ ref_path, int32_t* __restrict__ n_ref,
                                                                    double* __restrict__ lane_offset) {
    __shared__ Shared sh;
    const int tid = (int)threadIdx.x, k = tid >> 6, lane = lane_id();
    const size_t v = blockIdx.x, cam = v * (size_t)K + (size_t)k;

    // ---- 1. rows: at most RPL per lane, kept in registers ----
    double X1[RPL], Y1[RPL], X2[RPL], Y2[RPL], len[RPL], ms[RPL];
    int wt[RPL], asg[RPL];
    bool is_row[RPL];
    {
        int n = nseg[cam];
        n = n < 0 ? 0 : (n > max_segments ? max_segments : n);
        const int over = n > scap ? n - scap : 0;
        n = n > scap ? scap : n;                                             // <= scap <= 256 = 64 * RPL, <= max_segments
        const av_ground_cfg* g = ground + cam;
        const av_rig_mount mt = mounts[cam];
        int c_rows = 0, c_off = 0, c_short = 0, c_steep = 0;
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int i = lane + 64 * j;
            X1[j] = Y1[j] = X2[j] = Y2[j] = len[j] = ms[j] = 0.0, wt[j] = 0, asg[j] = -1, is_row[j] = false;
            if (i < n) {
                const int32_t* sg = segments + (cam * (size_t)max_segments + (size_t)i) * 4;
                const grounddev::RoadPoint p1 = grounddev::project(g->g, g->max_range, (double)sg[0], (double)sg[1]);
                const grounddev::RoadPoint p2 = grounddev::project(g->g, g->max_range, (double)sg[2], (double)sg[3]);
                double xa = (mt.x + mt.c * p1.f) - mt.s * p1.l, ya = (mt.y + mt.s * p1.f) + mt.c * p1.l;
                double xb = (mt.x + mt.c * p2.f) - mt.s * p2.l, yb = (mt.y + mt.s * p2.f) + mt.c * p2.l;
                if (xb < xa) {
                    const double tx = xa, ty = ya;
                    xa = xb, ya = yb, xb = tx, yb = ty;
                }
                const double dX = xb - xa, dY = yb - ya, l = sqrt(dX * dX + dY * dY);
                if (!(p1.on_road && p2.on_road)) ++c_off;
                else if (!(l >= cfg.min_len)) ++c_short;
                else if (!(dX > 0.0 && fabs(dY) <= cfg.slope_max * dX)) ++c_steep;
                else {
                    ++c_rows, is_row[j] = true;
                    X1[j] = xa, Y1[j] = ya, X2[j] = xb, Y2[j] = yb, len[j] = l, ms[j] = dY / dX;
                    wt[j] = (int)fmin(fmax(floor(l / cfg.vote_len), 1.0), 255.0);
                }
            }
        }
        c_rows = wave_sum_i(c_rows), c_off = wave_sum_i(c_off), c_short = wave_sum_i(c_short), c_steep = wave_sum_i(c_steep);
        if (lane == 0) sh.cnt[k][0] = c_rows, sh.cnt[k][1] = c_off, sh.cnt[k][2] = c_short, sh.cnt[k][3] = c_steep, sh.cnt[k][5] = over;
    }
    if (tid < BINS) sh.hist[tid] = 0;
    __syncthreads();

    // ---- 2. direction vote ----
    bool voter[RPL];
    int bin[RPL];
    {
        const double scale = 32.0 / cfg.slope_max;
        int c_vot = 0;
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            voter[j] = is_row[j] && (X1[j] + X2[j]) * 0.5 <= cfg.x_vote;
            bin[j] = 0;
            if (voter[j]) {
                const double t = floor((ms[j] + cfg.slope_max) * scale);
                bin[j] = t < 0.0 ? 0 : (t > 63.0 ? 63 : (int)t);
                atomicAdd(&sh.hist[bin[j]], wt[j]);
                ++c_vot;
            }
        }
        c_vot = wave_sum_i(c_vot);
        if (lane == 0) sh.cnt[k][4] = c_vot;
    }
    __syncthreads();
    if (k == 0) {
        const int hp = smoothed(sh.hist, lane);
        const unsigned key = wave_max_u32(hp > 0 ? ((unsigned)hp << 6) | (unsigned)(63 - lane) : 0u);
        if (lane == 0) sh.dir_bin = key ? 63 - (int)(key & 63u) : -1, sh.nb = 0, sh.n_cand = 0, sh.m_star = 0.0;
    }
    __syncthreads();
    const int dir_bin = sh.dir_bin;
    if (tid < BINS) sh.hist[tid] = 0;                                        // (wave 0 has read it: the offset vote's now)
    if (dir_bin >= 0) {                                                      // (uniform: the barriers inside are the workgroup's)
        {
            double s = 0.0;
            int sw = 0;
#pragma unroll
            for (int j = 0; j < RPL; ++j)
                if (voter[j] && abs(bin[j] - dir_bin) <= 1) s += (double)wt[j] * ms[j], sw += wt[j];
            s = wave_sum_dpp(s), sw = wave_sum_i(sw);
            if (lane == 0) sh.part[k][0][0] = s, sh.part_n[k][0] = sw;
        }
        __syncthreads();
        double m_star;
        {
            double s = sh.part[0][0][0];
            int sw = sh.part_n[0][0];
            for (int q = 1; q < K; ++q) s += sh.part[q][0][0], sw += sh.part_n[q][0];
            m_star = s / (double)sw;                                         // the peak has a voter within one bin: sw >= 1
        }
        // ---- 3. offset vote ----
        bool ovoter[RPL];
        double bs[RPL];
        {
            const double scale = 32.0 / cfg.y_max;
#pragma unroll
            for (int j = 0; j < RPL; ++j) {
                ovoter[j] = false, bs[j] = 0.0, bin[j] = 0;
                if (voter[j] && fabs(ms[j] - m_star) <= cfg.slope_tol) {
                    bs[j] = (Y1[j] + Y2[j]) * 0.5 - m_star * ((X1[j] + X2[j]) * 0.5);
                    const double t = (bs[j] + cfg.y_max) * scale;
                    if (t >= 0.0 && t < 64.0) ovoter[j] = true, bin[j] = (int)floor(t), atomicAdd(&sh.hist[bin[j]], wt[j]);
                }
            }
        }
        __syncthreads();                                                     // (also: every thread has read part[.][0][0])
        if (k == 0) {
            const int hp = smoothed(sh.hist, lane);
            const int hl = __shfl(hp, lane > 0 ? lane - 1 : 0, 64), hr = __shfl(hp, lane < 63 ? lane + 1 : 63, 64);
            bool cand = hp >= cfg.min_votes && hp > (lane > 0 ? hl : 0) && hp >= (lane < 63 ? hr : 0);
            const int n_cand = __popcll(__ballot(cand));
            const double bw = cfg.y_max / 32.0;
            unsigned long long acc = 0ull;
            for (int it = 0; it < MAXB; ++it) {
                const unsigned key = wave_max_u32(cand ? ((unsigned)hp << 6) | (unsigned)(63 - lane) : 0u);
                if (!key) break;
                const int ia = 63 - (int)(key & 63u);
                acc |= 1ull << ia;
                if ((double)abs(lane - ia) * bw < cfg.min_sep) cand = false;
            }
            if ((acc >> lane) & 1ull) sh.peaks[__popcll(acc & ((1ull << lane) - 1ull))] = lane;       // rank < 8
            if (lane == 0) sh.nb = __popcll(acc), sh.n_cand = n_cand, sh.m_star = m_star;
        }
        __syncthreads();
        const int nb = sh.nb;
        for (int p = 0; p < nb; ++p) {
            const int pk = sh.peaks[p];
            double s = 0.0;
            int sw = 0;
#pragma unroll
            for (int j = 0; j < RPL; ++j)
                if (ovoter[j] && abs(bin[j] - pk) <= 1) s += (double)wt[j] * bs[j], sw += wt[j];
            s = wave_sum_dpp(s), sw = wave_sum_i(sw);
            if (lane == 0) sh.part[k][p][0] = s, sh.part_n[k][p] = sw;
        }
        __syncthreads();
        if (tid < nb) {
            double s = sh.part[0][tid][0];
            int sw = sh.part_n[0][tid];
            for (int q = 1; q < K; ++q) s += sh.part[q][tid][0], sw += sh.part_n[q][tid];
            sh.model[tid][0] = s / (double)sw, sh.model[tid][1] = m_star, sh.model[tid][2] = 0.0;
            sh.st_flags[tid] = 0, sh.st_n[tid] = 0, sh.st_views[tid] = 0;
            sh.st_xmin[tid] = sh.st_xmax[tid] = sh.st_s0[tid] = 0.0;
        }
        __syncthreads();
        // ---- 4. grow and refit ----
        for (int round = 0; round < 3; ++round) {
            const double range = round == 0 ? cfg.x_vote : 2.0 * cfg.x_vote;
#pragma unroll
            for (int j = 0; j < RPL; ++j) {
                asg[j] = -1;
                if (!is_row[j] || !(round == 2 || (X1[j] + X2[j]) * 0.5 <= range)) continue;
                double best = INFINITY;
                for (int p = 0; p < nb; ++p) {
                    const double r1 = fabs(Y1[j] - model_at(sh.model[p], X1[j])), r2 = fabs(Y2[j] - model_at(sh.model[p], X2[j]));
                    if (r1 <= cfg.gate && r2 <= cfg.gate) {
                        const double c = fmax(r1, r2);
                        if (c < best) best = c, asg[j] = p;
                    }
                }
            }
            for (int p = 0; p < nb; ++p) {
                double S[NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, xmn = INFINITY, xmx = -INFINITY;
                int cn = 0;
#pragma unroll
                for (int j = 0; j < RPL; ++j) {
                    if (asg[j] != p) continue;
                    ++cn, xmn = fmin(xmn, X1[j]), xmx = fmax(xmx, X2[j]);
                    const double l = len[j];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const double X = e ? X2[j] : X1[j], Y = e ? Y2[j] : Y1[j], XX = X * X;
                        S[0] += l, S[1] += l * X, S[2] += l * XX, S[3] += l * (XX * X), S[4] += l * (XX * XX);
                        S[5] += l * Y, S[6] += l * (X * Y), S[7] += l * (XX * Y);
                    }
                }
#pragma unroll
                for (int q = 0; q < NSUM; ++q) S[q] = wave_sum_dpp(S[q]);
                cn = wave_sum_i(cn);
                xmx = wave_max(xmx), xmn = -wave_max(-xmn);
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < NSUM; ++q) sh.part[k][p][q] = S[q];
                    sh.part_n[k][p] = cn, sh.part_min[k][p] = xmn, sh.part_max[k][p] = xmx;
                }
            }
            __syncthreads();
            if (tid < nb) {
                double S[NSUM], xmn = sh.part_min[0][tid], xmx = sh.part_max[0][tid];
                int cn = sh.part_n[0][tid], views = cn > 0 ? 1 : 0;
#pragma unroll
                for (int q = 0; q < NSUM; ++q) S[q] = sh.part[0][tid][q];
                for (int c = 1; c < K; ++c) {
#pragma unroll
                    for (int q = 0; q < NSUM; ++q) S[q] += sh.part[c][tid][q];
                    cn += sh.part_n[c][tid], xmn = fmin(xmn, sh.part_min[c][tid]), xmx = fmax(xmx, sh.part_max[c][tid]);
                    if (sh.part_n[c][tid] > 0) views |= 1 << c;
                }
                int fl = sh.st_flags[tid] & AV_ROAD_BOUND_KEPT;
                double a[3];
                const bool quad = cn >= 3 && xmx - xmn >= cfg.span_quad;
                if (cn > 0 && fit_bound(S, quad, a)) {
                    sh.model[tid][0] = a[0], sh.model[tid][1] = a[1], sh.model[tid][2] = a[2];
                    if (quad) fl |= AV_ROAD_BOUND_QUAD;
                } else {
                    fl |= AV_ROAD_BOUND_KEPT | (sh.st_flags[tid] & AV_ROAD_BOUND_QUAD);
                }
                sh.st_flags[tid] = fl, sh.st_n[tid] = cn, sh.st_views[tid] = views, sh.st_s0[tid] = cn > 0 ? S[0] : 0.0;
                sh.st_xmin[tid] = cn > 0 ? xmn : 0.0, sh.st_xmax[tid] = cn > 0 ? xmx : 0.0;
            }
            __syncthreads();
        }
    }
    // ---- 5. - 7. ----
    if (tid == 0)
        finish(cfg, sh, K, dir_bin < 0, motion ? motion + v : nullptr, state + v, bounds + v * MAXB, info + v, row + v, n_ref + v,
               lane_offset + v);
    __syncthreads();
    if (tid < sh.n_ref) {                                                    // n_ref <= n_points <= min(rcap, 64)
        const double x0 = plan_state[v * 4], y0 = plan_state[v * 4 + 1], h = plan_state[v * 4 + 2];
        double sn, cs, s2, c2;
        sincos(h, &sn, &cs);
        sincos(h + 1.5707963267948966, &s2, &c2);
        const double step = (sh.x_end - cfg.path_near) / (double)(cfg.n_points - 1);
        const double X = cfg.path_near + (double)tid * step, Y = model_at(sh.centre, X);
        double* o = ref_path + (v * (size_t)rcap + (size_t)tid) * 2;
        o[0] = (x0 + X * cs) + Y * c2;
        o[1] = (y0 + X * sn) + Y * s2;
    }
}

int check_cfg(const av_road_lanes_cfg* c, const char* who) {
    AV_REQUIRE(c, AV_EINVAL, "%s: null cfg", who);
    const double d[16] = {c->min_len, c->slope_max, c->vote_len, c->x_vote, c->slope_tol, c->y_max, c->min_sep, c->gate, c->span_quad,
                          c->w_min, c->w_max, c->default_width, c->alpha, c->jump, c->path_near, c->path_far};
    static const char* const names[16] = {"min_len", "slope_max", "vote_len", "x_vote", "slope_tol", "y_max", "min_sep", "gate", "span_quad",
                                          "w_min", "w_max", "default_width", "alpha", "jump", "path_near", "path_far"};
    for (int i = 0; i < 16; ++i) AV_REQUIRE(std::isfinite(d[i]), AV_EINVAL, "%s: cfg %s must be finite", who, names[i]);
    for (int i = 0; i < 14; ++i)
        if (i != 1 && i != 10 && i != 12) AV_REQUIRE(d[i] > 0.0, AV_EINVAL, "%s: cfg %s must be > 0", who, names[i]);
    AV_REQUIRE(c->slope_max > 0.0 && c->slope_max <= 4.0, AV_EINVAL, "%s: cfg slope_max must be in (0, 4]", who);
    AV_REQUIRE(c->w_max >= c->w_min, AV_EINVAL, "%s: cfg w_max must be >= w_min", who);
    AV_REQUIRE(c->alpha >= 0.0 && c->alpha < 1.0, AV_EINVAL, "%s: cfg alpha must be in [0, 1)", who);
    AV_REQUIRE(c->path_near >= 0.0 && c->path_far > c->path_near, AV_EINVAL, "%s: cfg path_near must be >= 0 and path_far beyond it", who);
    AV_REQUIRE(c->min_votes >= 1, AV_EINVAL, "%s: cfg min_votes must be >= 1", who);
    AV_REQUIRE(c->max_coast >= 0, AV_EINVAL, "%s: cfg max_coast must be >= 0", who);
    AV_REQUIRE(c->one_sided == 0 || c->one_sided == 1, AV_EINVAL, "%s: cfg one_sided must be 0 or 1", who);
    AV_REQUIRE(c->n_points >= 2 && c->n_points <= 64, AV_EINVAL, "%s: cfg n_points %d not in 2..64", who, c->n_points);
    return AV_OK;
}

}  // namespace

extern "C" int av_road_lanes_check(const av_road_lanes_cfg* cfg) { return check_cfg(cfg, "av_road_lanes_check"); }

extern "C" size_t av_road_lanes_state_bytes(void) { return sizeof(av_road_lanes_state); }

extern "C" int av_road_lanes(av_ctx* ctx, av_stream_t stream, const av_road_lanes_cfg* cfg, int n_vehicles, int n_cams,
                             const av_ground_cfg* ground, const av_rig_mount* mounts, int max_segments, int scap, const int32_t* segments,
                             const int32_t* nseg, const av_egoflow_motion* motion, const double* plan_state, av_road_lanes_state* state,
                             av_road_lane_bound* bounds, av_road_lanes_info* info, av_road_lanes_row* row, int rcap, double* ref_path,
                             int32_t* n_ref, double* lane_offset) {
    static const char* const who = "av_road_lanes";
    if (int rc = check_cfg(cfg, who)) return rc;
    AV_REQUIRE(n_vehicles >= 1 && n_vehicles <= 65535, AV_EINVAL, "%s: n_vehicles %d not in 1..65535", who, n_vehicles);
    AV_REQUIRE(n_cams >= 1 && n_cams <= MAX_CAMS, AV_EINVAL, "%s: n_cams %d not in 1..%d", who, n_cams, MAX_CAMS);
    AV_REQUIRE(max_segments >= 1, AV_EINVAL, "%s: max_segments must be >= 1", who);
    AV_REQUIRE(scap >= 1 && scap <= MAX_SCAP, AV_EINVAL, "%s: scap %d not in 1..%d", who, scap, MAX_SCAP);
    AV_REQUIRE(cfg->n_points <= rcap, AV_EINVAL, "%s: cfg n_points %d exceeds rcap %d", who, cfg->n_points, rcap);
#define ROAD_LANES_PTR(p) AV_REQUIRE(p, AV_EINVAL, "%s: null " #p, who)
    ROAD_LANES_PTR(ground);
    ROAD_LANES_PTR(mounts);
    ROAD_LANES_PTR(segments);
    ROAD_LANES_PTR(nseg);
    ROAD_LANES_PTR(plan_state);
    ROAD_LANES_PTR(state);
    ROAD_LANES_PTR(bounds);
    ROAD_LANES_PTR(info);
    ROAD_LANES_PTR(row);
    ROAD_LANES_PTR(ref_path);
    ROAD_LANES_PTR(n_ref);
    ROAD_LANES_PTR(lane_offset);
    ROAD_LANES_PTR(ctx);
#undef ROAD_LANES_PTR
    hipLaunchKernelGGL(road_lanes_kernel, dim3((unsigned)n_vehicles), dim3(64 * (unsigned)n_cams), 0, as_stream(stream), *cfg, n_cams, ground,
                       mounts, max_segments, scap, segments, nseg, motion, plan_state, state, bounds, info, row, rcap, ref_path, n_ref,
                       lane_offset);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_road_lanes_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int vehicle, av_road_lanes_state* state) {
    AV_REQUIRE(n_vehicles >= 1 && n_vehicles <= 65535, AV_EINVAL, "av_road_lanes_reset: n_vehicles %d not in 1..65535", n_vehicles);
    AV_REQUIRE(vehicle >= -1 && vehicle < n_vehicles, AV_EINVAL, "av_road_lanes_reset: vehicle %d is neither -1 nor in 0..%d", vehicle,
               n_vehicles - 1);
    AV_REQUIRE(state, AV_EINVAL, "av_road_lanes_reset: null state");
    AV_REQUIRE(ctx, AV_EINVAL, "av_road_lanes_reset: null ctx");
    if (vehicle < 0) AV_HIP(hipMemsetAsync(state, 0, sizeof(av_road_lanes_state) * (size_t)n_vehicles, as_stream(stream)));
    else AV_HIP(hipMemsetAsync(state + vehicle, 0, sizeof(av_road_lanes_state), as_stream(stream)));
    return AV_OK;
}
