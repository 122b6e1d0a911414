// What the ground odometry's two translation units share (include/avhot.h: av_egoflow_* in egoflow.hip, av_rig_egoflow_* in
// rigflow.hip): the checked geometry, the stage launches of egoflow.hip, and the one device statement of the solve's pieces -- the
// "accepted" rule, the vote, a tile's displacement, the fit's elimination and the residual.
#pragma once
#include "common.h"

namespace egoflow {

constexpr int MAX_T = 32, MAX_R = 15, MAX_SIDE = 4096, MAX_BINS = (2 * MAX_R + 1) * (2 * MAX_R + 1);

struct Geom {
    int gh, gw, vw;                             // patch rows, columns, validity words per row
    int T, R, ty, tx, n_tiles;
};

// the header's checks of an av_egoflow_cfg; *g (if given) only on success
int geometry(const av_egoflow_cfg* c, const char* who, Geom* g);

// the stage launches (arguments already checked).  st: NULL (the stage entries: slot 0) or the states whose frame counters pick the
// ping-pong slot, camera `cam` reading st[cam / cams_per_state] (1: a state per camera; K: a state per vehicle of K cameras)
int launch_patch(av_stream_t stream, const av_egoflow_cfg* c, const Geom& g, const av_ground_cfg* ground, int n_cams, int h, int w,
                 const uint8_t* bgr, uint8_t* patch, size_t cam_stride, const av_egoflow_state* st, int cams_per_state, uint32_t* valid);
int launch_match(av_stream_t stream, const av_egoflow_cfg* c, const Geom& g, int n_cams, const uint8_t* cur, const uint8_t* prev,
                 size_t cam_stride, const av_egoflow_state* st, int cams_per_state, const uint32_t* valid, av_egoflow_tile* tiles);
int launch_measure(av_stream_t stream, const av_egoflow_cfg* c, int n_cams, const av_egoflow_motion* motion, av_egoflow_state* state,
                   double* z, uint8_t* mode);

// ---- the solve's pieces ----------------------------------------------------------------------------------------------------------
struct Fit {
    double tf, tl, om;
    int n;
    bool ok;
};
struct Disp {
    double df, dl;
};
// the six sums of the fit, a lane's or a wave's or a camera's
struct Sums {
    double sf, sl, q, b1, b2, b3;
};

// a row counts as accepted only with (dy, dx) inside the search range: the histogram's bounds do not rest on the caller's rows
__device__ __forceinline__ bool accepted(const av_egoflow_tile& t, int R) {
    return (t.flags & AV_EGOFLOW_ACCEPTED) && abs(t.dy) <= R && abs(t.dx) <= R;
}
__device__ __forceinline__ Disp displacement(const av_egoflow_tile& t, double m_per_px) {
    return Disp{-((double)t.dy + t.sub_dy) * m_per_px, ((double)t.dx + t.sub_dx) * m_per_px};
}
// a row at p = (f, l) with displacement d, added to a lane's sums
__device__ __forceinline__ void add_row(Sums& s, double f, double l, const Disp& d) {
    s.sf += f, s.sl += l, s.q += f * f + l * l, s.b1 += d.df, s.b2 += d.dl, s.b3 += f * d.dl - l * d.df;
}
__device__ __forceinline__ double residual2(double f, double l, const Disp& d, const Fit& fit) {
    const double rf = d.df - (fit.tf - fit.om * l), rl = d.dl - (fit.tl + fit.om * f);
    return rf * rf + rl * rl;
}
// the header's elimination from the whole set's sums
__device__ __forceinline__ Fit fit_of_sums(int count, const Sums& s) {
    Fit r{0.0, 0.0, 0.0, count, false};
    if (r.n < 1) return r;
    const double n = (double)r.n;
    const double den = (s.q - (s.sl * s.sl) / n) - (s.sf * s.sf) / n;
    if (!(den > 1e-9 * s.q)) return r;
    r.om = ((s.b3 + (s.sl * s.b1) / n) - (s.sf * s.b2) / n) / den;
    r.tf = (s.b1 + r.om * s.sl) / n;
    r.tl = (s.b2 - r.om * s.sf) / n;
    r.ok = true;
    return r;
}
// a wave's sums from its lanes': the wave's fixed tree
__device__ __forceinline__ Sums wave_sums(const Sums& s) {
    return Sums{wave_sum_dpp(s.sf), wave_sum_dpp(s.sl), wave_sum_dpp(s.q), wave_sum_dpp(s.b1), wave_sum_dpp(s.b2), wave_sum_dpp(s.b3)};
}

// the vote of one wave over one camera's table: hist is the wave's own (2R+1)^2 ints of LDS.  -> the mode's bin (the fullest, among
// equals the first in row-major (dy, dx) order; the centre where nothing is accepted); n_acc: the accepted rows.  Every wave of the
// workgroup calls it together (the barriers are the workgroup's).
__device__ __forceinline__ int vote(int* hist, const av_egoflow_tile* __restrict__ tl, int n_tiles, int R, int lane, int& n_acc) {
    const int C1 = 2 * R + 1, C = C1 * C1;
    for (int b = lane; b < C; b += 64) hist[b] = 0;
    __syncthreads();
    int n = 0;
    for (int k = lane; k < n_tiles; k += 64) {
        const av_egoflow_tile t = tl[k];
        if (accepted(t, R)) atomicAdd(&hist[(t.dy + R) * C1 + (t.dx + R)], 1), ++n;
    }
    n_acc = wave_sum_i(n);
    __syncthreads();
    unsigned key = 0;                                               // count << 10 | (1023 - bin): the fullest bin, then the first
    for (int b = lane; b < C; b += 64)
        if (hist[b] > 0) key = max(key, ((unsigned)hist[b] << 10) | (unsigned)(1023 - b));
    key = wave_max_u32(key);
    return key ? 1023 - (int)(key & 1023u) : R * C1 + R;
}

}  // namespace egoflow
