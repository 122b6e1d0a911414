// Per-track constant-velocity Kalman filter over the tracker's snapshot tables (av_track_filter_update): the SORT filter, fed the
// matched centres, predicting through misses, with a state of its own keyed by the row's slot.
//
// The reference has no such filter (what it has is Track.velocity, the last centre difference, multi_object_tracker.py:35-47, and
// predict_next_position); include/avhot.h states the equations.  State (cx, cy, vx, vy), F the unit-step constant-velocity
// transition, Q = q_accel G G^T, H = [I2 0], R = r_meas I2.  x and y never mix: F, Q, H, R and the initial P are the same 2 x 2
// block for either axis, so P stays block-diagonal with two EQUAL blocks that depend only on the track's hit / miss pattern.  The
// kernel keeps that one block (ppp, ppv, pvv) and updates it in Joseph form.
//
// Mapping: one workgroup per stream, tcap threads (1 .. 16 waves), thread = table row within a frame.  The frames of a window
// are a serial chain; the slot table (8 words per slot) lives in LDS for the whole window, structure-of-arrays, so a frame costs
// one LDS round trip and one barrier, no trip to HBM: slots are unique among the live rows of a frame (tracker_dev.h), so the
// threads of a frame touch disjoint slots, and the barrier orders a slot's hand-over to whichever thread holds its row in the
// next frame.  The pieces of a row that the filter reads (id .. x2 | y2 | misses, slot) and the frame's row count are fetched
// three frames ahead into registers, without a branch around the loads; the chain never waits for a load it has just issued.
// Global state is read once at the start and written once at the end.  float64, -ffp-contract=off: no FMA.
#include "common.h"

#include <cmath>

namespace {

constexpr int HDR_BYTES = 64;          // int32 hdr[16]; hdr[0] = status
constexpr int SLOT_BYTES = 64;         // int32 id, int32 reserved (0), double x[4] (cx, cy, vx, vy), double p[3] (ppp, ppv, pvv)

__host__ __device__ inline size_t state_bytes(int tcap) { return (size_t)HDR_BYTES + (size_t)tcap * SLOT_BYTES; }

struct FilterRow {                     // what the filter reads of a frame: the row's three pieces and the frame's row count
    int4 a;                            // id, x1, y1, x2
    int y2;
    int2 m;                            // misses, slot
    int n;
};

// Row t of frame f (t < tcap, f < n_frames: always inside snap, whether the row is live or not) and the frame's count.  No branch
// around the loads: they are issued in program order and waited for by count.
__device__ __forceinline__ FilterRow fetch_row(const av_track_row* rows, const int32_t* cnt, int f, int t, int tcap) {
    FilterRow r;
    const char* p = reinterpret_cast<const char*>(rows + (size_t)f * tcap + t);
    r.a = *reinterpret_cast<const int4*>(p);
    r.y2 = *reinterpret_cast<const int*>(p + 16);
    r.m = *reinterpret_cast<const int2*>(p + 32);
    r.n = cnt[f];
    return r;
}

__device__ __forceinline__ int clamp_n(int n, int tcap) { return n < 0 ? 0 : (n > tcap ? tcap : n); }

__global__ void __launch_bounds__(1024) track_filter_kernel(av_track_filter_cfg cfg, int n_frames, int tcap,
                                                            const av_track_row* __restrict__ snap,
                                                            const int32_t* __restrict__ snap_n, unsigned char* __restrict__ state,
                                                            double* __restrict__ filt) {
    extern __shared__ double lds[];                                 // 7 double arrays of tcap, then the ids
    const int t = threadIdx.x, s = blockIdx.x;                      // blockDim.x == tcap
    double* const l_cx = lds;
    double* const l_cy = lds + tcap;
    double* const l_vx = lds + 2 * tcap;
    double* const l_vy = lds + 3 * tcap;
    double* const l_ppp = lds + 4 * tcap;
    double* const l_ppv = lds + 5 * tcap;
    double* const l_pvv = lds + 6 * tcap;
    int* const l_id = reinterpret_cast<int*>(lds + 7 * tcap);

    unsigned char* const st = state + (size_t)s * state_bytes(tcap);
    double* const mine = reinterpret_cast<double*>(st + HDR_BYTES + (size_t)t * SLOT_BYTES);     // slot t of this stream
    {
        const double2 w0 = *reinterpret_cast<const double2*>(mine), w1 = *reinterpret_cast<const double2*>(mine + 2);
        const double2 w2 = *reinterpret_cast<const double2*>(mine + 4), w3 = *reinterpret_cast<const double2*>(mine + 6);
        l_id[t] = __double2loint(w0.x);
        l_cx[t] = w0.y, l_cy[t] = w1.x, l_vx[t] = w1.y, l_vy[t] = w2.x, l_ppp[t] = w2.y, l_ppv[t] = w3.x, l_pvv[t] = w3.y;
    }
    const av_track_row* const rows = snap + (size_t)s * n_frames * tcap;
    const int32_t* const cnt = snap_n + (size_t)s * n_frames;
    double* const out = filt + (size_t)s * n_frames * tcap * 6;

    const double q4 = cfg.q_accel / 4.0, q2 = cfg.q_accel / 2.0, q = cfg.q_accel, rm = cfg.r_meas;
    const int last = n_frames - 1;
    bool bad = false;
    // One frame.  `r` holds the frame's row, fetched three frames ago; once the frame is done with it, it is refilled with frame
    // f + 3's, so the rows of the next two to three frames are in flight while a frame is computed.  (Past the window the last
    // frame is fetched again and never used.)  The loop below is unrolled by three and the refill follows the last use, so the
    // three buffers stay in their registers: a move from a buffer would have to wait for the newest load.
    auto frame = [&](int f, FilterRow& r) {
        if (t < clamp_n(r.n, tcap)) {
            const int k = r.m.y;
            double cx, cy, vx, vy, sp, sv;
            if (k < 0 || k >= tcap) {                                // a hand-made table: skipped, reported
                bad = true;
                cx = cy = vx = vy = sp = sv = 0.0;
            } else {
                const double zx = (double)(r.a.y + r.a.w) / 2.0, zy = (double)(r.a.z + r.y2) / 2.0;
                double ppp, ppv, pvv;
                if (l_id[k] != r.a.x) {                              // birth
                    l_id[k] = r.a.x;
                    cx = zx, cy = zy, vx = 0.0, vy = 0.0;
                    ppp = cfg.p0_pos, ppv = 0.0, pvv = cfg.p0_vel;
                } else {                                             // x <- F x, P <- F P F^T + Q
                    vx = l_vx[k], vy = l_vy[k];
                    cx = l_cx[k] + vx, cy = l_cy[k] + vy;
                    const double a = l_ppp[k], b = l_ppv[k], c = l_pvv[k];
                    ppp = ((a + b) + (b + c)) + q4;
                    ppv = (b + c) + q2;
                    pvv = c + q;
                }
                if (r.m.x == 0) {                                    // K = P H^T / (H P H^T + R), Joseph form
                    const double sx = ppp + rm;
                    const double k0 = ppp / sx, k1 = ppv / sx;
                    const double yx = zx - cx, yy = zy - cy;
                    cx = cx + k0 * yx, cy = cy + k0 * yy;
                    vx = vx + k1 * yx, vy = vy + k1 * yy;
                    const double a1 = 1.0 - k0;
                    const double m01 = ppv - k1 * ppp;               // ((I - KH) P)[1][0]
                    const double npp = (a1 * ppp) * a1 + (rm * k0) * k0;
                    const double npv = a1 * m01 + (rm * k0) * k1;
                    const double nvv = ((pvv - k1 * ppv) - k1 * m01) + (rm * k1) * k1;
                    ppp = npp, ppv = npv, pvv = nvv;
                }
                l_cx[k] = cx, l_cy[k] = cy, l_vx[k] = vx, l_vy[k] = vy, l_ppp[k] = ppp, l_ppv[k] = ppv, l_pvv[k] = pvv;
                sp = sqrt(ppp + ppp), sv = sqrt(pvv + pvv);
            }
            double2* const o = reinterpret_cast<double2*>(out + ((size_t)f * tcap + t) * 6);
            o[0] = make_double2(cx, cy), o[1] = make_double2(vx, vy), o[2] = make_double2(sp, sv);
        }
        r = fetch_row(rows, cnt, f + 3 < last ? f + 3 : last, t, tcap);
        __syncthreads();
    };
    FilterRow b0 = fetch_row(rows, cnt, 0, t, tcap), b1 = fetch_row(rows, cnt, 1 < last ? 1 : last, t, tcap);
    FilterRow b2 = fetch_row(rows, cnt, 2 < last ? 2 : last, t, tcap);
    __syncthreads();
    int f = 0;
    for (; f + 3 <= n_frames; f += 3) {
        frame(f, b0);
        frame(f + 1, b1);
        frame(f + 2, b2);
    }
    if (f < n_frames) frame(f, b0);                                  // (uniform: every thread meets every barrier)
    if (f + 1 < n_frames) frame(f + 1, b1);
    {
        double2* const m2 = reinterpret_cast<double2*>(mine);
        m2[0] = make_double2(__hiloint2double(0, l_id[t]), l_cx[t]);
        m2[1] = make_double2(l_cy[t], l_vx[t]);
        m2[2] = make_double2(l_vy[t], l_ppp[t]);
        m2[3] = make_double2(l_ppv[t], l_pvv[t]);
    }
    if (bad) atomicOr(reinterpret_cast<int*>(st), 1);
}

__global__ void __launch_bounds__(256) track_filter_reset_kernel(size_t n_words, int words_per_stream, int2* __restrict__ state) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;         // one 8-byte word each
    if (i >= n_words) return;
    const int w = (int)(i % (size_t)words_per_stream);
    const bool id_word = w >= HDR_BYTES / 8 && (w - HDR_BYTES / 8) % (SLOT_BYTES / 8) == 0;
    state[i] = make_int2(id_word ? -1 : 0, 0);
}

bool tcap_ok(int tcap) { return tcap >= 64 && tcap <= 1024 && (tcap % 64) == 0; }

}  // namespace

extern "C" {

size_t av_track_filter_state_bytes(int tcap) { return tcap <= 0 ? 0 : state_bytes(tcap); }

int av_track_filter_reset(av_ctx* ctx, av_stream_t stream, int n_streams, int tcap, void* state) {
    AV_REQUIRE(ctx && state, AV_EINVAL, "av_track_filter_reset: null argument");
    AV_REQUIRE(n_streams > 0, AV_EINVAL, "av_track_filter_reset: n_streams must be > 0");
    AV_REQUIRE(tcap_ok(tcap), AV_EINVAL, "av_track_filter_reset: tcap %d must be a multiple of 64 in [64,1024]", tcap);
    const int per = (int)(state_bytes(tcap) / 8);
    const size_t n_words = (size_t)n_streams * per;
    AV_REQUIRE((n_words + 255) / 256 <= 0x7fffffffull, AV_EINVAL, "av_track_filter_reset: n_streams %d is too large", n_streams);
    hipLaunchKernelGGL(track_filter_reset_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, as_stream(stream), n_words, per,
                       (int2*)state);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_track_filter_update(av_ctx* ctx, av_stream_t stream, const av_track_filter_cfg* cfg, int n_streams, int n_frames, int tcap,
                           const av_track_row* snap, const int32_t* snap_n, void* state, double* filt) {
    AV_REQUIRE(ctx && cfg && snap && snap_n && state && filt, AV_EINVAL, "av_track_filter_update: null argument");
    AV_REQUIRE(n_streams > 0 && n_frames > 0, AV_EINVAL, "av_track_filter_update: n_streams/n_frames must be > 0");
    AV_REQUIRE(tcap_ok(tcap), AV_EINVAL, "av_track_filter_update: tcap %d must be a multiple of 64 in [64,1024]", tcap);
    AV_REQUIRE(std::isfinite(cfg->q_accel) && cfg->q_accel >= 0.0, AV_EINVAL, "av_track_filter_update: q_accel must be finite and >= 0");
    AV_REQUIRE(std::isfinite(cfg->r_meas) && cfg->r_meas > 0.0, AV_EINVAL, "av_track_filter_update: r_meas must be finite and > 0");
    AV_REQUIRE(std::isfinite(cfg->p0_pos) && cfg->p0_pos >= 0.0 && std::isfinite(cfg->p0_vel) && cfg->p0_vel >= 0.0, AV_EINVAL,
               "av_track_filter_update: p0_pos and p0_vel must be finite and >= 0");
    hipLaunchKernelGGL(track_filter_kernel, dim3(n_streams), dim3(tcap), (size_t)tcap * 60, as_stream(stream), *cfg, n_frames, tcap, snap,
                       snap_n, (unsigned char*)state, filt);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"
