// Vehicle-frame tracks (av_rig_track): av_rig_fuse's list followed over time -- a multi-object tracker in the planner's frame with a
// persistent state per vehicle and a constant-velocity Kalman filter per track, so a fused obstacle keeps its id across frames and
// cameras and coasts through the frames in which nobody sees it.
//
// The reference tracks boxes in one camera's image (multi_object_tracker.py); what this kernel takes from it is the greedy
// association (:136-159: best pair first, each row and each column taken once) and the max_age / min_hits life cycle, with
// av_rig_fuse's squared distance and gate in place of the IoU (rig_dev.h).  Semantics and operation order: include/avhot.h.
//
// Mapping: one workgroup per vehicle, max(tcap, ocap_in) threads rounded up to whole waves (1 .. 8).  Thread t owns slot t (its 96
// bytes live in registers from the first load to the last store) and row t of the input.  The predicted slots (x, y, r, taken) and
// the kept rows live in LDS, 43 KB.  The association is the header's greedy one, run in rounds that take many pairs at once:
// thread j keeps, for its row, the nearest admissible slot still free (the smallest slot among equals), and thread i, for its slot,
// the nearest admissible row still free (the smallest row among equals); either scan reads one entry at a time, the same for all
// lanes (an LDS broadcast).  A pair that is each other's choice has the smallest (d2, slot, row) of all pairs that share its slot
// or its row, so the serial greedy pass takes it whatever else it takes first: a round takes every such pair, and then only the
// threads whose choice was just taken scan again.  While an admissible pair is left, the one with the smallest (d2, slot, row) of
// all is mutual, so a round takes at least one pair and the rounds are bounded by min(live slots, kept rows) <= 512; a scene whose
// rows each lie nearest to their own track is done in one round.  (A first version ran the pass serially, one pair per iteration
// with a workgroup-wide minimum: DESIGN.md section 7p has both timings.)  Births and the output compaction are ballots and prefix
// counts over the waves.  float64, -ffp-contract=off: every operation rounded on its own.
//
// The class form (av_rig_track_cls) is the same kernel with an int32 lane beside the rows: a slot's first reserved word holds the
// class of its latest classified row plus one, and the word travels with the slot's other integers.  The association never reads it.
#include "rig_dev.h"

#include <cmath>

static_assert(sizeof(av_rig_track_cfg) == 72, "av_rig_track_cfg is 8 doubles and 2 int32 (include/avhot.h)");

namespace {

constexpr int MAX_T = 512, MAX_IN = 512, MAX_WAVES = 8;
constexpr int HDR_BYTES = 64;          // int32 hdr[16]: status, next id, frames, live
constexpr int SLOT_BYTES = 96;         // int32 id, hits, misses, age, views, views_ever, 2 reserved (the first: class + 1); double x[4], p[3], r
static_assert(HDR_BYTES % 16 == 0 && SLOT_BYTES % 16 == 0, "slots are read and written 16 bytes at a time");

__host__ __device__ inline size_t state_bytes(int tcap) { return (size_t)HDR_BYTES + (size_t)tcap * SLOT_BYTES; }

struct Shared {
    double X[MAX_T], Y[MAX_T], R[MAX_T];                                     // the slots, predicted
    double cX[MAX_IN], cY[MAX_IN], cR[MAX_IN], cVX[MAX_IN], cVY[MAX_IN];     // the kept rows, at their row index
    int32_t cViews[MAX_IN];
    int32_t cCls[MAX_IN];                                                    // (av_rig_track_cls: the rows' classes)
    int32_t taken[MAX_T];                                                    // the slot takes no (further) row: free, or matched
    int32_t row_taken[MAX_IN];                                               // the row takes no (further) slot: not kept, or matched
    int32_t row_best[MAX_IN];                                                // a round's post: the slot row j would take, -1: none
    int32_t birth_row[MAX_IN];                                               // the b-th row to be born
    int32_t took[2];                                                         // a round took a pair (rounds alternate between the two)
    int32_t n_skipped[MAX_WAVES], n_free[MAX_WAVES], n_birth[MAX_WAVES], n_conf[MAX_WAVES], n_live[MAX_WAVES];
};

// row (x, y, r) against the slots 0 .. tcap - 1 that are still free to be matched: the nearest admissible one, the smallest index
// among equals
__device__ __forceinline__ void scan_slots(const Shared& sh, const av_rig_track_cfg& cfg, int tcap, double x, double y, double r,
                                           double& bd, int& bi) {
    bd = INFINITY, bi = -1;
    for (int i = 0; i < tcap; ++i) {
        if (sh.taken[i]) continue;
        double d2;
        if (rig_pair(sh.X[i], sh.Y[i], sh.R[i], x, y, r, cfg.gate_min, cfg.gate_scale, d2) && d2 < bd) bd = d2, bi = i;
    }
}

// slot (X, Y, R) against the rows 0 .. n - 1 that are still free to be matched: the nearest admissible one, the smallest index among
// equals (the same pair test with the same operands as scan_slots: a pair has one d2, whichever side computes it)
__device__ __forceinline__ int scan_rows(const Shared& sh, const av_rig_track_cfg& cfg, int n, double X, double Y, double R) {
    double bd = INFINITY;
    int bj = -1;
    for (int j = 0; j < n; ++j) {
        if (sh.row_taken[j]) continue;
        double d2;
        if (rig_pair(X, Y, R, sh.cX[j], sh.cY[j], sh.cR[j], cfg.gate_min, cfg.gate_scale, d2) && d2 < bd) bd = d2, bj = j;
    }
    return bj;
}

// the sum of a per-wave count over the waves in front of wave w, and over all nw waves
__device__ __forceinline__ void wave_prefix(const int32_t* cnt, int w, int nw, int& before, int& total) {
    before = total = 0;
    for (int q = 0; q < nw; ++q) {
        const int c = cnt[q];
        before += q < w ? c : 0;
        total += c;
    }
}

template <int NCOL>
__global__ void __launch_bounds__(MAX_T) rig_track_kernel(av_rig_track_cfg cfg, int tcap, int ocap_in, const double* __restrict__ obs_in,
                                                         const int32_t* __restrict__ n_in, const int32_t* __restrict__ views_in,
                                                         const double* __restrict__ plan_state, unsigned char* __restrict__ state,
                                                         int ocap_out, double* __restrict__ obstacles, int32_t* __restrict__ n_obs,
                                                         int32_t* __restrict__ obs_slot, int32_t* __restrict__ match,
                                                         int32_t* __restrict__ n_skip, int32_t* __restrict__ n_drop,
                                                         const int32_t* __restrict__ cls_in, int32_t* __restrict__ cls_out) {
    constexpr bool MOVING = NCOL == 5;
    __shared__ Shared sh;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, nw = (int)blockDim.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const size_t v = blockIdx.x;
    unsigned char* const st = state + v * state_bytes(tcap);
    int32_t* const hdr = reinterpret_cast<int32_t*>(st);
    const int next_id = hdr[1];
    const double x0 = plan_state[v * 4], y0 = plan_state[v * 4 + 1];
    const bool own = tid < tcap;                                             // this thread owns slot tid
    // ---- slot tid: load, predict, post ----
    int id = -1, hits = 0, misses = 0, age = 0, views = 0, views_ever = 0;
    unsigned cls1 = 0;                                                       // the slot's first reserved word: class + 1, 0: none known
    double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0, pa = 0.0, pb = 0.0, pc = 0.0, rad = 0.0;
    unsigned char* const mine = st + HDR_BYTES + (size_t)tid * SLOT_BYTES;   // (only dereferenced when own)
    if (own) {
        const int4 i0 = *reinterpret_cast<const int4*>(mine);
        const int4 i1 = *reinterpret_cast<const int4*>(mine + 16);
        const double2 d0 = *reinterpret_cast<const double2*>(mine + 32), d1 = *reinterpret_cast<const double2*>(mine + 48);
        const double2 d2 = *reinterpret_cast<const double2*>(mine + 64), d3 = *reinterpret_cast<const double2*>(mine + 80);
        id = i0.x, hits = i0.y, misses = i0.z, age = i0.w, views = i1.x, views_ever = i1.y, cls1 = (unsigned)i1.z;
        x = d0.x, y = d0.y, vx = d1.x, vy = d1.y, pa = d2.x, pb = d2.y, pc = d3.x, rad = d3.y;
        if (id >= 0) {                                                       // x <- F x, P <- F P F^T + Q
            const double dt = cfg.dt, dt2 = dt * dt;
            const double q11 = cfg.q_accel * ((dt2 * dt2) / 4.0), q12 = cfg.q_accel * ((dt2 * dt) / 2.0), q22 = cfg.q_accel * dt2;
            x = x + vx * dt, y = y + vy * dt;
            const double bc = pb + dt * pc;
            pa = ((pa + dt * pb) + dt * bc) + q11;
            pb = bc + q12;
            pc = pc + q22;
            age += 1;
        }
        sh.X[tid] = x, sh.Y[tid] = y, sh.R[tid] = rad;
        sh.taken[tid] = id < 0;
    }
    // ---- row tid: load, keep or skip ----
    int n = n_in[v];
    n = n < 0 ? 0 : (n > ocap_in ? ocap_in : n);
    bool keep = false;
    double zx = 0.0, zy = 0.0, zr = 0.0;
    if (tid < ocap_in) {                                                     // (inside the list whatever n is)
        const double* row = obs_in + (v * (size_t)ocap_in + (size_t)tid) * NCOL;
        zx = row[0], zy = row[1], zr = row[2];
        keep = tid < n && std::isfinite(zx) && std::isfinite(zy) && std::isfinite(zr) && zr > 0.0;
        double zvx = 0.0, zvy = 0.0;
        if constexpr (MOVING) {
            zvx = row[3], zvy = row[4];
            keep = keep && std::isfinite(zvx) && std::isfinite(zvy);
        }
        const int zviews = views_in ? views_in[v * (size_t)ocap_in + (size_t)tid] : 0;
        const int zcls = cls_in ? cls_in[v * (size_t)ocap_in + (size_t)tid] : -1;
        if (keep) {
            sh.cX[tid] = zx, sh.cY[tid] = zy, sh.cR[tid] = zr, sh.cViews[tid] = zviews, sh.cCls[tid] = zcls;
            if constexpr (MOVING) sh.cVX[tid] = zvx, sh.cVY[tid] = zvy;
        }
        sh.row_taken[tid] = !keep;
    }
    if (tid == 0) sh.took[0] = 0, sh.took[1] = 0;
    const bool skipped = tid < n && !keep;
    {
        const int c = __popcll(__ballot(skipped));
        if (lane == 0) sh.n_skipped[w] = c;
    }
    __syncthreads();
    // ---- association: rounds of mutual choices ----
    bool active = keep;                                                      // the row still looks for a slot
    bool open = own && id >= 0;                                              // the slot still looks for a row
    bool matched = false;
    double bd = INFINITY;
    int bi = -1, sj = -1, my_row = -1;
    if (active) scan_slots(sh, cfg, tcap, zx, zy, zr, bd, bi);
    if (open) sj = scan_rows(sh, cfg, n, x, y, rad);
    for (int round = 0;; ++round) {                                          // (every thread runs the same rounds: barriers inside)
        if (tid < ocap_in) sh.row_best[tid] = active ? bi : -1;
        __syncthreads();
        if (tid == 0) sh.took[(round + 1) & 1] = 0;                          // (last read before this round's barrier, next set behind the next)
        if (open && sj >= 0 && sh.row_best[sj] == tid) {                     // each other's choice; sj < n <= ocap_in
            open = false, my_row = sj;
            sh.taken[tid] = 1, sh.row_taken[sj] = 1, sh.took[round & 1] = 1;
        }
        __syncthreads();
        if (!sh.took[round & 1]) break;                                      // (uniform: read behind the barrier, cleared a round later)
        if (active && sh.row_taken[tid]) active = false, matched = true;
        if (active && bi >= 0 && sh.taken[bi]) scan_slots(sh, cfg, tcap, zx, zy, zr, bd, bi);   // the slot this row chose is gone
        if (open && sj >= 0 && sh.row_taken[sj]) sj = scan_rows(sh, cfg, n, x, y, rad);         // the row this slot chose is gone
    }
    // ---- matched slots: the Kalman update; unmatched live slots: a miss, and death ----
    if (own && id >= 0) {
        const int j = my_row;
        if (j >= 0) {
            const double mx = sh.cX[j], my = sh.cY[j];
            const double ex = mx - x0, ey = my - y0;
            const double m = fmax(ex * ex + ey * ey, 1.0);
            const double R = cfg.r_meas + cfg.r_range * (m * m);
            const double S = pa + R;
            const double k0 = pa / S, k1 = pb / S;
            const double yx = mx - x, yy = my - y;
            x = x + k0 * yx, vx = vx + k1 * yx;
            y = y + k0 * yy, vy = vy + k1 * yy;
            const double na = pa - k0 * pa, nb = pb - k0 * pb, nc = pc - k1 * pb;
            pa = na, pb = nb, pc = nc;
            rad = sh.cR[j];
            hits += 1, misses = 0;
            views = sh.cViews[j], views_ever |= views;
            if (cls_in && sh.cCls[j] >= 0) cls1 = (unsigned)sh.cCls[j] + 1u;  // the latest observation wins; a row without a class leaves it
            if (match) match[v * (size_t)ocap_in + (size_t)j] = id;
        } else {
            misses += 1, views = 0;
            if (misses > cfg.max_age) {
                id = -1, hits = misses = age = views_ever = 0, cls1 = 0u;
                x = y = vx = vy = pa = pb = pc = rad = 0.0;
            }
        }
    }
    // ---- births: the b-th kept row left over goes to the b-th free slot ----
    const bool is_free = own && id < 0, wants = keep && !matched;
    const unsigned long long fm = __ballot(is_free), bm = __ballot(wants);
    if (lane == 0) sh.n_free[w] = __popcll(fm), sh.n_birth[w] = __popcll(bm);
    __syncthreads();
    int free_rank, n_free, birth_rank, n_wants;
    wave_prefix(sh.n_free, w, nw, free_rank, n_free);
    wave_prefix(sh.n_birth, w, nw, birth_rank, n_wants);
    free_rank += __popcll(fm & below), birth_rank += __popcll(bm & below);
    const int n_born = n_wants < n_free ? n_wants : n_free;
    if (wants) {
        sh.birth_row[birth_rank] = tid;                                      // birth_rank < n_wants <= ocap_in
        if (match) match[v * (size_t)ocap_in + (size_t)tid] = birth_rank < n_free ? next_id + birth_rank : -2;
    }
    if (skipped && match) match[v * (size_t)ocap_in + (size_t)tid] = -1;
    __syncthreads();
    if (is_free && free_rank < n_born) {
        const int j = sh.birth_row[free_rank];
        id = next_id + free_rank;
        x = sh.cX[j], y = sh.cY[j], rad = sh.cR[j];
        if constexpr (MOVING) vx = sh.cVX[j], vy = sh.cVY[j];
        else vx = 0.0, vy = 0.0;
        pa = cfg.p0_pos, pb = 0.0, pc = cfg.p0_vel;
        hits = 1, misses = 0, age = 0;
        views = views_ever = sh.cViews[j];
        if (cls_in) cls1 = sh.cCls[j] >= 0 ? (unsigned)sh.cCls[j] + 1u : 0u;
    }
    // ---- the state back; the confirmed slots, compacted in slot order ----
    const bool live = own && id >= 0, conf = live && hits >= cfg.min_hits;
    const unsigned long long cm = __ballot(conf);
    {
        const int c = __popcll(__ballot(live));
        if (lane == 0) sh.n_conf[w] = __popcll(cm), sh.n_live[w] = c;
    }
    if (own) {
        *reinterpret_cast<int4*>(mine) = make_int4(id, hits, misses, age);
        *reinterpret_cast<int4*>(mine + 16) = make_int4(views, views_ever, (int)cls1, 0);
        double2* const o = reinterpret_cast<double2*>(mine + 32);
        o[0] = make_double2(x, y), o[1] = make_double2(vx, vy), o[2] = make_double2(pa, pb), o[3] = make_double2(pc, rad);
    }
    __syncthreads();
    int out_row, n_out;
    wave_prefix(sh.n_conf, w, nw, out_row, n_out);
    out_row += __popcll(cm & below);
    if (conf) {                                                              // out_row < tcap <= ocap_out
        double* o = obstacles + (v * (size_t)ocap_out + (size_t)out_row) * NCOL;
        o[0] = x, o[1] = y, o[2] = rad;
        if constexpr (MOVING) o[3] = vx, o[4] = vy;
        if (obs_slot) obs_slot[v * (size_t)ocap_out + (size_t)out_row] = tid;
        if (cls_out) cls_out[v * (size_t)ocap_out + (size_t)out_row] = (int)(cls1 - 1u);
    }
    if (tid == 0) {
        int n_live = 0, n_skipped = 0;
        for (int q = 0; q < nw; ++q) n_live += sh.n_live[q], n_skipped += sh.n_skipped[q];
        const int dropped = n_wants - n_born;
        hdr[0] = hdr[0] | (dropped > 0 ? 1 : 0);
        hdr[1] = next_id + n_born;
        hdr[2] = hdr[2] + 1;
        hdr[3] = n_live;
        n_obs[v] = n_out;
        if (n_skip) n_skip[v] = n_skipped;
        if (n_drop) n_drop[v] = dropped;
    }
}

__global__ void __launch_bounds__(256) rig_track_reset_kernel(size_t n_words, int words_per_vehicle, int2* __restrict__ state) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;                 // one 8-byte word each
    if (i >= n_words) return;
    const int wd = (int)(i % (size_t)words_per_vehicle);
    const bool id_word = wd >= HDR_BYTES / 8 && (wd - HDR_BYTES / 8) % (SLOT_BYTES / 8) == 0;
    state[i] = wd == 0 ? make_int2(0, 1) : make_int2(id_word ? -1 : 0, 0);   // (status, next id); (id, hits)
}

bool tcap_ok(int tcap) { return tcap >= 1 && tcap <= MAX_T; }

}  // namespace

extern "C" {

size_t av_rig_track_state_bytes(int tcap) { return tcap_ok(tcap) ? state_bytes(tcap) : 0; }

int av_rig_track_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int tcap, void* state) {
    AV_REQUIRE(n_vehicles >= 1, AV_EINVAL, "av_rig_track_reset: n_vehicles must be >= 1");
    AV_REQUIRE(tcap_ok(tcap), AV_EINVAL, "av_rig_track_reset: tcap %d not in 1..%d", tcap, MAX_T);
    AV_REQUIRE(ctx && state, AV_EINVAL, "av_rig_track_reset: null argument");
    const int per = (int)(state_bytes(tcap) / 8);
    const size_t n_words = (size_t)n_vehicles * per;
    hipLaunchKernelGGL(rig_track_reset_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, as_stream(stream), n_words, per,
                       (int2*)state);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

static int rig_track(const char* who, av_ctx* ctx, av_stream_t stream, const av_rig_track_cfg* cfg, int n_vehicles, int tcap, int ncol, int ocap_in,
                 const double* obs_in, const int32_t* n_in, const int32_t* views_in, const double* plan_state, void* state,
                 int ocap_out, double* obstacles, int32_t* n_obs, int32_t* obs_slot, int32_t* match, int32_t* n_skip,
                 int32_t* n_drop, const int32_t* cls_in, int32_t* cls_out) {
    AV_REQUIRE(n_vehicles >= 1, AV_EINVAL, "%s: n_vehicles must be >= 1", who);
    AV_REQUIRE(tcap_ok(tcap), AV_EINVAL, "%s: tcap %d not in 1..%d", who, tcap, MAX_T);
    AV_REQUIRE(ncol == 3 || ncol == 5, AV_EINVAL, "%s: ncol %d is neither 3 (x, y, r) nor 5 (x, y, r, vx, vy)", who, ncol);
    AV_REQUIRE(ocap_in >= 1 && ocap_in <= MAX_IN, AV_EINVAL, "%s: ocap_in %d not in 1..%d", who, ocap_in, MAX_IN);
    AV_REQUIRE(ocap_out >= tcap, AV_EINVAL, "%s: ocap_out %d < tcap %d (every track may be confirmed)", who, ocap_out, tcap);
    AV_REQUIRE(cfg, AV_EINVAL, "%s: null cfg", who);
    const double* d = &cfg->dt;
    for (int i = 0; i < 8; ++i)
        AV_REQUIRE(std::isfinite(d[i]) && d[i] >= 0.0, AV_EINVAL, "%s: cfg double %d (dt, q_accel, r_meas, r_range, p0_pos, "
                   "p0_vel, gate_scale, gate_min) must be finite and >= 0", who, i);
    AV_REQUIRE(cfg->dt > 0.0 && cfg->r_meas > 0.0, AV_EINVAL, "%s: cfg dt and r_meas must be > 0", who);
    AV_REQUIRE(cfg->max_age >= 0 && cfg->min_hits >= 1, AV_EINVAL, "%s: cfg max_age must be >= 0 and min_hits >= 1", who);
    AV_REQUIRE(ctx && obs_in && n_in && plan_state && state && obstacles && n_obs, AV_EINVAL, "%s: null argument", who);
    const int most = tcap > ocap_in ? tcap : ocap_in;
    const unsigned threads = (unsigned)((most + 63) / 64 * 64);
    if (ncol == 5)
        hipLaunchKernelGGL(rig_track_kernel<5>, dim3((unsigned)n_vehicles), dim3(threads), 0, as_stream(stream), *cfg, tcap, ocap_in,
                           obs_in, n_in, views_in, plan_state, (unsigned char*)state, ocap_out, obstacles, n_obs, obs_slot, match, n_skip,
                           n_drop, cls_in, cls_out);
    else
        hipLaunchKernelGGL(rig_track_kernel<3>, dim3((unsigned)n_vehicles), dim3(threads), 0, as_stream(stream), *cfg, tcap, ocap_in,
                           obs_in, n_in, views_in, plan_state, (unsigned char*)state, ocap_out, obstacles, n_obs, obs_slot, match, n_skip,
                           n_drop, cls_in, cls_out);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_rig_track(av_ctx* ctx, av_stream_t stream, const av_rig_track_cfg* cfg, int n_vehicles, int tcap, int ncol, int ocap_in,
                 const double* obs_in, const int32_t* n_in, const int32_t* views_in, const double* plan_state, void* state,
                 int ocap_out, double* obstacles, int32_t* n_obs, int32_t* obs_slot, int32_t* match, int32_t* n_skip,
                 int32_t* n_drop) {
    return rig_track("av_rig_track", ctx, stream, cfg, n_vehicles, tcap, ncol, ocap_in, obs_in, n_in, views_in, plan_state, state,
                     ocap_out, obstacles, n_obs, obs_slot, match, n_skip, n_drop, nullptr, nullptr);
}

int av_rig_track_cls(av_ctx* ctx, av_stream_t stream, const av_rig_track_cfg* cfg, int n_vehicles, int tcap, int ncol, int ocap_in,
                     const double* obs_in, const int32_t* n_in, const int32_t* views_in, const int32_t* cls_in,
                     const double* plan_state, void* state, int ocap_out, double* obstacles, int32_t* n_obs, int32_t* obs_slot,
                     int32_t* match, int32_t* n_skip, int32_t* n_drop, int32_t* cls_out) {
    return rig_track("av_rig_track_cls", ctx, stream, cfg, n_vehicles, tcap, ncol, ocap_in, obs_in, n_in, views_in, plan_state, state,
                     ocap_out, obstacles, n_obs, obs_slot, match, n_skip, n_drop, cls_in, cls_out);
}

}  // extern "C"
