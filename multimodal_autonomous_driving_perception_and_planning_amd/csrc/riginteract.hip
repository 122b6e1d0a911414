// Interaction tags from the vehicle-frame tracks (av_rig_interact): the rig's counterpart of interaction.hip.
//
// The reference's InteractionDetector (interaction_detector.py:132-222) guesses a distance from a box height and "in front" from the
// image centre.  Behind av_rig_track a rig holds the quantities themselves: a metric position and a filtered velocity on the road,
// an id that survives camera hand-overs, and objects beside and behind the vehicle.  This kernel applies the reference's rule table
// and thresholds (:117-125) to them, and adds the rules a forward camera can never fire (being_followed, vehicle_cut_out, passing,
// being_passed).  Semantics and operation order: include/avhot.h.
//
// Mapping: one workgroup per vehicle, tcap threads rounded up to whole waves (1 .. 8); thread t owns slot t of the tracker's state
// (read only) and slot t of this stage's own state, the ring of the slot's last 30 lateral offsets, of which it touches two entries
// per frame in global memory.  The per-track rules are element-wise.  The summary is ballots and DPP wave reductions (common.h) per
// wave, posted to LDS and folded over the waves by thread 0.  float64, -ffp-contract=off: every operation rounded on its own.
#include "common.h"

#include <cmath>

static_assert(sizeof(av_rig_interact_cfg) == 112, "av_rig_interact_cfg is 5 doubles and 18 int32 (include/avhot.h)");

namespace {

constexpr int MAX_T = 512, MAX_WAVES = 8, RING = 30;
constexpr int TRACK_HDR_BYTES = 64, TRACK_SLOT_BYTES = 96;      // av_rig_track's state (rigtrack.hip)
constexpr int HDR_BYTES = 16, SLOT_BYTES = 8 + RING * 8;        // int64 frames, 8 bytes of 0; per slot int32 id, cnt; double lat[30]
static_assert(SLOT_BYTES == 248, "the slot of av_rig_interact's state");

__host__ __device__ inline size_t state_bytes(int tcap) { return (size_t)HDR_BYTES + (size_t)tcap * SLOT_BYTES; }
__host__ __device__ inline size_t track_bytes(int tcap) { return (size_t)TRACK_HDR_BYTES + (size_t)tcap * TRACK_SLOT_BYTES; }

struct Shared {
    int32_t n_on[MAX_WAVES], n_ped[MAX_WAVES], n_cyc[MAX_WAVES], n_veh[MAX_WAVES], n_int[MAX_WAVES];
    int32_t risk1[MAX_WAVES], slot[MAX_WAVES], type[MAX_WAVES];  // the wave's primary: risk + 1 (0: none), its slot and type
    double conf[MAX_WAVES], min_d[MAX_WAVES], min_ttc[MAX_WAVES];
};

__global__ void __launch_bounds__(MAX_T) rig_interact_kernel(av_rig_interact_cfg cfg, int tcap, const unsigned char* __restrict__ track,
                                                            const double* __restrict__ plan_state, unsigned char* __restrict__ state,
                                                            av_interaction_row* __restrict__ rows,
                                                            av_interaction_summary* __restrict__ summary) {
    __shared__ Shared sh;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, nw = (int)blockDim.x >> 6;
    const size_t v = blockIdx.x;
    const bool own = tid < tcap;                                             // this thread owns slot tid
    const double x0 = plan_state[v * 4], y0 = plan_state[v * 4 + 1], h = plan_state[v * 4 + 2], v0 = plan_state[v * 4 + 3];
    unsigned char* const st = state + v * state_bytes(tcap);
    // ---- slot tid of the tracker (only dereferenced when own) ----
    int id = -1, hits = 0, cls1 = 0;
    double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0;
    if (own) {
        const unsigned char* slot = track + v * track_bytes(tcap) + TRACK_HDR_BYTES + (size_t)tid * TRACK_SLOT_BYTES;
        const int4 i0 = *reinterpret_cast<const int4*>(slot);
        const int4 i1 = *reinterpret_cast<const int4*>(slot + 16);
        const double2 d0 = *reinterpret_cast<const double2*>(slot + 32), d1 = *reinterpret_cast<const double2*>(slot + 48);
        id = i0.x, hits = i0.y, cls1 = i1.z;
        x = d0.x, y = d0.y, vx = d1.x, vy = d1.y;
    }
    const bool on = own && id >= 0 && hits >= cfg.min_hits;                  // a confirmed live track, coasting ones included
    double sn, cs, s2, c2;
    sincos(h, &sn, &cs);
    sincos(h + 1.5707963267948966, &s2, &c2);
    int kind = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) kind = cls1 == k + 1 ? cfg.class_kind[k] : kind;            // (no class, or one outside 0..15: 0)
    // ---- the track relative to the ego ----
    const double ex = x - x0, ey = y - y0;
    const double X = ex * cs + ey * sn, Y = ex * c2 + ey * s2;               // forward, lateral
    const double rvx = vx - v0 * cs, rvy = vy - v0 * sn;
    const double RVX = rvx * cs + rvy * sn;
    const double d = sqrt(ex * ex + ey * ey);
    const double closing = d > 0.0 ? -((ex * rvx + ey * rvy) / d) : 0.0;     // > 0 when the range shrinks
    const bool has_ttc = closing > 0.1;
    const double ttc = has_ttc ? d / closing : 0.0;
    // ---- the ring of lateral offsets: append, then the oldest of the last min(cnt, 30) entries ----
    int hl = 0;
    double Y0 = Y;
    if (on) {
        int32_t* const hd = reinterpret_cast<int32_t*>(st + HDR_BYTES + (size_t)tid * SLOT_BYTES);
        double* const ring = reinterpret_cast<double*>(hd + 2);
        const int2 ic = *reinterpret_cast<const int2*>(hd);
        const int c = ic.x == id ? ic.y : 0;                                 // another id in the slot: the ring restarts
        const int c1 = c + 1;
        if (c > 0) Y0 = c1 <= RING ? ring[0] : ring[c1 % RING];              // (never the entry written below)
        ring[c % RING] = Y;
        *reinterpret_cast<int2*>(hd) = make_int2(id, c1);
        hl = c1 < RING ? c1 : RING;
    }
    const double aY = fabs(Y);
    const bool ahead = X > 0.0, in_path = aY < cfg.corridor_half, beside = !in_path && aY < cfg.adjacent_half;
    // ---- the rules, the first hit wins ----
    const double none = __builtin_nan("");
    int type = -1, risk = 0;
    double conf = 0.0, o_rel = closing, o_ttc = has_ttc ? ttc : none;
    if (on) {
        if (d < 3.0) {
            type = 9, conf = 0.9, risk = 3;
        } else if (kind == 1 && d < 10.0) {
            if (ahead && in_path) type = 6, conf = 0.8, risk = d < 8.0 ? 2 : 1;
            else type = 7, conf = 0.6, risk = 0, o_rel = 0.0, o_ttc = none;
        } else if (kind == 2 && d < 15.0) {
            type = 8, conf = 0.7, risk = d < 8.0 ? 1 : 0, o_ttc = none;
        } else if (kind == 3) {
            const bool was_in = fabs(Y0) < cfg.corridor_half;
            const bool turn = hl >= 10 && d < 15.0 && ahead;
            const bool follow = in_path && d > 5.0 && d < 30.0;
            const bool along = beside && fabs(X) < cfg.alongside;
            if (turn && in_path && !was_in) {
                type = 4, conf = 0.7, risk = 1;
            } else if (turn && !in_path && was_in) {
                type = 5, conf = 0.7, risk = 0;
            } else if (follow && ahead) {
                type = 1, conf = 0.75, risk = d < 10.0 ? 1 : 0;
                if (has_ttc && ttc < 3.0) risk = 2;
            } else if (follow) {
                type = 2, conf = 0.75, risk = 0;
                if (has_ttc && ttc < 3.0) risk = 2;
            } else if (along && RVX < -cfg.pass_speed) {
                type = 11, conf = 0.7, risk = 0;
            } else if (along && RVX > cfg.pass_speed) {
                type = 12, conf = 0.7, risk = 0;
            }
        }
    }
    if (own) {
        av_interaction_row o;
        o.type = type, o.risk = risk, o.agent_id = on ? id : -1, o.cls = on ? cls1 - 1 : -1;
        o.confidence = conf, o.distance = on ? d : 0.0, o.relative_speed = type >= 0 ? o_rel : 0.0;
        o.ttc = type >= 0 ? o_ttc : none;
        rows[v * (size_t)tcap + (size_t)tid] = o;
    }
    // ---- the summary: per wave, then over the waves ----
    const double inf = __builtin_inf();
    {
        const int n_on = __popcll(__ballot(on)), n_ped = __popcll(__ballot(on && kind == 1));
        const int n_cyc = __popcll(__ballot(on && kind == 2)), n_veh = __popcll(__ballot(on && (kind == 3 || kind == 4)));
        const bool is_int = type >= 0;
        const int n_int = __popcll(__ballot(is_int));
        const double min_d = -wave_max(on ? -d : -inf);
        const double min_ttc = -wave_max(on && has_ttc ? -ttc : -inf);
        // the wave's primary: the largest risk, then the largest confidence, then the smallest slot
        const unsigned r1 = wave_max_u32(is_int ? (unsigned)risk + 1u : 0u);
        const bool top = is_int && (unsigned)risk + 1u == r1;
        const double bc = wave_max(top ? conf : -1.0);
        const unsigned long long pm = __ballot(top && conf == bc);
        const int pl = pm ? __ffsll((long long)pm) - 1 : 0;
        const int ptype = __shfl(type, pl, 64);
        if (lane == 0) {
            sh.n_on[w] = n_on, sh.n_ped[w] = n_ped, sh.n_cyc[w] = n_cyc, sh.n_veh[w] = n_veh, sh.n_int[w] = n_int;
            sh.min_d[w] = min_d, sh.min_ttc[w] = min_ttc;
            sh.risk1[w] = (int)r1, sh.conf[w] = bc, sh.slot[w] = w * 64 + pl, sh.type[w] = ptype;
        }
    }
    __syncthreads();
    if (tid == 0) {
        long long* const frames = reinterpret_cast<long long*>(st);
        const long long f = frames[0];
        av_interaction_summary q;
        q.agent_count = q.pedestrian_count = q.cyclist_count = q.vehicle_count = q.n_interactions = 0;
        int best_r1 = 0, best_slot = -1, best_type = -1;
        double best_c = -1.0, min_d = inf, min_ttc = inf;
        for (int k = 0; k < nw; ++k) {                                       // (in wave order: the smaller slot stays among equals)
            q.agent_count += sh.n_on[k], q.pedestrian_count += sh.n_ped[k], q.cyclist_count += sh.n_cyc[k];
            q.vehicle_count += sh.n_veh[k], q.n_interactions += sh.n_int[k];
            min_d = fmin(min_d, sh.min_d[k]), min_ttc = fmin(min_ttc, sh.min_ttc[k]);
            const int r1 = sh.risk1[k];
            const double c = sh.conf[k];
            if (r1 > best_r1 || (r1 == best_r1 && r1 > 0 && c > best_c)) best_r1 = r1, best_c = c, best_slot = sh.slot[k], best_type = sh.type[k];
        }
        q.closest_distance = min_d;
        q.min_ttc = min_ttc == inf ? none : min_ttc;
        q.primary_type = best_type, q.primary_row = best_slot;
        q.overall_risk = best_r1 > 0 ? (min_ttc < 1.5 ? 3 : best_r1 - 1) : 0;
        q.timestamp = (double)f * cfg.dt;
        summary[v] = q;
        frames[0] = f + 1;
    }
}

__global__ void __launch_bounds__(256) rig_interact_reset_kernel(size_t n_words, int words_per_vehicle, int2* __restrict__ state) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;                 // one 8-byte word each
    if (i >= n_words) return;
    const int wd = (int)(i % (size_t)words_per_vehicle);
    const bool id_word = wd >= HDR_BYTES / 8 && (wd - HDR_BYTES / 8) % (SLOT_BYTES / 8) == 0;
    state[i] = make_int2(id_word ? -1 : 0, 0);                               // (id, cnt)
}

bool tcap_ok(int tcap) { return tcap >= 1 && tcap <= MAX_T; }

}  // namespace

extern "C" {

size_t av_rig_interact_state_bytes(int tcap) { return tcap_ok(tcap) ? state_bytes(tcap) : 0; }

int av_rig_interact_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int tcap, void* state) {
    AV_REQUIRE(n_vehicles >= 1, AV_EINVAL, "av_rig_interact_reset: n_vehicles must be >= 1");
    AV_REQUIRE(tcap_ok(tcap), AV_EINVAL, "av_rig_interact_reset: tcap %d not in 1..%d", tcap, MAX_T);
    AV_REQUIRE(ctx && state, AV_EINVAL, "av_rig_interact_reset: null argument");
    const int per = (int)(state_bytes(tcap) / 8);
    const size_t n_words = (size_t)n_vehicles * per;
    hipLaunchKernelGGL(rig_interact_reset_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, as_stream(stream), n_words, per,
                       (int2*)state);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_rig_interact(av_ctx* ctx, av_stream_t stream, const av_rig_interact_cfg* cfg, int n_vehicles, int tcap, const void* track_state,
                    const double* plan_state, void* state, av_interaction_row* rows, av_interaction_summary* summary) {
    AV_REQUIRE(n_vehicles >= 1, AV_EINVAL, "av_rig_interact: n_vehicles must be >= 1");
    AV_REQUIRE(tcap_ok(tcap), AV_EINVAL, "av_rig_interact: tcap %d not in 1..%d", tcap, MAX_T);
    AV_REQUIRE(cfg, AV_EINVAL, "av_rig_interact: null cfg");
    static const char* const names[5] = {"dt", "corridor_half", "adjacent_half", "alongside", "pass_speed"};
    const double* d = &cfg->dt;
    for (int i = 0; i < 5; ++i)
        AV_REQUIRE(std::isfinite(d[i]) && d[i] > 0.0, AV_EINVAL, "av_rig_interact: cfg %s must be finite and > 0", names[i]);
    AV_REQUIRE(cfg->min_hits >= 1, AV_EINVAL, "av_rig_interact: cfg min_hits must be >= 1");
    AV_REQUIRE(ctx && track_state && plan_state && state && rows && summary, AV_EINVAL, "av_rig_interact: null argument");
    const unsigned threads = (unsigned)((tcap + 63) / 64 * 64);
    hipLaunchKernelGGL(rig_interact_kernel, dim3((unsigned)n_vehicles), dim3(threads), 0, as_stream(stream), *cfg, tcap,
                       (const unsigned char*)track_state, plan_state, (unsigned char*)state, rows, summary);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"
