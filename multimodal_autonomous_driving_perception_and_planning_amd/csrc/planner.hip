// P1-P3: batched candidate-trajectory planner.
//
// Reference: MotionPlanner (src/planning/motion_planner.py)
//   generate_polynomial_trajectory :126-204, evaluate_trajectory_cost :206-262, plan :264-303.
//
// Data layout (HBM):  waypoints [n_states][C][n][6] float64, AoS per waypoint
//   (x, y, heading, velocity, timestamp, curvature) -- the field order of the Waypoint dataclass --
//   so one trajectory is one contiguous n*48-byte run; cost/order [n_states][C].
//
// Mapping: a 256-thread workgroup owns G consecutive start states.
//   phase 1  3*G lanes run the sequential part the reference has per speed option: the velocity
//            blend, the prefix sum s_i = s_{i-1} + v_i*dt (:156-157) and the velocity/acceleration
//            cost accumulated left to right (:235-244).  These depend only on (v0, vt) and are
//            shared by the num_samples lateral offsets.  G more lanes take cos/sin of the heading.
//   phase 2  each wave takes whole trajectories; lane = waypoint.  Positions, tangent heading
//            (atan2 of the forward difference), curvature and the per-waypoint cost terms are
//            computed in registers, the AoS image of the trajectory is assembled in a per-wave LDS
//            tile, and the tile is streamed out as contiguous 16-byte-per-lane stores (the kernel's
//            HBM traffic is these stores: 48 B per waypoint).
//   phase 3  stable rank of the C costs (== Python's stable sort, :300).
// All arithmetic is float64 in the reference's operation order; the library is built with
// -ffp-contract=off so a*b+c stays two roundings like NumPy scalar code.
// This file: the four kernels, the instantiation tables, the launch plan and the entry points.  What the kernels are made of -- the
// reference's arithmetic, the list types, plan_block (phases 1-3 above) -- is in planner_dev.h.
#include "planner_dev.h"

namespace {

template <int G, int NW, class Lists = PlanShared>
__global__ void __launch_bounds__(NW * 64) planner_kernel(PlanParams p, int n_states, const double* __restrict__ state, Lists lists,
                                                          double* __restrict__ wp, double* __restrict__ cost,
                                                          int32_t* __restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    plan_block_lists<G, NW, PlanNoHook, Lists>(p, blockIdx.x * G, n_states, state, lists, wp, cost, order, sm);
}

// Throughput variant for large batches and n <= 64: every wave is autonomous (no workgroup barrier).
// A wave owns FPW consecutive start states; lane = waypoint index, so the per-waypoint constants
// (1-exp(-t_i), quintic blend, timestamp) sit in registers for the whole kernel.
//   1a  all lanes: velocity profile + acceleration cost terms of the 3*FPW (state, speed) pairs
//   1b  3*FPW lanes: the reference's sequential sums (prefix s_i, velocity cost, acceleration cost)
//   2   for each of the FPW*C trajectories: positions, heading, curvature, cost, AoS tile -> HBM
//   3   stable rank of each state's C costs
template <int FPW, bool EXTRA, class Lists = PlanShared>     // EXTRA: a reference path and/or obstacles take part in the cost
__global__ void __launch_bounds__(256) planner_wave_kernel(PlanParams p, int n_states,
                                                           const double* __restrict__ state, Lists lists,
                                                           double* __restrict__ wp, double* __restrict__ cost,
                                                           int32_t* __restrict__ order) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = p.n, C = p.C;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double* vs = sm + wid * wave_lds_doubles(FPW, n, C);                 // [FPW*3][n][2]  (v, s)
    double* stage = vs + (size_t)FPW * 3 * n * 2;      // output ring (256 x 16 B); phase 1: acc terms [FPW*3][n]
    double* costs = stage + RING_DOUBLES;              // [FPW][C]
    double* base = costs + even_up(FPW * C);           // [FPW*3][4]  S_v, S_a, running
    double* trig = base + FPW * 3 * 4;                 // [FPW][8]
    const long long gw = (long long)blockIdx.x * 4 + wid;
    const long long f0l = gw * FPW;
    if (f0l >= n_states) return;
    const int f0 = (int)f0l;
    const int nf = (n_states - f0) < FPW ? (n_states - f0) : FPW;    // states this wave really has

    // All global reads of this wave happen here, in one batch: per-lane table entries (lane = waypoint
    // index), the lateral offsets (lane = sample index) and the wave's start states.  Nothing below
    // reads memory again, so the loops never queue behind the store traffic.
    const bool in = lane < n;
    const int li_c = in ? lane : n - 1;                 // clamped waypoint index of this lane
    const int ln_c = (lane + 1 < n) ? lane + 1 : n - 1; // clamped index of the next waypoint
    const int lp_c = li_c > 0 ? li_c - 1 : 0;
    const double q_i = p.q[li_c], q_n = p.q[ln_c], t_i = p.t[li_c];
    const double al_i = p.alpha[li_c], al_p = p.alpha[lp_c], dtd_i = p.dtd[li_c];
    const double lat_l = p.lat[lane < p.n_lat ? lane : 0];
    double st_x[FPW], st_y[FPW], st_h[FPW], st_v[FPW];
#pragma unroll
    for (int g = 0; g < FPW; ++g) {
        const double4 sv4 = reinterpret_cast<const double4*>(state)[f0 + (g < nf ? g : 0)];
        st_x[g] = sv4.x, st_y[g] = sv4.y, st_h[g] = sv4.z, st_v[g] = sv4.w;
    }

    // ---- 1a: lane = waypoint; velocity profile and acceleration cost term of every (state, speed) -----
#pragma unroll
    for (int g = 0; g < FPW; ++g) {
        if (g < nf) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int pair = g * 3 + k;
                const double v0 = st_v[g];
                const double dv = target_speed(k) - v0;
                const double v = blend_velocity(v0, dv, al_i);
                const double acc = (lane > 0 && dtd_i > 0.0) ? acceleration_term(p.w_acc, v, blend_velocity(v0, dv, al_p), dtd_i) : 0.0;
                if (in) {
                    vs[((size_t)pair * n + lane) * 2] = v;
                    stage[(size_t)pair * n + lane] = acc;
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < FPW; ++g) {
        if (g < nf && lane == 32 + g) {
            const double h0 = st_h[g];
            const double hp = h0 + 1.5707963267948966;
            double* tg = trig + g * 8;
            tg[0] = st_x[g], tg[1] = st_y[g];
            tg[2] = cos(h0), tg[3] = sin(h0), tg[4] = cos(hp), tg[5] = sin(hp), tg[6] = h0;
        }
    }
    wave_lds_fence();
    // ---- 1b: 3*nf lanes run the reference's sequential sums over LDS-resident terms -----------------
    if (lane < nf * 3) {
        double* o = vs + (size_t)lane * n * 2;
        const double* ac = stage + (size_t)lane * n;
        double s = 0.0, sv = 0.0;
        for (int i = 0; i < n; ++i) {
            const double v = o[2 * i];
            if (i > 0) s = s + v * p.dt;                               // :157
            o[2 * i + 1] = s;
            sv = sv + velocity_term(p.w_vel, v);
        }
        double run = sv, sa = 0.0;
        for (int i = 1; i < n; ++i) {                                  // zero terms stand for skipped ones
            const double term = ac[i];
            run = run + term, sa = sa + term;
        }
        double* b = base + lane * 4;
        b[0] = sv, b[1] = sa, b[2] = run;
    }
    wave_lds_fence();

    // ---- 2 -----------------------------------------------------------------------------------------
    // Lanes >= n run the same arithmetic on a clamped index (no predication inside the loop); their
    // results are dropped at the sum and at the store.
    // Output stream.  The wave's trajectories are contiguous in HBM (memory order), 3n 16-byte units each.
    // Tiles are appended to an LDS ring in stream order and leave as FULL 1-KB wave stores aligned in
    // absolute address (only the very first and last store of the wave are partial): a 2448-B tile written
    // as 64+64+25 lanes straddles cache lines at both ends and reaches 5.3 TB/s store-only, aligned full
    // stores 6.0 (tools/wpattern.hip, tools/wfill.hip).  Software pipeline: the chunks completed by tile
    // c-1 are read from the ring at the top of iteration c and stored after its arithmetic.
    const int n3 = n * 3;                                   // units per trajectory (153 for n = 51)
    const size_t G0 = (size_t)(reinterpret_cast<uintptr_t>(wp) >> 4) + (size_t)f0 * C * n3;   // unit address of the stream
    const int A = (int)(G0 & 63);                           // stream unit u sits at virtual unit v = u + A
    double2* const gch = reinterpret_cast<double2*>((G0 - (size_t)A) << 4);                   // virtual unit 0
    double2* const ring = reinterpret_cast<double2*>(stage);
    int ti = 0, jdone = 0;                                  // tiles staged, chunks stored
    double2 r0 = make_double2(0.0, 0.0), r1 = r0, r2 = r0;
    for (int g = 0; g < nf; ++g) {
        const int f = f0 + g;
        const double* tg = trig + g * 8;
        const PlanFrame fr{tg[0], tg[1], tg[2], tg[3], tg[4], tg[5]};
        const double h0 = tg[6];
        const PlanLists ls = lists.at(f);                            // this state's reference path and obstacles
        const double* ref = ls.ref;
        const double* obs = ls.obs;
        const int n_ref = ls.n_ref, n_obs = ls.n_obs;
        // per speed k: everything the 7 lateral samples share, kept in registers so that the trajectories can
        // be produced in memory order c = li*3 + k (a wave then writes its 51 KB sequentially; the speed-outer
        // order hops 7344 B between tiles and costs a quarter of the write rate -- tools/wpattern.hip)
        double kv[3], kbx[3], kby[3], kbx1[3], kby1[3], kden[3], krden[3], kb0[3], kb1[3], kb2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double* o = vs + ((size_t)(g * 3 + k) * n) * 2;
            const double v = o[2 * li_c], s = o[2 * li_c + 1], s1 = o[2 * ln_c + 1];
            kv[k] = v;
            fr.along(s, kbx[k], kby[k]);
            fr.along(s1, kbx1[k], kby1[k]);
            kden[k] = v * p.dt + 1e-6;                               // :196 denominator
            krden[k] = 1.0 / kden[k];                                // shared by the n_lat trajectories of this speed
            const double* b = base + (g * 3 + k) * 4;
            kb0[k] = b[0], kb1[k] = b[1], kb2[k] = b[2];
        }
        for (int li = 0; li < p.n_lat; ++li) {
            const double df = readlane_f64(lat_l, li);
            double dxc, dyc, dxc1, dyc1;
            fr.across(df * q_i, dxc, dyc);
            fr.across(df * q_n, dxc1, dyc1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int c = li * 3 + k;
                const double v = kv[k], bx = kbx[k], by = kby[k], bx1 = kbx1[k], by1 = kby1[k];
                const double den = kden[k], rden = krden[k], b0 = kb0[k], b1 = kb1[k], b2 = kb2[k];
                const int jend = (A + ti * n3) >> 6;       // chunks complete once tiles < ti are staged
                const int np = wp ? jend - jdone : 0;        // 0 (first tile) .. 3
                if (np > 0) {            // issue the LDS reads early; consumed after the math
                    wave_lds_fence();
                    const int u0 = jdone * 64 + lane;
                    r0 = ring[u0 & (RING_UNITS - 1)];
                    if (np > 1) r1 = ring[(u0 + 64) & (RING_UNITS - 1)];
                    if (np > 2) r2 = ring[(u0 + 128) & (RING_UNITS - 1)];
                    wave_lds_fence();
                }
                const double x = bx + dxc, y = by + dyc;             // (PlanFrame::point, its two halves made above)
                const double x1 = bx1 + dxc1, y1 = by1 + dyc1;
                double hd = atan2_fast(y1 - y, x1 - x, p.atq);       // :188
                const double hprev = dpp_mov_f64<0x138>(hd);         // lane i <- lane i-1
                // (hd - hprev) / den, correctly rounded from the correctly rounded reciprocal (Markstein):
                // q0 = a*r, q = q0 + (a - q0*den)*r
                const double dh = hd - hprev;
                const double cq = dh * rden;
                double curv = __builtin_fma(__builtin_fma(-cq, den, dh), rden, cq);
                curv = (lane > 0 && lane < n - 1) ? curv : 0.0;
                if (lane == n - 1) hd = n > 1 ? hprev : h0;          // :190
                double lat_sum = 0.0, obs_sum = 0.0;
                if (EXTRA && n_ref > 0) {
                    const double term = ref_path_term(p.w_lat, ref, n_ref, x, y);
                    lat_sum = wave_sum_dpp(in ? term : 0.0);
                }
                if (EXTRA && n_obs > 0) {
                    for (int q = 0; q < n_obs; ++q)
                        add_obstacle_penalty<Lists::MOVING>(obs_sum, obs + Lists::OSTRIDE * q, x, y, t_i);
                    obs_sum = wave_sum_dpp(in ? obs_sum : 0.0);
                }
                const double curv_sum = wave_sum_dpp(in ? p.w_curv * (curv * curv) : 0.0);
                if (lane == 0) {
                    const double va = (EXTRA && n_ref > 0) ? (lat_sum + b0) + b1 : b2;
                    costs[g * C + c] = EXTRA ? (va + curv_sum) + obs_sum : va + curv_sum;
                }
                if (wp) {
                    // stream out the chunks read at the top of this iteration, then append this tile
                    if (np > 0) {
                        const int v0 = jdone * 64 + lane;
                        if (v0 >= A) gch[v0] = r0;                       // only chunk 0 has units before the stream
                        if (np > 1) gch[v0 + 64] = r1;
                        if (np > 2) gch[v0 + 128] = r2;
                        jdone = jend;
                    }
                    if (in) {
                        const int u = A + ti * n3 + lane * 3;
                        ring[u & (RING_UNITS - 1)] = make_double2(x, y);
                        ring[(u + 1) & (RING_UNITS - 1)] = make_double2(hd, v);
                        ring[(u + 2) & (RING_UNITS - 1)] = make_double2(t_i, curv);
                    }
                    ++ti;
                }
            }
        }
    }
    if (wp) {                 // drain: remaining full chunks and the partial tail
        wave_lds_fence();
        const int vend = A + ti * n3;
        for (int j = jdone; j * 64 < vend; ++j) {
            const int v = j * 64 + lane;
            if (v >= A && v < vend) gch[v] = ring[v & (RING_UNITS - 1)];
        }
    }
    wave_lds_fence();
    // ---- 3 -----------------------------------------------------------------------------------------
    for (int idx = lane; idx < nf * C; idx += 64) {
        const int g = idx / C, c = idx - g * C;
        rank_and_store(costs + g * C, C, c, f0 + g, cost, order);
    }
}

// generate_polynomial_trajectory for one arbitrary (df, vt): one wave per trajectory.
__global__ void __launch_bounds__(64) planner_generate_kernel(PlanParams p, int n_traj, const double* __restrict__ state,
                                                              const double* __restrict__ dfs,
                                                              const double* __restrict__ vts, double* __restrict__ wp) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int n = p.n, lane = threadIdx.x, j = blockIdx.x;
    if (j >= n_traj) return;
    double* vs = sm;                 // [n][2]
    double* stage = sm + 2 * n;      // [n][6]
    const double x0 = state[4 * j], y0 = state[4 * j + 1], h0 = state[4 * j + 2], v0 = state[4 * j + 3];
    const double df = dfs[j], vt = vts[j];
    if (lane == 0) {
        const double dv = vt - v0;
        double s = 0.0;
        for (int i = 0; i < n; ++i) {
            const double v = blend_velocity(v0, dv, p.alpha[i]);
            if (i > 0) s = s + v * p.dt;
            vs[2 * i] = v, vs[2 * i + 1] = s;
        }
    }
    wave_lds_fence();
    const double hp2 = h0 + 1.5707963267948966;
    const PlanFrame fr{x0, y0, cos(h0), sin(h0), cos(hp2), sin(hp2)};
    for (int i = lane; i < n; i += 64) {
        const double v = vs[2 * i], s = vs[2 * i + 1];
        double x, y, hd = 0.0;
        fr.point(s, df * p.q[i], x, y);
        if (i < n - 1) {
            double x1, y1;
            fr.point(vs[2 * i + 3], df * p.q[i + 1], x1, y1);
            hd = atan2(y1 - y, x1 - x);                         // (libm's here, atan2_fast in the plan kernels)
        }
        double* w = stage + (size_t)i * 6;
        w[0] = x, w[1] = y, w[2] = hd, w[3] = v, w[4] = p.t[i], w[5] = 0.0;
    }
    wave_lds_fence();
    for (int i = lane; i < n; i += 64)
        if (i > 0 && i < n - 1) stage[(size_t)i * 6 + 5] = tile_curvature(stage, i, p.dt);
    wave_lds_fence();
    if (lane == 0) tile_last_heading(stage, n, h0);
    wave_lds_fence();
    double* dst = wp + (size_t)j * n * 6;
    for (int q = lane; q < n * 6; q += 64) dst[q] = stage[q];
}

// evaluate_trajectory_cost for an arbitrary trajectory, strictly in the reference's accumulation order
// (one thread per trajectory; this is a utility entry, the hot path is planner_kernel).
template <bool MOVING>      // MOVING: obstacle rows (x, y, radius, vx, vy), each at its place for the waypoint's own timestamp (field 4)
__global__ void planner_evaluate_kernel(PlanParams p, int n_traj, int n_wp, const double* __restrict__ wp,
                                        const double* __restrict__ ref, int n_ref, const double* __restrict__ obs,
                                        int n_obs, double* __restrict__ cost) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_traj) return;
    if (n_wp == 0) {
        cost[j] = INFINITY;
        return;
    }
    const double* w = wp + (size_t)j * n_wp * 6;
    double c = 0.0;
    if (n_ref > 0)
        for (int i = 0; i < n_wp; ++i) c = c + ref_path_term(p.w_lat, ref, n_ref, w[6 * i], w[6 * i + 1]);
    for (int i = 0; i < n_wp; ++i) c = c + velocity_term(p.w_vel, w[6 * i + 3]);
    for (int i = 1; i < n_wp; ++i) {
        const double dtt = w[6 * i + 4] - w[6 * (i - 1) + 4];
        if (dtt > 0.0) c = c + acceleration_term(p.w_acc, w[6 * i + 3], w[6 * (i - 1) + 3], dtt);
    }
    for (int i = 0; i < n_wp; ++i) c = c + p.w_curv * (w[6 * i + 5] * w[6 * i + 5]);
    for (int q = 0; q < n_obs; ++q)                     // obstacle outer, every term straight into the running cost: the reference's order
        for (int i = 0; i < n_wp; ++i) add_obstacle_penalty<MOVING>(c, obs + (MOVING ? 5 : 3) * q, w[6 * i], w[6 * i + 1], w[6 * i + 4]);
    cost[j] = c;
}

}  // namespace

// Every instantiation of the two plan kernels there is, per list type.  planner_plan finds its kernel here and nowhere else.
// wave: planner_wave_kernel<G, extra> (G start states per wave, four waves); else planner_kernel<G, NW>.
template <class Lists>
struct PlanInst {
    bool wave, extra;
    int G, NW;
    void (*fn)(PlanParams, int, const double*, Lists, double*, double*, int32_t*);
};
template <class Lists>
const PlanInst<Lists> plan_insts[] = {
    {false, false, 1, 8, planner_kernel<1, 8, Lists>}, {false, false, 1, 4, planner_kernel<1, 4, Lists>},
    {false, false, 1, 2, planner_kernel<1, 2, Lists>}, {false, false, 2, 4, planner_kernel<2, 4, Lists>},
    {false, false, 4, 4, planner_kernel<4, 4, Lists>}, {false, false, 8, 4, planner_kernel<8, 4, Lists>},
    {true, false, 2, 4, planner_wave_kernel<2, false, Lists>}, {true, true, 2, 4, planner_wave_kernel<2, true, Lists>},
};

// Everything a launch of av_planner_plan, av_planner_plan_each and av_planner_plan_moving is decided by, decided in one place.
template <class Lists>
struct PlanLaunch {
    const PlanInst<Lists>* inst;
    unsigned grid, block;
    size_t lds;                        // dynamic LDS bytes
};
// `extra`: a reference path and / or obstacles may take part in the cost (the wave kernel's EXTRA form).  The shape does not depend on
// the list type.
template <class Lists>
static PlanLaunch<Lists> planner_plan(int n, int C, int n_states, bool extra) {
    const bool wave = n <= 64 && n_states >= 1024;
    int G, NW = 4;
    size_t lds;
    if (wave) {
        // two states per wave (103-KB output regions); one per wave -- 51-KB regions, twice the waves -- measured the same
        // (59.4-60.7 % of HBM peak at 16 384 states either way, alternating runs on one box)
        G = 2;
        lds = wave_lds_doubles(G, n, C) * NW * sizeof(double);
    } else {
        extra = false;                 // (the workgroup kernel has one form)
        G = n_states >= 4096 ? 8 : (n_states >= 1024 ? 4 : (n_states >= 512 ? 2 : 1));
        while (G > 1 && plan_lds_doubles(G, n, C, 4) * 8 > 48 * 1024) G >>= 1;
        // one state per workgroup: its 3 C trajectories over eight waves, or four / two where eight per-wave tiles do not fit
        // (two fit every configuration av_planner_configure accepts: n = 256, C = 192 needs 41.6 KB)
        if (G == 1) NW = 8;
        while (G == 1 && NW > 2 && plan_lds_doubles(1, n, C, NW) * 8 > 64 * 1024) NW >>= 1;
        lds = plan_lds_doubles(G, n, C, NW) * 8;
    }
    const int per_group = wave ? G * NW : G;          // start states of a workgroup
    PlanLaunch<Lists> p{nullptr, (unsigned)((n_states + per_group - 1) / per_group), (unsigned)NW * 64, lds};
    for (const PlanInst<Lists>& k : plan_insts<Lists>)
        if (k.wave == wave && k.extra == extra && k.G == G && k.NW == NW) p.inst = &k;
    return p;
}

template <class Lists>
static int plan_dispatch(av_ctx* ctx, hipStream_t st, int n_states, const double* state, const Lists& lists, bool extra,
                         double* waypoints, double* cost, int32_t* order, const char* who) {
    const PlanLaunch<Lists> l = planner_plan<Lists>(ctx->n_points, ctx->n_cand, n_states, extra);
    AV_REQUIRE(l.lds <= 64 * 1024, AV_EINVAL, "%s: configuration needs %zu B of LDS", who, l.lds);
    PlanParams p;
    fill_params(ctx, p);
    hipLaunchKernelGGL(l.inst->fn, dim3(l.grid), dim3(l.block), l.lds, st, p, n_states, state, lists, waypoints, cost, order);
    AV_LAUNCH_CHECK();
    return AV_OK;
}


extern "C" {

int av_planner_generate(av_ctx* ctx, av_stream_t stream, int n_traj, const double* state,
                        const double* end_lateral_offset, const double* target_velocity, double* waypoints) {
    AV_REQUIRE(ctx && state && end_lateral_offset && target_velocity && waypoints, AV_EINVAL,
               "av_planner_generate: null argument");
    AV_REQUIRE(ctx->planner_ready, AV_ESTATE, "av_planner_generate: call av_planner_configure first");
    AV_REQUIRE(n_traj > 0, AV_EINVAL, "av_planner_generate: n_traj must be > 0");
    PlanParams p;
    fill_params(ctx, p);
    hipLaunchKernelGGL(planner_generate_kernel, dim3(n_traj), dim3(64), (size_t)p.n * 8 * 8, as_stream(stream), p,
                       n_traj, state, end_lateral_offset, target_velocity, waypoints);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"

// av_planner_evaluate and av_planner_evaluate_moving: the same checks and launch, the obstacle rows 3 or 5 doubles wide
template <bool MOVING>
static int evaluate_launch(av_ctx* ctx, av_stream_t stream, int n_traj, int n_wp, const double* waypoints, const double* ref_path,
                           int n_ref, const double* obstacles, int n_obs, double* cost, const char* who) {
    AV_REQUIRE(ctx && cost && (waypoints || n_wp == 0), AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE(ctx->planner_ready, AV_ESTATE, "%s: call av_planner_configure first", who);
    AV_REQUIRE(n_traj > 0 && n_wp >= 0, AV_EINVAL, "%s: bad sizes", who);
    AV_REQUIRE(n_ref >= 0 && n_obs >= 0 && (n_ref == 0 || ref_path) && (n_obs == 0 || obstacles), AV_EINVAL,
               "%s: ref_path/obstacles pointer missing", who);
    PlanParams p;
    fill_params(ctx, p);
    hipLaunchKernelGGL(planner_evaluate_kernel<MOVING>, dim3((n_traj + 63) / 64), dim3(64), 0, as_stream(stream), p, n_traj,
                       n_wp, waypoints, ref_path, n_ref, obstacles, n_obs, cost);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

// av_planner_plan_each and av_planner_plan_moving: the same checks and dispatch, the obstacle rows 3 or 5 doubles wide
template <int OS>
static int plan_each_launch(av_ctx* ctx, av_stream_t stream, int n_states, const double* state, const double* ref_path,
                            const int32_t* n_ref, int rcap, int ref_stride, const double* obstacles, const int32_t* n_obs, int ocap,
                            double* waypoints, double* cost, int32_t* order, const char* who) {
    AV_REQUIRE(ctx && state && cost && order, AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE(ctx->planner_ready, AV_ESTATE, "%s: call av_planner_configure first", who);
    AV_REQUIRE(n_states > 0, AV_EINVAL, "%s: n_states must be > 0", who);
    AV_REQUIRE(!ref_path == !n_ref && !obstacles == !n_obs, AV_EINVAL, "%s: a list and its counts go together", who);
    AV_REQUIRE(ref_stride >= 1, AV_EINVAL, "%s: ref_stride must be >= 1", who);
    AV_REQUIRE((!ref_path || rcap >= 0) && (!obstacles || ocap >= 0), AV_EINVAL, "%s: negative capacity", who);
    return plan_dispatch(ctx, as_stream(stream), n_states, state, PlanEachT<OS>{ref_path, n_ref, obstacles, n_obs, rcap, ref_stride, ocap},
                         ref_path || obstacles, waypoints, cost, order, who);
}

extern "C" {

int av_planner_evaluate(av_ctx* ctx, av_stream_t stream, int n_traj, int n_wp, const double* waypoints,
                        const double* ref_path, int n_ref, const double* obstacles, int n_obs, double* cost) {
    return evaluate_launch<false>(ctx, stream, n_traj, n_wp, waypoints, ref_path, n_ref, obstacles, n_obs, cost, "av_planner_evaluate");
}

int av_planner_evaluate_moving(av_ctx* ctx, av_stream_t stream, int n_traj, int n_wp, const double* waypoints,
                               const double* ref_path, int n_ref, const double* obstacles, int n_obs, double* cost) {
    return evaluate_launch<true>(ctx, stream, n_traj, n_wp, waypoints, ref_path, n_ref, obstacles, n_obs, cost,
                                 "av_planner_evaluate_moving");
}

int av_planner_configure(av_ctx* ctx, const av_planner_cfg* cfg) {
    AV_REQUIRE(ctx && cfg, AV_EINVAL, "av_planner_configure: null argument");
    AV_REQUIRE(cfg->dt > 0.0 && cfg->planning_horizon > 0.0, AV_EINVAL, "av_planner_configure: dt and horizon must be > 0");
    AV_REQUIRE(cfg->num_samples >= 1 && cfg->num_samples <= 64, AV_EINVAL,
               "av_planner_configure: num_samples %d not in [1,64]", cfg->num_samples);
    const double H = cfg->planning_horizon;
    const int n = (int)(H / cfg->dt) + 1;                               // :143
    AV_REQUIRE(n >= 1 && n <= 256, AV_EINVAL, "av_planner_configure: %d waypoints per trajectory not in [1,256]", n);
    const int nl = cfg->num_samples;
    std::vector<double> tab((size_t)4 * n + nl);
    double *t = tab.data(), *alpha = t + n, *q = alpha + n, *dtd = q + n, *lat = dtd + n;
    // numpy.linspace(0, H, n): arange * step + start, last element forced to stop      (:144)
    if (n == 1) {
        t[0] = 0.0;
    } else {
        const double step = (H - 0.0) / (double)(n - 1);
        for (int i = 0; i < n; ++i) t[i] = (step == 0.0 ? ((double)i / (double)(n - 1)) * H : (double)i * step) + 0.0;
        t[n - 1] = H;
    }
    for (int i = 0; i < n; ++i) {
        alpha[i] = 1.0 - std::exp(-t[i]);                                // :153
        double tau = t[i] / H;                                           // :166-167
        tau = tau < 0.0 ? 0.0 : (tau > 1.0 ? 1.0 : tau);
        q[i] = 10.0 * std::pow(tau, 3.0) - 15.0 * std::pow(tau, 4.0) + 6.0 * std::pow(tau, 5.0);   // :169
        dtd[i] = i > 0 ? t[i] - t[i - 1] : 0.0;
    }
    if (nl == 1) {
        lat[0] = -3.5;                                                   // linspace(-3.5, 3.5, 1)
    } else {
        const double step = (3.5 - (-3.5)) / (double)(nl - 1);           // :279
        for (int i = 0; i < nl; ++i) lat[i] = (double)i * step + (-3.5);
        lat[nl - 1] = 3.5;
    }
    AV_HIP(hipSetDevice(ctx->device));
    if (ctx->d_ptab) {
        AV_HIP(hipFree(ctx->d_ptab));
        ctx->d_ptab = nullptr;
    }
    AV_HIP(hipMalloc(&ctx->d_ptab, tab.size() * sizeof(double)));
    AV_HIP(hipMemcpy(ctx->d_ptab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->pcfg = *cfg;
    ctx->n_points = n, ctx->n_lat = nl, ctx->n_cand = 3 * nl;
    ctx->planner_ready = true;
    return AV_OK;
}

int av_planner_dims(const av_ctx* ctx, int* n_points, int* n_candidates) {
    AV_REQUIRE(ctx && n_points && n_candidates, AV_EINVAL, "av_planner_dims: null argument");
    AV_REQUIRE(ctx->planner_ready, AV_ESTATE, "av_planner_dims: call av_planner_configure first");
    *n_points = ctx->n_points, *n_candidates = ctx->n_cand;
    return AV_OK;
}

int av_planner_launch_shape(int n_points, int n_candidates, int n_states, int extra, int32_t out[4]) {
    AV_REQUIRE(out, AV_EINVAL, "av_planner_launch_shape: null argument");
    AV_REQUIRE(n_points >= 1 && n_points <= 256 && n_candidates >= 3 && n_candidates <= 192 && n_candidates % 3 == 0, AV_EINVAL,
               "av_planner_launch_shape: %d waypoints, %d candidates: not a configuration av_planner_configure accepts", n_points,
               n_candidates);
    AV_REQUIRE(n_states > 0, AV_EINVAL, "av_planner_launch_shape: n_states must be > 0");
    const PlanLaunch<PlanShared> l = planner_plan<PlanShared>(n_points, n_candidates, n_states, extra != 0);
    out[0] = l.inst->wave, out[1] = l.inst->G, out[2] = l.inst->NW, out[3] = (int32_t)l.lds;
    return AV_OK;
}

int av_planner_plan(av_ctx* ctx, av_stream_t stream, int n_states, const double* state, const double* ref_path,
                    int n_ref, const double* obstacles, int n_obs, double* waypoints, double* cost, int32_t* order) {
    AV_REQUIRE(ctx && state && cost && order, AV_EINVAL, "av_planner_plan: null argument");
    AV_REQUIRE(ctx->planner_ready, AV_ESTATE, "av_planner_plan: call av_planner_configure first");
    AV_REQUIRE(n_states > 0, AV_EINVAL, "av_planner_plan: n_states must be > 0");
    AV_REQUIRE(n_ref >= 0 && n_obs >= 0 && (n_ref == 0 || ref_path) && (n_obs == 0 || obstacles), AV_EINVAL,
               "av_planner_plan: ref_path/obstacles pointer missing");
    AV_REQUIRE(n_ref != 1, AV_EINVAL, "av_planner_plan: a reference path needs >= 2 points (set_reference_path ignores shorter)");
    return plan_dispatch(ctx, as_stream(stream), n_states, state, PlanShared{ref_path, n_ref, obstacles, n_obs}, n_ref > 0 || n_obs > 0,
                         waypoints, cost, order, "av_planner_plan");
}

int av_planner_plan_each(av_ctx* ctx, av_stream_t stream, int n_states, const double* state, const double* ref_path,
                         const int32_t* n_ref, int rcap, int ref_stride, const double* obstacles, const int32_t* n_obs, int ocap,
                         double* waypoints, double* cost, int32_t* order) {
    return plan_each_launch<3>(ctx, stream, n_states, state, ref_path, n_ref, rcap, ref_stride, obstacles, n_obs, ocap, waypoints, cost,
                               order, "av_planner_plan_each");
}

int av_planner_plan_moving(av_ctx* ctx, av_stream_t stream, int n_states, const double* state, const double* ref_path,
                           const int32_t* n_ref, int rcap, int ref_stride, const double* obstacles, const int32_t* n_obs, int ocap,
                           double* waypoints, double* cost, int32_t* order) {
    return plan_each_launch<5>(ctx, stream, n_states, state, ref_path, n_ref, rcap, ref_stride, obstacles, n_obs, ocap, waypoints, cost,
                               order, "av_planner_plan_moving");
}

}  // extern "C"

