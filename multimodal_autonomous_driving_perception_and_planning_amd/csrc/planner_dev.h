// P1-P3: batched candidate-trajectory planner, device code: the kernel argument block (PlanParams; fill_params fills it on the host),
// the reference's arithmetic, one copy each, the list types and plan_block, the workgroup-cooperative planner that planner.hip's
// planner_kernel and the planner role of step.hip's one-launch time-step both run.  planner.hip has the reference, the data layout
// and the kernels.
#pragma once
#include "common.h"

#include <cmath>

namespace {

struct PlanParams {
    int n, n_lat, C;
    double dt, H;
    double w_lat, w_vel, w_acc, w_curv;
    const double *t, *alpha, *q, *dtd, *lat;
    double atq[20];      // atan polynomial (kernel argument -> scalar registers, one per Horner step)
};

// atan(t) = t + t*z*Q(z), z = t*t, t in [0,1]: degree-19 Chebyshev interpolant of (atan(sqrt z)/sqrt z - 1)/z
// derived in long double by tools/atan_poly.py; float64 Horner error <= 2.1 ulp over [0,1].
static const double ATAN_Q[20] = {
    -0x1.5555555555549p-2, 0x1.99999999979b9p-3,  -0x1.24924923e22b4p-3, 0x1.c71c718e5a102p-4,
    -0x1.745d120df88fbp-4, 0x1.3b1362fc35ab5p-4,  -0x1.110deef367776p-4, 0x1.e1b3c8d50e91fp-5,
    -0x1.ae2c7119eb922p-5, 0x1.81fdd2525246ap-5,  -0x1.56daf4786fd80p-5, 0x1.2575526b2309ap-5,
    -0x1.d168e01adf666p-6, 0x1.462cc26bda000p-6,  -0x1.8055065b73333p-7, 0x1.693bd6b79999ap-8,
    -0x1.fdf4e15cccccdp-10, 0x1.f224118000000p-12, -0x1.2568700000000p-14, 0x1.2ed799999999ap-18,
};

// atan2 for finite arguments of ordinary magnitude (waypoint deltas), |error| <= ~2 ulp like libm's.
// NumPy's arctan2 is libm's, so this call is tolerance-matched either way; what this version avoids is
// ocml's special-case handling and the ~40 moves that materialise its 64-bit constants per call.
__device__ __forceinline__ double atan2_fast(double y, double x, const double (&Q)[20]) {
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const bool swap = ay > ax;
    const double mx = swap ? ay : ax, mn = swap ? ax : ay;
    // t = mn / mx: reciprocal refined twice (as the compiler's own f64 divide does), then one residual
    // correction of the quotient -> correctly rounded but for astronomically rare operands
    double r = __builtin_amdgcn_rcp(mx);
    r = __builtin_fma(__builtin_fma(-mx, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-mx, r, 1.0), r, r);
    double t = mn * r;
    t = __builtin_fma(__builtin_fma(-t, mx, mn), r, t);
    t = mx == 0.0 ? 0.0 : t;                                     // atan2(0, 0) = 0
    const double z = t * t;
    double pz = Q[19];
#pragma unroll
    for (int k = 18; k >= 0; --k) pz = __builtin_fma(pz, z, Q[k]);
    double a = __builtin_fma(t * z, pz, t);
    a = swap ? 1.5707963267948966 - a : a;
    a = x < 0.0 ? 3.141592653589793 - a : a;
    return __builtin_copysign(a, y);
}

__host__ __device__ constexpr int even_up(int v) { return (v + 1) & ~1; }

// doubles of dynamic LDS for G start states per workgroup of NW waves
__host__ __device__ inline size_t plan_lds_doubles(int G, int n, int C, int NW = 4) {
    return (size_t)G * 3 * n * 2 + even_up(G * 3 * 3) + (size_t)G * 8 + (size_t)3 * even_up(G * C) + (size_t)NW * n * 6;
}

// Output ring of planner_wave_kernel: 256 units of 16 B.  It holds at most 63 carried units + one tile of
// 3n <= 192 units; FPW*3*n <= 384 doubles of phase-1 scratch also fit.
constexpr int RING_UNITS = 256, RING_DOUBLES = RING_UNITS * 2;

// doubles of dynamic LDS of ONE wave of planner_wave_kernel, FPW start states each: (v, s) | ring | costs | sums | heading terms
__host__ __device__ constexpr size_t wave_lds_doubles(int FPW, int n, int C) {
    return (size_t)FPW * 3 * n * 2 + RING_DOUBLES + even_up(FPW * C) + FPW * 3 * 4 + FPW * 8;
}
// the most its four waves ever need (n <= 64, C <= 192, two states per wave): (768 + 512 + 384 + 24 + 16) doubles each
static_assert(wave_lds_doubles(2, 64, 192) * 4 * sizeof(double) == 54528, "the wave kernel fits 64 KB of LDS whatever the configuration");

// Orders this wave's LDS accesses for the compiler.  The hardware executes one wave's DS operations
// in issue order, so no s_waitcnt is needed (and none for outstanding global stores either).
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// ---- the reference's arithmetic, one copy each; every kernel below calls these ----------------------------------------------
__device__ __forceinline__ double target_speed(int k) { return 8.0 + 2.0 * (double)k; }                        // [8.0, 10.0, 12.0]  (:280)
__device__ __forceinline__ double blend_velocity(double v0, double dv, double alpha) { return v0 + dv * alpha; }   // :153-154
__device__ __forceinline__ double velocity_term(double w_vel, double v) {                                      // :236
    const double e = v - 10.0;
    return w_vel * (e * e);
}
// from two consecutive velocities and the time between them; the callers add it up only where that time is > 0 (:240-244)
__device__ __forceinline__ double acceleration_term(double w_acc, double v, double vp, double dtd) {
    const double a = (v - vp) / dtd;
    return w_acc * (a * a);
}
// A start state as the waypoints are placed from it: the point at arc length s is `along` the heading (:175-176), its lateral
// offset d `across` it (:179-180); a waypoint is the sum of the two.
struct PlanFrame {
    double x0, y0, cs, sn, c2, s2;      // position, cos / sin of the heading and of heading + pi/2
    __device__ __forceinline__ void along(double s, double& bx, double& by) const { bx = x0 + s * cs, by = y0 + s * sn; }
    __device__ __forceinline__ void across(double d, double& dx, double& dy) const { dx = d * c2, dy = d * s2; }
    __device__ __forceinline__ void point(double s, double d, double& x, double& y) const {
        double dx, dy;
        along(s, x, y), across(d, dx, dy);
        x = x + dx, y = y + dy;
    }
};
// curvature of interior waypoint i of an AoS tile whose headings are in place (:196)
__device__ __forceinline__ double tile_curvature(const double* tile, int i, double dt) {
    const double* w = tile + (size_t)i * 6;
    return (w[2] - tile[(size_t)(i - 1) * 6 + 2]) / (w[3] * dt + 1e-6);
}
// the last waypoint has no forward difference: it repeats the heading before it, a lone one the start state's (:190)
__device__ __forceinline__ void tile_last_heading(double* tile, int n, double h0) {
    tile[(size_t)(n - 1) * 6 + 2] = n > 1 ? tile[(size_t)(n - 2) * 6 + 2] : h0;
}
// reference-path term of a waypoint: the squared distance to the nearest of the n_ref > 0 path points (:229-231)
__device__ __forceinline__ double ref_path_term(double w_lat, const double* ref, int n_ref, double x, double y) {
    double md = INFINITY;
    for (int r = 0; r < n_ref; ++r) {
        const double dx = ref[2 * r] - x, dy = ref[2 * r + 1] - y;
        const double dd = sqrt(dx * dx + dy * dy);
        md = dd < md ? dd : md;
    }
    return w_lat * (md * md);
}
// adds to `sum` what obstacle row o (x, y, radius; MOVING: + vx, vy, the disc where its velocity has carried it by the waypoint's
// time tw) costs the waypoint at (x, y) (:253-259).  The callers own the loops: their summation orders differ.
template <bool MOVING>
__device__ __forceinline__ void add_obstacle_penalty(double& sum, const double* o, double x, double y, double tw) {
    double ox = o[0], oy = o[1];
    const double rad = o[2];
    if constexpr (MOVING) ox = ox + o[3] * tw, oy = oy + o[4] * tw;
    const double ex = x - ox, ey = y - oy;
    const double dist = sqrt(ex * ex + ey * ey);
    if (dist < rad * 2.0) sum = sum + 1000.0 * (rad * 2.0 - dist);
    else if (dist < rad * 4.0) sum = sum + 10.0 / (dist - rad + 0.1);
}
// candidate c of state f: its stable ascending rank among the state's C costs cc (== Python's stable sort, :300), stored with its cost
__device__ __forceinline__ void rank_and_store(const double* cc, int C, int c, int f, double* __restrict__ cost,
                                               int32_t* __restrict__ order) {
    const double mine = cc[c];
    int rank = 0;
    for (int o2 = 0; o2 < C; ++o2) {
        const double v = cc[o2];
        rank += (v < mine || (v == mine && o2 < c)) ? 1 : 0;
    }
    cost[(size_t)f * C + c] = mine;
    order[(size_t)f * C + rank] = c;
}

// The workgroup-cooperative planner for small batches (and n > 64): G consecutive start states f0 .. f0 + G - 1 by a workgroup of
// NW waves.  A device function, so that the fused time-step kernel (step.hip) runs the very same code after its Kalman step.
//   phase 1  per (state, speed) pair, one wave each: lanes make the per-waypoint terms in parallel (velocity blend v_i, v_i dt, the
//            velocity and acceleration cost terms -- the 50 float64 divides of the acceleration used to sit in ONE lane's
//            sequential loop) and the wave adds up the arc length s_i = s_{i-1} + v_i dt left to right, the reference's order
//            (:156-157), terms broadcast from registers by v_readlane: no memory access on the sequential path.  Only this
//            chain is in front of the barrier; the two cost chains (:235-244) have no consumer before phase 3 and run behind
//            it, in the same waves, which in exchange get fewer trajectories (in-kernel cycle stamps: the three chains back to
//            back were 6 of the kernel's 14 us for one start state)
//   phase 2  each wave takes whole trajectories; lane = waypoint (positions, tangent heading by atan2_fast, curvature, cost terms;
//            AoS image assembled in a per-wave LDS tile and streamed out as 16-byte-per-lane stores); per-trajectory sums by DPP
//   phase 3  costs assembled from the per-trajectory sums as ([reference path] + velocity + acceleration) + curvature + obstacles.
//            The reference adds every per-waypoint term into one running sum (:224-259), so the two agree to rounding, not bit
//            for bit (nor do the headings: atan2_fast vs libm); then the stable rank of the C costs (== Python's stable sort, :300)
// The fused time-step kernel's variations (all defaults: the planner kernels' own behaviour):
//   state_f0  index in `state` of start state f0 (default f0: `state` is the batch's array).  The step kernel hands over the four
//             doubles its Kalman wave left in LDS, index 0, while wp / cost / order stay indexed by the stream
//   rot       the waves' tasks (phase-1 pair, heading terms, trajectories) are dealt by (wave - rot) mod NW: the step kernel keeps
//             its Kalman wave free of phase-1 work
//   after1    called by every wave as after1(task wave id) behind the phase-1 barrier and its cost chains: work with no consumer
//             inside the planner, on a wave with slack (task waves < 3 G take fewer trajectories)
struct PlanNoHook {
    __device__ __forceinline__ void operator()(int) const {}
};

// Where a start state's reference path and obstacle list come from.  `at(f)` is what state f reads, asked by a whole wave for
// one state (f wave-uniform); `has_ref(f)` may be asked per lane.  For PlanShared both are the launch's own arguments whatever
// f is, so those instantiations pay nothing for the lookup.
struct PlanLists {
    const double* ref; int n_ref;      // [n_ref][2]
    const double* obs; int n_obs;      // [n_obs][OSTRIDE]
};
// one reference path and one obstacle list for every state of the launch (av_planner_plan)
struct PlanShared {
    static constexpr int OSTRIDE = 3;             // doubles per obstacle row: (x, y, radius)
    static constexpr bool MOVING = false;
    const double* ref; int n_ref;
    const double* obs; int n_obs;
    __device__ __forceinline__ PlanLists at(int) const { return PlanLists{ref, n_ref, obs, n_obs}; }
    __device__ __forceinline__ bool has_ref(int) const { return n_ref > 0; }
};
// state f reads obstacle list f and reference path f / ref_stride (av_planner_plan_each); a null list pointer: none for any state.
// OS = 5 (av_planner_plan_moving): rows (x, y, radius, vx, vy), the disc of the waypoint with timestamp t is at (x + vx t, y + vy t);
// the row width and the motion are properties of the type, so the OS = 3 kernels are the ones they were
template <int OS>
struct PlanEachT {
    static constexpr int OSTRIDE = OS;
    static constexpr bool MOVING = OS == 5;
    const double* ref; const int32_t* n_ref;      // [n_paths][rcap][2], [n_paths]
    const double* obs; const int32_t* n_obs;      // [n_states][ocap][OS], [n_states]
    int rcap, ref_stride, ocap;
    __device__ __forceinline__ int path_points(int pth) const {
        const int k = n_ref[pth] > rcap ? rcap : n_ref[pth];
        return k < 2 ? 0 : k;                                   // set_reference_path ignores lists shorter than two (:100-101)
    }
    __device__ __forceinline__ bool has_ref(int f) const { return ref && path_points(f / ref_stride) > 0; }
    __device__ __forceinline__ PlanLists at(int f) const {
        f = __builtin_amdgcn_readfirstlane(f);                  // (the same in every lane: counts and lists by scalar loads)
        PlanLists l{nullptr, 0, nullptr, 0};
        if (ref) {
            const int pth = f / ref_stride;
            l.n_ref = path_points(pth);
            l.ref = ref + (size_t)pth * rcap * 2;
        }
        if (obs) {
            const int k = n_obs[f];
            l.n_obs = k < 0 ? 0 : (k > ocap ? ocap : k);
            l.obs = obs + (size_t)f * ocap * OS;
        }
        return l;
    }
};
using PlanEach = PlanEachT<3>;
using PlanEachMoving = PlanEachT<5>;

template <int G, int NW, class Hook = PlanNoHook, class Lists = PlanShared>
__device__ __forceinline__ void plan_block_lists(const PlanParams& p, int f0, int n_states, const double* __restrict__ state,
                                                 const Lists lists, double* __restrict__ wp, double* __restrict__ cost,
                                                 int32_t* __restrict__ order, double* sm, int state_f0 = -1, int rot = 0,
                                                 Hook after1 = Hook()) {
    const int n = p.n, C = p.C;
    const int sd = state_f0 < 0 ? 0 : state_f0 - f0;      // start state f is state[(f + sd) * 4 ..]
    double* vs = sm;                                   // [G][3][n][2]  (v, s)
    double* base = vs + (size_t)G * 3 * n * 2;         // [G][3][3]     S_v, S_a, running(S_v then acc terms)
    double* trig = base + even_up(G * 3 * 3);          // [G][8]        x0 y0 cos sin cos(h+pi/2) sin(h+pi/2) h0
    double* costs = trig + G * 8;                      // [3][G][C]     per trajectory: reference-path, curvature, obstacle sums; then [0]: the cost
    double* stage_all = costs + 3 * even_up(G * C);    // [NW][n*6]
    const int CS = even_up(G * C);

    const int tid = threadIdx.x, lane = tid & 63;
    // (the wave's number by the scalar unit: its place in the dealing, the trajectories it takes, their indices, tile and output
    // addresses are then scalar values, not one copy per lane in vector registers)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* stage = stage_all + (size_t)wave * n * 6;
    const int wid = (wave + NW - rot) % NW;            // the wave's place in the dealing of tasks
    constexpr int P = G * 3;                           // (state, speed) pairs
    static_assert(NW >= 2, "the heading terms take the last wave");   // (fast, P <= NW: one wave per pair keeps its terms in registers)

    auto bcast = [&](double x, int i) {
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)__double_as_longlong(x), i);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)__double_as_longlong(x) >> 32), i);
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    };
    auto terms = [&](double v0, double dv, int i, double& v, double& vdt, double& velt, double& acct) {
        v = blend_velocity(v0, dv, p.alpha[i]);
        vdt = v * p.dt;
        velt = velocity_term(p.w_vel, v);
        acct = 0.0;
        if (i > 0)                                            // (added up only where dtd[i] > 0, like the reference's test)
            acct = acceleration_term(p.w_acc, v, blend_velocity(v0, dv, p.alpha[i - 1]), p.dtd[i]);
    };
    // the cost chains of one pair from its terms: S_v over all waypoints, then the acceleration terms on top (:235-244)
    auto cost_chains = [&](double velt, double acct, unsigned long long hasm, double* b) {
        double sv = 0.0;
#pragma unroll
        for (int i = 0; i < 64; ++i)
            if (i < n) sv = sv + bcast(velt, i);
        double run = sv, sa = 0.0;
#pragma unroll
        for (int i = 1; i < 64; ++i)
            if ((hasm >> i) & 1ull) {          // (hasm has no bit from n on: tested again here, the 63 `i < n` of the loop above stay live in scalar pairs)
                const double term = bcast(acct, i);
                run = run + term, sa = sa + term;
            }
        if (lane == 0) b[0] = sv, b[1] = sa, b[2] = run;
    };

    // ---- phase 1 ---------------------------------------------------------------------------------
    const bool fast = n <= 64 && P <= NW;              // terms in registers, one pair per wave
    double k_velt = 0.0, k_acct = 0.0;                 // this wave's pair: cost terms kept for after the barrier
    unsigned long long k_has = 0;
    bool k_live = false;
    if (fast) {
        if (wid < P) {
            const int g = wid / 3, k = wid - g * 3, f = f0 + g;
            if (f < n_states) {
                const double v0 = state[(size_t)(f + sd) * 4 + 3];
                const double dv = target_speed(k) - v0;
                double* o = vs + ((size_t)(g * 3 + k) * n) * 2;
                double v = 0.0, vdt = 0.0;
                bool has = false;
                if (lane < n) terms(v0, dv, lane, v, vdt, k_velt, k_acct), has = lane > 0 && p.dtd[lane] > 0.0;
                k_has = __ballot(has), k_live = true;
                double sacc = 0.0, my_s = 0.0;
#pragma unroll
                for (int i = 1; i < 64; ++i)
                    if (i < n) {
                        sacc = sacc + bcast(vdt, i);          // :157
                        my_s = lane == i ? sacc : my_s;
                    }
                if (lane < n) o[2 * lane] = v, o[2 * lane + 1] = my_s;
            }
        }
    } else {
        for (int pr = wid; pr < P; pr += NW) {
            const int g = pr / 3, k = pr - g * 3, f = f0 + g;
            if (f >= n_states) continue;
            const double v0 = state[(size_t)(f + sd) * 4 + 3];
            const double dv = target_speed(k) - v0;
            double* o = vs + ((size_t)(g * 3 + k) * n) * 2;
            double* b = base + (g * 3 + k) * 3;
            double* tv = stage;                               // [n] v_i dt | [n] velocity cost term | [n] acceleration cost term
            for (int i = lane; i < n; i += 64) {
                double v, vdt, velt, acct;
                terms(v0, dv, i, v, vdt, velt, acct);
                o[2 * i] = v, tv[i] = vdt, tv[n + i] = velt, tv[2 * n + i] = acct;
            }
            wave_lds_fence();
            if (lane == 0) {
                double sacc = 0.0, sv = 0.0;
                o[1] = 0.0;
                sv = sv + tv[n];
                for (int i = 1; i < n; ++i) {
                    sacc = sacc + tv[i];                      // :157
                    o[2 * i + 1] = sacc;
                    sv = sv + tv[n + i];
                }
                double run = sv, sa = 0.0;
                for (int i = 1; i < n; ++i) {
                    if (p.dtd[i] > 0.0) {
                        const double term = tv[2 * n + i];
                        run = run + term, sa = sa + term;
                    }
                }
                b[0] = sv, b[1] = sa, b[2] = run;
            }
            wave_lds_fence();
        }
    }
    // heading terms: the last wave (free in phase 1 when the pairs are fewer than the waves), two lanes per state -- lane 2 g takes
    // sin / cos of the heading, lane 2 g + 1 of heading + pi/2 (one sincos each, side by side)
    if (wid == NW - 1 && lane < 2 * G) {
        const int g = lane >> 1, f = f0 + g;
        if (f < n_states) {
            const double h0 = state[(size_t)(f + sd) * 4 + 2];
            double* tg = trig + g * 8;
            double sn, cs;
            if (lane & 1) {
                sincos(h0 + 1.5707963267948966, &sn, &cs);       // heading0 + np.pi/2  (:179)
                tg[4] = cs, tg[5] = sn;
            } else {
                sincos(h0, &sn, &cs);
                tg[0] = state[(size_t)(f + sd) * 4 + 0], tg[1] = state[(size_t)(f + sd) * 4 + 1];
                tg[2] = cs, tg[3] = sn, tg[6] = h0;
            }
        }
    }
    __syncthreads();
    if (k_live) cost_chains(k_velt, k_acct, k_has, base + wid * 3);        // consumed in phase 3
    after1(wid);

    // ---- phase 2 ---------------------------------------------------------------------------------
    // the per-waypoint constants of this lane's first waypoint, loaded once (not once per trajectory behind the LDS fences)
    const double q_l = lane < n ? p.q[lane] : 0.0, q_l1 = lane + 1 < n ? p.q[lane + 1] : 0.0, t_l = lane < n ? p.t[lane] : 0.0;
    // trajectories are dealt round-robin starting BEHIND the waves that still have cost chains to add up
    for (int j = fast ? (wid - P % NW + NW) % NW : wid; j < G * C; j += NW) {
        const int g = j / C, c = j - g * C, f = f0 + g;
        if (f >= n_states) continue;
        const PlanLists ls = lists.at(f);                       // this state's reference path and obstacles
        const double* ref = ls.ref;
        const double* obs = ls.obs;
        const int n_ref = ls.n_ref, n_obs = ls.n_obs;
        const bool extra = n_ref > 0 || n_obs > 0;
        const int li = c / 3, k = c - li * 3;
        const double df = p.lat[li];
        const double* tg = trig + g * 8;
        const PlanFrame fr{tg[0], tg[1], tg[2], tg[3], tg[4], tg[5]};
        const double h0 = tg[6];
        const double* o = vs + ((size_t)(g * 3 + k) * n) * 2;

        for (int i = lane; i < n; i += 64) {
            const double v = o[2 * i], s = o[2 * i + 1];
            const bool first = i == lane;
            double x, y, hd = 0.0;
            fr.point(s, df * (first ? q_l : p.q[i]), x, y);
            if (i < n - 1) {
                double x1, y1;
                fr.point(o[2 * i + 3], df * (first ? q_l1 : p.q[i + 1]), x1, y1);
                hd = atan2_fast(y1 - y, x1 - x, p.atq);         // :188
            }
            double* w = stage + (size_t)i * 6;
            w[0] = x, w[1] = y, w[2] = hd, w[3] = v, w[4] = first ? t_l : p.t[i], w[5] = 0.0;
        }
        wave_lds_fence();
        double lat_sum = 0.0, curv_sum = 0.0, obs_sum = 0.0;
        for (int i = lane; i < n; i += 64) {
            double* w = stage + (size_t)i * 6;
            double curv = 0.0;
            if (i > 0 && i < n - 1) w[5] = curv = tile_curvature(stage, i, p.dt);
            curv_sum += p.w_curv * (curv * curv);               // :248
            const double x = w[0], y = w[1];
            if (n_ref > 0) lat_sum += ref_path_term(p.w_lat, ref, n_ref, x, y);
            for (int q = 0; q < n_obs; ++q)
                add_obstacle_penalty<Lists::MOVING>(obs_sum, obs + Lists::OSTRIDE * q, x, y, w[4]);
        }
        wave_lds_fence();
        if (lane == 0) tile_last_heading(stage, n, h0);
        curv_sum = wave_sum_dpp(curv_sum);
        if (extra) lat_sum = wave_sum_dpp(lat_sum), obs_sum = wave_sum_dpp(obs_sum);
        if (lane == 0) costs[g * C + c] = lat_sum, costs[CS + g * C + c] = curv_sum, costs[2 * CS + g * C + c] = obs_sum;
        wave_lds_fence();
        if (wp) {
            const double2* src = reinterpret_cast<const double2*>(stage);
            double2* dst = reinterpret_cast<double2*>(wp + ((size_t)f * C + c) * n * 6);
            for (int q = lane; q < n * 3; q += 64) dst[q] = src[q];
        }
        wave_lds_fence();
    }
    __syncthreads();

    // ---- phase 3: costs, stable ascending rank (:300) -------------------------------------------------------------------------
    for (int idx = tid; idx < G * C; idx += NW * 64) {
        const int g = idx / C, c = idx - g * C, k = c % 3;
        const double* b = base + (g * 3 + k) * 3;
        const bool with_ref = lists.has_ref(f0 + g < n_states ? f0 + g : f0);   // (states past the batch: computed, never stored)
        // reference accumulates [ref-path] -> velocity -> acceleration -> curvature -> obstacles
        const double va = with_ref ? (costs[idx] + b[0]) + b[1] : b[2];
        const double total = (va + costs[CS + idx]) + costs[2 * CS + idx];
        costs[idx] = total;
    }
    __syncthreads();
    for (int idx = tid; idx < G * C; idx += NW * 64) {
        const int g = idx / C, c = idx - g * C, f = f0 + g;
        if (f >= n_states) continue;
        rank_and_store(costs + g * C, C, c, f, cost, order);
    }
}

// plan_block_lists with one reference path and one obstacle list for all states: what the fused time-step kernel calls
template <int G, int NW, class Hook = PlanNoHook>
__device__ __forceinline__ void plan_block(const PlanParams& p, int f0, int n_states, const double* state, const double* ref, int n_ref,
                                           const double* obs, int n_obs, double* wp, double* cost, int32_t* order, double* sm,
                                           int state_f0 = -1, int rot = 0, Hook after1 = Hook()) {
    plan_block_lists<G, NW, Hook, PlanShared>(p, f0, n_states, state, PlanShared{ref, n_ref, obs, n_obs}, wp, cost, order, sm, state_f0,
                                              rot, after1);
}

}  // namespace

static void fill_params(const av_ctx* ctx, PlanParams& p) {
    const int n = ctx->n_points;
    p.n = n, p.n_lat = ctx->n_lat, p.C = ctx->n_cand;
    p.dt = ctx->pcfg.dt, p.H = ctx->pcfg.planning_horizon;
    p.w_lat = ctx->pcfg.w_lateral, p.w_vel = ctx->pcfg.w_velocity, p.w_acc = ctx->pcfg.w_acceleration;
    p.w_curv = ctx->pcfg.w_curvature;
    p.t = ctx->d_ptab, p.alpha = p.t + n, p.q = p.alpha + n, p.dtd = p.q + n, p.lat = p.dtd + n;
    for (int k = 0; k < 20; ++k) p.atq[k] = ATAN_Q[k];
}
