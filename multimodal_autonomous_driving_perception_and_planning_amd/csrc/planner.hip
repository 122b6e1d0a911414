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

static void fill_params(const av_ctx* ctx, PlanParams& p) {
    const int n = ctx->n_points;
    p.n = n, p.n_lat = ctx->n_lat, p.C = ctx->n_cand;
    p.dt = ctx->pcfg.dt, p.H = ctx->pcfg.planning_horizon;
    p.w_lat = ctx->pcfg.w_lateral, p.w_vel = ctx->pcfg.w_velocity, p.w_acc = ctx->pcfg.w_acceleration;
    p.w_curv = ctx->pcfg.w_curvature;
    p.t = ctx->d_ptab, p.alpha = p.t + n, p.q = p.alpha + n, p.dtd = p.q + n, p.lat = p.dtd + n;
    for (int k = 0; k < 20; ++k) p.atq[k] = ATAN_Q[k];
}

#ifndef AVHOT_DEVICE_ONLY      // (step.hip includes this file for its device code only)

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

#endif  // AVHOT_DEVICE_ONLY
