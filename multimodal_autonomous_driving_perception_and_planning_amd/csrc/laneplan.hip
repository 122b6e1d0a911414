// Lane planner: the planner's candidates charged for the lane boundaries they cross, by the boundaries' marks, and ranked again
// (av_lane_plan, include/avhot.h).  A post-pass over what av_planner_plan_each / _plan_moving wrote: it reads
// their waypoints and costs and runs none of their arithmetic but the ranking rule (planner_dev.h's rank_and_store).
//
// One launch, one workgroup of 256 threads per vehicle.  Thread 64 takes the sine and cosine of the heading while threads 0 .. 9 lay
// out the vehicle's lines (everything they decide on is the same for the whole workgroup: scalar loads).  The candidates are taken
// in tiles of TC: the tile's waypoints are carried into the vehicle frame once, one thread per waypoint, and staged in LDS as
// (X, Y); then one thread per (candidate, line) pair walks along the candidate's waypoints in index order -- the sums are
// sequential by construction, and the threads of one candidate read one LDS address, a broadcast -- and leaves its term and its
// bits in LDS; then one thread per candidate adds its lines up in order.  A tile is at most TILE_POINTS waypoints (the default 21
// candidates of 51 waypoints are one tile), so LDS does not grow with the limits 192 x 256.  Behind the tiles one thread per
// candidate ranks the totals, and thread 0 writes the row.  The kernel is bound by latency, not by bandwidth: a vehicle reads 51 KB.
#include "common.h"
#include "planner_dev.h"

#include <cmath>

namespace {

constexpr int MAXB = AV_ROAD_LANES_MAX_BOUNDS, MAXL = AV_LANEPLAN_MAX_LINES, MAXC = AV_LANEPLAN_MAX_CAND, MAXN = AV_LANEPLAN_MAX_POINTS;
constexpr int THREADS = 256, TILE_POINTS = 1536, TILE_CAND = 64;
static_assert(TILE_POINTS >= MAXN, "a tile holds at least one candidate");

// candidates per tile: what TILE_POINTS waypoints hold, at most TILE_CAND (the pair arrays' size)
__host__ __device__ inline int tile_cands(int C, int n) {
    const int t = TILE_POINTS / n;
    return t < C ? (t < TILE_CAND ? t : TILE_CAND) : (C < TILE_CAND ? C : TILE_CAND);
}

__device__ __forceinline__ int mark_type(int t) { return t >= 0 && t <= 2 ? t : AV_ROAD_MARK_UNKNOWN; }
// w[type] of a kernel argument, by selects: an index that differs from lane to lane would send the table through scratch
__device__ __forceinline__ double by_type(const double (&w)[3], int type) {
    return type == AV_ROAD_MARK_SOLID ? w[1] : type == AV_ROAD_MARK_DASHED ? w[2] : w[0];
}

__global__ void __launch_bounds__(THREADS) lane_plan_kernel(av_lane_plan_cfg cfg, int C, int n, const double* __restrict__ plan_state,
                                                            const double* __restrict__ waypoints, const double* __restrict__ cost,
                                                            const av_road_lane_bound* __restrict__ bounds,
                                                            const av_road_lanes_row* __restrict__ lanes,
                                                            const av_road_mark* __restrict__ marks,
                                                            const av_road_marks_row* __restrict__ sides,
                                                            av_lane_plan_line* __restrict__ lines, double* __restrict__ lane_cost,
                                                            double* __restrict__ total, int32_t* order, uint32_t* __restrict__ cross,
                                                            int32_t* __restrict__ delta, av_lane_plan_row* __restrict__ row) {
    __shared__ double2 pts[TILE_POINTS];                                 // (X, Y) of the tile's waypoints, candidate-major
    __shared__ double pair_term[TILE_CAND * MAXL];                       // per (candidate of the tile, line)
    __shared__ uint32_t pair_bits[TILE_CAND * MAXL];                     // bit 0 crossed, bit 1 on, bits 2..3 delta_j + 1
    __shared__ double s_cost[MAXC], s_lane[MAXC], s_total[MAXC];
    __shared__ uint32_t s_cross[MAXC];
    __shared__ int32_t s_delta[MAXC];
    __shared__ av_lane_plan_line s_lines[MAXL];
    __shared__ double s_trig[2];
    __shared__ int s_base;
    const int v = blockIdx.x, tid = threadIdx.x;

    // ---- 1 the lines (what decides is the same in every thread) ----
    const av_road_lanes_row& ln = lanes[v];
    const int nb = min(max(ln.n_bounds, 0), MAXB);
    const bool lane = (ln.status & AV_ROAD_LANE) != 0;
    const av_road_lane_bound* const bd = bounds + (size_t)v * MAXB;
    bool has_left = false, has_right = false;
    for (int b = 0; b < nb; ++b) has_left |= (bd[b].flags & AV_ROAD_BOUND_LEFT) != 0, has_right |= (bd[b].flags & AV_ROAD_BOUND_RIGHT) != 0;
    const bool add_left = lane && !has_left, add_right = lane && !has_right;
    const int n_lines = nb + (int)add_left + (int)add_right;
    const int left_type = sides ? mark_type(sides[v].left.type) : AV_ROAD_MARK_UNKNOWN;
    const int right_type = sides ? mark_type(sides[v].right.type) : AV_ROAD_MARK_UNKNOWN;
    if (tid < MAXL) {
        av_lane_plan_line l{};
        l.source = -1;
        if (tid < nb) {
            const av_road_lane_bound b = bd[tid];
            l.a0 = b.a0, l.a1 = b.a1, l.a2 = b.a2, l.xe = b.x_max, l.source = tid;
            l.type = (b.flags & AV_ROAD_BOUND_LEFT)    ? left_type
                     : (b.flags & AV_ROAD_BOUND_RIGHT) ? right_type
                     : marks                           ? mark_type(marks[(size_t)v * MAXB + tid].type)
                                                       : AV_ROAD_MARK_UNKNOWN;
        } else if (tid < n_lines) {
            const bool is_left = add_left && tid == nb;
            const double* a = is_left ? ln.left : ln.right;
            l.a0 = a[0], l.a1 = a[1], l.a2 = a[2], l.xe = cfg.x_far;
            l.type = is_left ? left_type : right_type, l.source = is_left ? AV_LANEPLAN_SRC_LEFT : AV_LANEPLAN_SRC_RIGHT;
        }
        s_lines[tid] = l;
        lines[(size_t)v * MAXL + tid] = l;
    }
    if (tid == 64) {
        double sn, cs;
        sincos(plan_state[(size_t)v * 4 + 2], &sn, &cs);
        s_trig[0] = cs, s_trig[1] = sn;
    }
    if (tid == 0) s_base = 0;
    for (int c = tid; c < C; c += THREADS) s_cost[c] = cost[(size_t)v * C + c];
    __syncthreads();

    // ---- 2 the course ----
    const bool follow = cfg.follow != 0 && lane;
    const double c1 = follow ? ln.centre[1] : 0.0, c2 = follow ? ln.centre[2] : 0.0;
    const double x0 = plan_state[(size_t)v * 4 + 0], y0 = plan_state[(size_t)v * 4 + 1], cs = s_trig[0], sn = s_trig[1];
    const double hw = cfg.half_width, x_far = cfg.x_far;

    // ---- 3, 4 the candidates, a tile at a time ----
    const int TC = tile_cands(C, n);
    for (int cbase = 0; cbase < C; cbase += TC) {
        const int tc = min(TC, C - cbase);
        if (n_lines > 0) {
            const double* const wp = waypoints + ((size_t)v * C + cbase) * n * 6;      // the tile's candidates lie one behind the other
            for (int q = tid; q < tc * n; q += THREADS) {
                const double dx = wp[(size_t)q * 6] - x0, dy = wp[(size_t)q * 6 + 1] - y0;
                pts[q] = make_double2(dx * cs + dy * sn, dy * cs - dx * sn);
            }
            __syncthreads();
            for (int p = tid; p < tc * n_lines; p += THREADS) {
                const int cl = p / n_lines, j = p - cl * n_lines;
                const av_lane_plan_line l = s_lines[j];
                const double b1 = l.a1 - c1, b2 = l.a2 - c2, w_on = by_type(cfg.w_on, l.type);
                const double2* const cp = pts + cl * n;
                bool any = false, crossed = false, on_any = false, first_side = false, last_side = false;
                double on = 0.0, last_d = 0.0;
                for (int i = 0; i < n; ++i) {
                    const double X = cp[i].x, Y = cp[i].y;
                    if (!(X >= 0.0 && X <= l.xe && X <= x_far)) continue;
                    const double e = Y - ((l.a0 + b1 * X) + b2 * (X * X));
                    const bool side = e > 0.0;
                    const double d = hw - fabs(e);
                    if (any) crossed |= side != last_side;
                    else first_side = side;
                    if (d > 0.0) on = on + w_on * (d * d), on_any = true;
                    any = true, last_side = side, last_d = d;
                }
                const double end = any && last_d > 0.0 ? cfg.w_end * (last_d * last_d) : 0.0;
                pair_term[cl * MAXL + j] = ((crossed ? by_type(cfg.w_cross, l.type) : 0.0) + on) + end;
                const int dj = any ? (int)last_side - (int)first_side : 0;
                pair_bits[cl * MAXL + j] = (crossed ? 1u : 0u) | (on_any ? 2u : 0u) | ((uint32_t)(dj + 1) << 2);
            }
            __syncthreads();
        }
        for (int cl = tid; cl < tc; cl += THREADS) {
            double sum = 0.0;
            uint32_t cr = 0;
            int dl = 0;
            for (int j = 0; j < n_lines; ++j) {
                const uint32_t b = pair_bits[cl * MAXL + j];
                sum = sum + pair_term[cl * MAXL + j];
                cr |= ((b & 1u) << j) | (((b >> 1) & 1u) << (16 + j));
                dl += (int)(b >> 2) - 1;
            }
            const int c = cbase + cl;
            s_lane[c] = sum, s_total[c] = s_cost[c] + sum, s_cross[c] = cr, s_delta[c] = dl;
            lane_cost[(size_t)v * C + c] = sum, cross[(size_t)v * C + c] = cr, delta[(size_t)v * C + c] = dl;
        }
        __syncthreads();
    }

    // ---- 4 the ranks; 5 the row ----
    for (int c = tid; c < C; c += THREADS) {
        rank_and_store(s_total, C, c, v, total, order);
        const double mine = s_cost[c];
        int better = 0;
        for (int o = 0; o < C; ++o) better += (s_cost[o] < mine || (s_cost[o] == mine && o < c)) ? 1 : 0;
        if (better == 0) s_base = c;
    }
    __syncthreads();
    if (tid != 0) return;
    av_lane_plan_row r{};
    const int best = min(max(order[(size_t)v * C], 0), C - 1);
    r.best = best, r.base_best = s_base, r.delta = s_delta[best];
    r.maneuver = r.delta < 0 ? AV_LANEPLAN_LEFT : r.delta > 0 ? AV_LANEPLAN_RIGHT : AV_LANEPLAN_KEEP;
    r.crossed = s_cross[best] & 0xffffu;
    for (int j = 0; j < n_lines; ++j) {
        if (!((r.crossed >> j) & 1u)) continue;
        if (s_lines[j].type == AV_ROAD_MARK_SOLID) r.crossed_solid |= 1u << j;
        if (s_lines[j].type == AV_ROAD_MARK_UNKNOWN) r.crossed_unknown |= 1u << j;
    }
    r.n_lines = n_lines;
    r.flags = (follow ? AV_LANEPLAN_FOLLOW : 0) | (best != s_base ? AV_LANEPLAN_CHANGED : 0) |
              ((r.crossed_solid | r.crossed_unknown) ? AV_LANEPLAN_FORCED : 0) | (n_lines == 0 ? AV_LANEPLAN_NO_LINES : 0);
    r.base_cost = s_cost[best], r.lane_cost = s_lane[best], r.total = s_total[best];
    row[v] = r;
}

int check_cfg(const av_lane_plan_cfg* c, const char* who) {
    static_assert(sizeof(av_lane_plan_cfg) == 80 && sizeof(av_lane_plan_line) == 48 && sizeof(av_lane_plan_row) == 64, "lane plan layouts");
    AV_REQUIRE(c, AV_EINVAL, "%s: null cfg", who);
    const double d[9] = {c->half_width, c->x_far, c->w_cross[0], c->w_cross[1], c->w_cross[2], c->w_on[0], c->w_on[1], c->w_on[2], c->w_end};
    static const char* const names[9] = {"half_width", "x_far",   "w_cross[0]", "w_cross[1]", "w_cross[2]",
                                         "w_on[0]",    "w_on[1]", "w_on[2]",    "w_end"};
    for (int i = 0; i < 9; ++i) AV_REQUIRE(std::isfinite(d[i]), AV_EINVAL, "%s: cfg %s must be finite", who, names[i]);
    for (int i = 0; i < 2; ++i) AV_REQUIRE(d[i] > 0.0, AV_EINVAL, "%s: cfg %s must be > 0", who, names[i]);
    for (int i = 2; i < 9; ++i) AV_REQUIRE(d[i] >= 0.0, AV_EINVAL, "%s: cfg %s must be >= 0", who, names[i]);
    AV_REQUIRE(c->follow == 0 || c->follow == 1, AV_EINVAL, "%s: cfg follow %d is neither 0 nor 1", who, c->follow);
    return AV_OK;
}

}  // namespace

extern "C" int av_lane_plan_check(const av_lane_plan_cfg* cfg) { return check_cfg(cfg, "av_lane_plan_check"); }

extern "C" int av_lane_plan(av_ctx* ctx, av_stream_t stream, const av_lane_plan_cfg* cfg, int n_vehicles, int n_cand, int n_points,
                            const double* plan_state, const double* waypoints, const double* cost, const av_road_lane_bound* bounds,
                            const av_road_lanes_row* lanes, const av_road_mark* marks, const av_road_marks_row* sides,
                            av_lane_plan_line* lines, double* lane_cost, double* total, int32_t* order, uint32_t* cross, int32_t* delta,
                            av_lane_plan_row* row) {
    static const char* const who = "av_lane_plan";
    if (int rc = check_cfg(cfg, who)) return rc;
    AV_REQUIRE(n_vehicles >= 1 && n_vehicles <= 65535, AV_EINVAL, "%s: n_vehicles %d not in 1..65535", who, n_vehicles);
    AV_REQUIRE(n_cand >= 1 && n_cand <= MAXC, AV_EINVAL, "%s: n_cand %d not in 1..%d", who, n_cand, MAXC);
    AV_REQUIRE(n_points >= 1 && n_points <= MAXN, AV_EINVAL, "%s: n_points %d not in 1..%d", who, n_points, MAXN);
    AV_REQUIRE((marks == nullptr) == (sides == nullptr), AV_EINVAL, "%s: marks and sides are NULL only together", who);
#define LANEPLAN_PTR(x) AV_REQUIRE(x, AV_EINVAL, "%s: null " #x, who)
    LANEPLAN_PTR(plan_state);
    LANEPLAN_PTR(waypoints);
    LANEPLAN_PTR(cost);
    LANEPLAN_PTR(bounds);
    LANEPLAN_PTR(lanes);
    LANEPLAN_PTR(lines);
    LANEPLAN_PTR(lane_cost);
    LANEPLAN_PTR(total);
    LANEPLAN_PTR(order);
    LANEPLAN_PTR(cross);
    LANEPLAN_PTR(delta);
    LANEPLAN_PTR(row);
    LANEPLAN_PTR(ctx);
#undef LANEPLAN_PTR
    hipLaunchKernelGGL(lane_plan_kernel, dim3((unsigned)n_vehicles), dim3(THREADS), 0, as_stream(stream), *cfg, n_cand, n_points,
                       plan_state, waypoints, cost, bounds, lanes, marks, sides, lines, lane_cost, total, order, cross, delta, row);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
