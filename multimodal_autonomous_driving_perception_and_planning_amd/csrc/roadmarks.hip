// Road marks: what each lane boundary is -- solid or dashed, white or yellow -- read from the rig's rectified frames along the
// boundaries av_road_lanes found (av_road_marks, include/avhot.h).
//
// Two launches.  road_marks_kernel: one workgroup per (vehicle, boundary), one thread per sample, in rounds of blockDim samples (two
// above 256).  A vehicle's mounts and ground entries and the boundary's polynomial are the same for the whole workgroup: scalar
// loads.  A thread asks every camera whether it sees the sample's two end taps, keeps the nearest such camera, and reads the core
// and shoulder taps there through ground_dev.h's position rule and bilinear sample, the ones av_rig_surround uses.  The seen and
// paint bits go by ballot into LDS as 64-bit words, the colour and contrast sums by a wave sum and one LDS atomic per wave
// (integers: the order does not matter).  Then wave 0 analyses the runs on the words: lane l looks at sample 64 w + l of every
// word w -- a paint run starts there or not -- and finds the run's end, the gap before it and whether both are measured with
// count-leading/trailing-zero scans over the words; the counts meet in a wave sum.  road_marks_sides_kernel: one thread per
// vehicle carries the two sides of the ego lane from frame to frame.  Nothing waits for another workgroup.
#include "common.h"
#include "ground_dev.h"

#include <cmath>

namespace {

constexpr int MAX_CAMS = 8, MAX_SIDE = 32768, MAXB = AV_ROAD_LANES_MAX_BOUNDS, MAXS = AV_ROAD_MARKS_MAX_SAMPLES, WORDS = MAXS / 64;
constexpr int MAX_COUNT = 65536, RUN_CAP = 1 << 30;

// the settings as the device takes them: the lengths as sample counts (the header's count())
struct MarksParams {
    double x_near, ds, dl;
    int n_samples, core, shoulder0, shoulder1, contrast, yellow_tenths, hold, forget;
    int gap_solid_n, gap_dash_n, min_seen_n, min_paint_n;
};

typedef unsigned long long u64;

// the highest index below i (0 <= i < WORDS * 64) whose bit of w equals `set`, -1 without one
__device__ __forceinline__ int prev_bit(const u64* w, int i, bool set) {
    u64 m = (1ull << (i & 63)) - 1ull;                                  // the bits below i's in its own word
    for (int wi = i >> 6; wi >= 0; --wi) {
        const u64 x = (set ? w[wi] : ~w[wi]) & m;
        if (x) return wi * 64 + 63 - __clzll((long long)x);
        m = ~0ull;
    }
    return -1;
}
// the lowest index above i whose bit of w is clear, WORDS * 64 without one
__device__ __forceinline__ int next_clear(const u64* w, int i) {
    u64 m = (i & 63) == 63 ? 0ull : (~0ull << ((i & 63) + 1));
    for (int wi = i >> 6; wi < WORDS; ++wi) {
        const u64 x = ~w[wi] & m;
        if (x) return wi * 64 + __ffsll((unsigned long long)x) - 1;
        m = ~0ull;
    }
    return WORDS * 64;
}
__device__ __forceinline__ bool bit_at(const u64* w, int i) { return (w[i >> 6] >> (i & 63)) & 1ull; }

struct Tap {
    double f, l;
};
// a vehicle-frame road point in the camera's road frame: av_rig_surround's order
__device__ __forceinline__ Tap to_camera(const av_rig_mount& m, double X, double Y) {
    const double dx = X - m.x, dy = Y - m.y;
    Tap t;
    t.f = m.c * dx + m.s * dy, t.l = m.c * dy - m.s * dx;
    return t;
}

template <bool WIDE>
__global__ void __launch_bounds__(256) road_marks_kernel(MarksParams p, int n_cams, const av_rig_mount* __restrict__ mounts,
                                                         const av_ground_cfg* __restrict__ ground, int h, int w,
                                                         const uint8_t* __restrict__ bgr, const av_road_lane_bound* __restrict__ bounds,
                                                         const av_road_lanes_row* __restrict__ lanes, av_road_mark* __restrict__ marks,
                                                         uint32_t* __restrict__ profile) {
    __shared__ u64 seen_w[WORDS], paint_w[WORDS];
    __shared__ unsigned sums[5];                                         // b, g, r, contrast, views
    const int b = blockIdx.x, v = blockIdx.y, tid = threadIdx.x;
    av_road_mark* const out = marks + (size_t)v * MAXB + b;
    uint32_t* const prof = profile ? profile + ((size_t)v * MAXB + b) * 2 * (MAXS / 32) : nullptr;
    const int nb = min(max(lanes[v].n_bounds, 0), MAXB);
    if (b >= nb) {                                                       // a dead boundary: zero rows (the same for the whole workgroup)
        if (tid < 16) reinterpret_cast<uint32_t*>(out)[tid] = 0u;
        if (prof && tid < 2 * (MAXS / 32)) prof[tid] = 0u;
        return;
    }
    if (tid < WORDS) seen_w[tid] = 0ull, paint_w[tid] = 0ull;
    if (tid < 5) sums[tid] = 0u;
    __syncthreads();
    const av_road_lane_bound bd = bounds[(size_t)v * MAXB + b];
    const size_t frame = (size_t)h * w * 3, cam0 = (size_t)v * n_cams;
    unsigned my_b = 0, my_g = 0, my_r = 0, my_c = 0, my_views = 0;
    for (int base = 0; base < p.n_samples; base += (int)blockDim.x) {    // blockDim is a multiple of 64: a wave's samples are one word
        const int i = base + tid;
        bool seen = false, paint = false;
        if (i < p.n_samples) {
            const double X = p.x_near + ((double)i + 0.5) * p.ds;
            const double Yc = (bd.a0 + bd.a1 * X) + bd.a2 * (X * X);
            const double Ya = Yc + (double)(-p.shoulder1) * p.dl, Yb = Yc + (double)p.shoulder1 * p.dl;
            int best_k = -1;
            double best = 0.0;
            for (int k = 0; k < n_cams; ++k) {
                const av_rig_mount m = mounts[cam0 + k];                 // the same for the whole workgroup: scalar loads
                const av_ground_cfg& g = ground[cam0 + k];
                const double max_range = g.max_range;
                const Tap ta = to_camera(m, X, Ya), tb = to_camera(m, X, Yb);
                if (!(ta.f >= 0.0 && ta.f <= max_range && tb.f >= 0.0 && tb.f <= max_range)) continue;
                long long iu, iv;
                if (!grounddev::warp_position(g.ginv, h, w, ta.f, ta.l, iu, iv)) continue;
                if (!grounddev::warp_position(g.ginv, h, w, tb.f, tb.l, iu, iv)) continue;
                const Tap tc = to_camera(m, X, Yc + 0.0 * p.dl);        // tap j = 0, in the taps' own form
                const double d2 = tc.f * tc.f + tc.l * tc.l;
                if (best_k < 0 || d2 < best) best = d2, best_k = k;     // equal d2: the smaller k stays
            }
            seen = best_k >= 0 && X >= bd.x_min && X <= bd.x_max;
            if (seen) {
                // the nearest camera differs from lane to lane: its mount and ginv in registers
                const av_rig_mount m = mounts[cam0 + best_k];
                double q[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) q[e] = ground[cam0 + best_k].ginv[e];
                const uint8_t* src = bgr + (cam0 + best_k) * frame;
                int peak = -1;
                unsigned peak_px = 0, shoulder = 0;
                for (int j = -p.shoulder1; j <= p.shoulder1; ++j) {
                    const int aj = j < 0 ? -j : j;
                    if (aj > p.core && aj < p.shoulder0) continue;      // (the same for the whole workgroup)
                    const Tap t = to_camera(m, X, Yc + (double)j * p.dl);
                    long long iu, iv;
                    unsigned px = 0;                                     // a tap that does not pass reads as black: nothing outside the frame
                    if (grounddev::warp_position(q, h, w, t.f, t.l, iu, iv)) px = grounddev::warp_sample<WIDE>(src, h, w, iu, iv);
                    const int gray = (int)((1868u * (px & 255u) + 9617u * ((px >> 8) & 255u) + 4899u * (px >> 16) + 8192u) >> 14);
                    if (aj <= p.core) {
                        if (gray > peak) peak = gray, peak_px = px;     // equal gray: the smaller j stays
                    } else {
                        shoulder += (unsigned)gray;
                    }
                }
                const int n_sh = 2 * (p.shoulder1 - p.shoulder0 + 1);
                const int bg = (int)((2u * shoulder + (unsigned)n_sh) / (2u * (unsigned)n_sh));
                my_views |= 1u << best_k;
                if (peak - bg >= p.contrast) {
                    paint = true;
                    my_b += peak_px & 255u, my_g += (peak_px >> 8) & 255u, my_r += peak_px >> 16, my_c += (unsigned)(peak - bg);
                }
            }
        }
        const u64 sb = __ballot(seen), pb = __ballot(paint);
        if ((tid & 63) == 0 && base + tid < MAXS) seen_w[(base + tid) >> 6] = sb, paint_w[(base + tid) >> 6] = pb;
    }
    {
        const unsigned sb = (unsigned)wave_sum_i((int)my_b), sg = (unsigned)wave_sum_i((int)my_g), sr = (unsigned)wave_sum_i((int)my_r),
                       sc = (unsigned)wave_sum_i((int)my_c), sv = wave_or_u32(my_views);
        if ((tid & 63) == 0) {
            atomicAdd(&sums[0], sb), atomicAdd(&sums[1], sg), atomicAdd(&sums[2], sr), atomicAdd(&sums[3], sc);
            atomicOr(&sums[4], sv);
        }
    }
    __syncthreads();
    if (prof && tid < 2 * (MAXS / 32)) {
        const u64* src_w = tid < MAXS / 32 ? seen_w : paint_w;
        const int t = tid & (MAXS / 32 - 1);
        prof[tid] = (uint32_t)(src_w[t >> 1] >> (32 * (t & 1)));
    }
    if (tid >= 64) return;
    // ---- the runs, on the words: lane l, word wd -> sample 64 wd + l ----
    int n_seen = 0, n_paint = 0, n_runs = 0, n_gaps = 0, gap_sum = 0, n_dashes = 0, dash_sum = 0;
    unsigned longest = 0;
    for (int wd = 0; wd * 64 < p.n_samples; ++wd) {
        const int i = wd * 64 + tid;
        n_seen += (int)bit_at(seen_w, i), n_paint += (int)bit_at(paint_w, i);
        if (!bit_at(paint_w, i) || (i > 0 && bit_at(paint_w, i - 1))) continue;      // not the first sample of a run
        n_runs += 1;
        const int e = next_clear(paint_w, i);                           // one past the run's last sample; <= n_samples (the bits beyond are clear)
        const bool before = i > 0 && bit_at(seen_w, i - 1), after = e < p.n_samples && bit_at(seen_w, e);
        if (before && after) n_dashes += 1, dash_sum += e - i;
        const int pp = prev_bit(paint_w, i, true);                      // the last sample of the run before this one
        if (pp >= 0 && prev_bit(seen_w, i, false) < pp) {               // a gap, and every sample of it is seen
            const int len = i - 1 - pp;
            n_gaps += 1, gap_sum += len, longest = max(longest, (unsigned)len);
        }
    }
    n_seen = wave_sum_i(n_seen), n_paint = wave_sum_i(n_paint), n_runs = wave_sum_i(n_runs), n_gaps = wave_sum_i(n_gaps);
    gap_sum = wave_sum_i(gap_sum), n_dashes = wave_sum_i(n_dashes), dash_sum = wave_sum_i(dash_sum);
    longest = wave_max_u32(longest);
    if (tid != 0) return;
    av_road_mark mk;
    mk.type = AV_ROAD_MARK_UNKNOWN, mk.colour = 0, mk.flags = 0;
    if (n_seen >= p.min_seen_n && n_paint >= p.min_paint_n) {
        if ((int)longest < p.gap_solid_n) mk.type = AV_ROAD_MARK_SOLID;
        else if (n_runs >= 2 && (int)longest >= p.gap_dash_n) mk.type = AV_ROAD_MARK_DASHED;
        else mk.flags = AV_ROAD_MARK_AMBIGUOUS;
    }
    if (mk.type != AV_ROAD_MARK_UNKNOWN)
        mk.colour = 10u * sums[0] < (unsigned)p.yellow_tenths * min(sums[1], sums[2]) ? AV_ROAD_MARK_YELLOW : AV_ROAD_MARK_WHITE;
    mk.n_seen = n_seen, mk.n_paint = n_paint, mk.n_runs = n_runs, mk.longest_gap = (int)longest, mk.n_gaps = n_gaps, mk.n_dashes = n_dashes;
    mk.contrast = n_paint > 0 ? (int)((2u * sums[3] + (unsigned)n_paint) / (2u * (unsigned)n_paint)) : 0;
    mk.views = (int)sums[4], mk.reserved = 0;
    mk.dash_m = n_dashes > 0 ? ((double)dash_sum / (double)n_dashes) * p.ds : 0.0;
    mk.gap_m = n_gaps > 0 ? ((double)gap_sum / (double)n_gaps) * p.ds : 0.0;
    *out = mk;
}

__device__ __forceinline__ void side_step(av_road_marks_side_state& s, int type, int colour, int hold, int forget) {
    if (type != AV_ROAD_MARK_UNKNOWN) {
        s.since = 0;
        if (type == s.cand_type && colour == s.cand_colour) s.run = min(s.run + 1, RUN_CAP);
        else s.cand_type = type, s.cand_colour = colour, s.run = 1;
        if (s.run >= hold) s.type = s.cand_type, s.colour = s.cand_colour;
    } else {
        s.since = min(s.since + 1, RUN_CAP);
        if (s.since >= forget) s = av_road_marks_side_state{};
    }
}
__device__ __forceinline__ int may_change(int type) {
    return type == AV_ROAD_MARK_DASHED ? 1 : type == AV_ROAD_MARK_SOLID ? 0 : -1;
}

__global__ void __launch_bounds__(64) road_marks_sides_kernel(int n_vehicles, int hold, int forget,
                                                              const av_road_lane_bound* __restrict__ bounds,
                                                              const av_road_lanes_row* __restrict__ lanes,
                                                              const av_road_mark* __restrict__ marks, av_road_marks_state* __restrict__ state,
                                                              av_road_marks_row* __restrict__ sides) {
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= n_vehicles) return;
    av_road_marks_state st = state[v];
    const int status = lanes[v].status, nb = min(max(lanes[v].n_bounds, 0), MAXB);
    if (status & AV_ROAD_CHANGE_LEFT) st.right = st.left, st.left = av_road_marks_side_state{};
    else if (status & AV_ROAD_CHANGE_RIGHT) st.left = st.right, st.right = av_road_marks_side_state{};
    av_road_marks_row row{};
    for (int side = 0; side < 2; ++side) {
        const int flag = side == 0 ? AV_ROAD_BOUND_LEFT : AV_ROAD_BOUND_RIGHT;
        av_road_marks_side_state& s = side == 0 ? st.left : st.right;
        av_road_marks_side& o = side == 0 ? row.left : row.right;
        int bi = -1;
        for (int b = nb - 1; b >= 0; --b)
            if (bounds[(size_t)v * MAXB + b].flags & flag) bi = b;      // the first such boundary
        o.bound = bi, o.observed = AV_ROAD_MARK_UNKNOWN, o.observed_colour = 0;
        if (bi >= 0) o.observed = marks[(size_t)v * MAXB + bi].type, o.observed_colour = marks[(size_t)v * MAXB + bi].colour;
        side_step(s, o.observed, o.observed_colour, hold, forget);
        o.type = s.type, o.colour = s.colour, o.run = s.run;
    }
    st.frames += 1;
    row.may_change_left = may_change(st.left.type), row.may_change_right = may_change(st.right.type);
    state[v] = st;
    sides[v] = row;
}

// the header's count(): false when it falls outside 1 .. 65536
bool count_of(double len, double ds, int* n) {
    const double c = std::floor(len / ds + 0.5);
    if (!(c >= 1.0 && c <= (double)MAX_COUNT)) return false;
    *n = (int)c;
    return true;
}

int check_cfg(const av_road_marks_cfg* c, const char* who, MarksParams* out) {
    static_assert(sizeof(av_road_marks_cfg) == 88 && sizeof(av_road_mark) == 64 && sizeof(av_road_marks_row) == 64 &&
                      sizeof(av_road_marks_state) == 64 && sizeof(av_road_lane_bound) == 64 && sizeof(av_road_lanes_row) == 128,
                  "road marks layouts");
    AV_REQUIRE(c, AV_EINVAL, "%s: null cfg", who);
    const double d[7] = {c->x_near, c->ds, c->dl, c->gap_solid, c->gap_dash, c->min_seen, c->min_paint};
    static const char* const names[7] = {"x_near", "ds", "dl", "gap_solid", "gap_dash", "min_seen", "min_paint"};
    for (int i = 0; i < 7; ++i) AV_REQUIRE(std::isfinite(d[i]), AV_EINVAL, "%s: cfg %s must be finite", who, names[i]);
    for (int i = 1; i < 7; ++i) AV_REQUIRE(d[i] > 0.0, AV_EINVAL, "%s: cfg %s must be > 0", who, names[i]);
    AV_REQUIRE(c->gap_dash >= c->gap_solid, AV_EINVAL, "%s: cfg gap_dash must be >= gap_solid", who);
    MarksParams p;
    int* const counts[4] = {&p.gap_solid_n, &p.gap_dash_n, &p.min_seen_n, &p.min_paint_n};
    for (int i = 0; i < 4; ++i)
        AV_REQUIRE(count_of(d[3 + i], c->ds, counts[i]), AV_EINVAL, "%s: cfg %s is not 1..%d samples of ds", who, names[3 + i], MAX_COUNT);
    AV_REQUIRE(c->n_samples >= 1 && c->n_samples <= MAXS, AV_EINVAL, "%s: cfg n_samples %d not in 1..%d", who, c->n_samples, MAXS);
    AV_REQUIRE(c->core >= 0, AV_EINVAL, "%s: cfg core must be >= 0", who);
    AV_REQUIRE(c->core < c->shoulder0 && c->shoulder0 <= c->shoulder1 && c->shoulder1 <= 16, AV_EINVAL,
               "%s: cfg wants core < shoulder0 <= shoulder1 <= 16", who);
    AV_REQUIRE(c->contrast >= 1 && c->contrast <= 255, AV_EINVAL, "%s: cfg contrast %d not in 1..255", who, c->contrast);
    AV_REQUIRE(c->yellow_tenths >= 0 && c->yellow_tenths <= 10, AV_EINVAL, "%s: cfg yellow_tenths %d not in 0..10", who, c->yellow_tenths);
    AV_REQUIRE(c->hold >= 1, AV_EINVAL, "%s: cfg hold must be >= 1", who);
    AV_REQUIRE(c->forget >= 1, AV_EINVAL, "%s: cfg forget must be >= 1", who);
    p.x_near = c->x_near, p.ds = c->ds, p.dl = c->dl;
    p.n_samples = c->n_samples, p.core = c->core, p.shoulder0 = c->shoulder0, p.shoulder1 = c->shoulder1, p.contrast = c->contrast;
    p.yellow_tenths = c->yellow_tenths, p.hold = c->hold, p.forget = c->forget;
    if (out) *out = p;
    return AV_OK;
}

}  // namespace

extern "C" int av_road_marks_check(const av_road_marks_cfg* cfg) { return check_cfg(cfg, "av_road_marks_check", nullptr); }

extern "C" size_t av_road_marks_state_bytes(void) { return sizeof(av_road_marks_state); }

extern "C" int av_road_marks(av_ctx* ctx, av_stream_t stream, const av_road_marks_cfg* cfg, int n_vehicles, int n_cams,
                             const av_rig_mount* mounts, const av_ground_cfg* ground, int h, int w, const uint8_t* bgr,
                             const av_road_lane_bound* bounds, const av_road_lanes_row* lanes, av_road_marks_state* state,
                             av_road_mark* marks, av_road_marks_row* sides, uint32_t* profile) {
    static const char* const who = "av_road_marks";
    MarksParams p;
    if (int rc = check_cfg(cfg, who, &p)) return rc;
    AV_REQUIRE(n_vehicles >= 1 && n_vehicles <= 65535, AV_EINVAL, "%s: n_vehicles %d not in 1..65535", who, n_vehicles);
    AV_REQUIRE(n_cams >= 1 && n_cams <= MAX_CAMS, AV_EINVAL, "%s: n_cams %d not in 1..%d", who, n_cams, MAX_CAMS);
    AV_REQUIRE(h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE, AV_EINVAL, "%s: frame size h %d, w %d not in 1..%d", who, h, w, MAX_SIDE);
#define ROAD_MARKS_PTR(x) AV_REQUIRE(x, AV_EINVAL, "%s: null " #x, who)
    ROAD_MARKS_PTR(mounts);
    ROAD_MARKS_PTR(ground);
    ROAD_MARKS_PTR(bgr);
    ROAD_MARKS_PTR(bounds);
    ROAD_MARKS_PTR(lanes);
    ROAD_MARKS_PTR(state);
    ROAD_MARKS_PTR(marks);
    ROAD_MARKS_PTR(sides);
    ROAD_MARKS_PTR(ctx);
#undef ROAD_MARKS_PTR
    const unsigned threads = (unsigned)std::min(256, (p.n_samples + 63) / 64 * 64);
    hipLaunchKernelGGL(w >= 2 ? road_marks_kernel<true> : road_marks_kernel<false>, dim3(MAXB, (unsigned)n_vehicles), dim3(threads), 0,
                       as_stream(stream), p, n_cams, mounts, ground, h, w, bgr, bounds, lanes, marks, profile);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(road_marks_sides_kernel, dim3(((unsigned)n_vehicles + 63) / 64), dim3(64), 0, as_stream(stream), n_vehicles, p.hold,
                       p.forget, bounds, lanes, marks, state, sides);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_road_marks_reset(av_ctx* ctx, av_stream_t stream, int n_vehicles, int vehicle, av_road_marks_state* state) {
    AV_REQUIRE(n_vehicles >= 1 && n_vehicles <= 65535, AV_EINVAL, "av_road_marks_reset: n_vehicles %d not in 1..65535", n_vehicles);
    AV_REQUIRE(vehicle >= -1 && vehicle < n_vehicles, AV_EINVAL, "av_road_marks_reset: vehicle %d is neither -1 nor in 0..%d", vehicle,
               n_vehicles - 1);
    AV_REQUIRE(state, AV_EINVAL, "av_road_marks_reset: null state");
    AV_REQUIRE(ctx, AV_EINVAL, "av_road_marks_reset: null ctx");
    if (vehicle < 0) AV_HIP(hipMemsetAsync(state, 0, sizeof(av_road_marks_state) * (size_t)n_vehicles, as_stream(stream)));
    else AV_HIP(hipMemsetAsync(state + vehicle, 0, sizeof(av_road_marks_state), as_stream(stream)));
    return AV_OK;
}
