// T3: scene classifier -- road type, conditions and lane count of S camera streams per call.
//
// Reference: SceneClassifier.classify (src/tagging/scene_classifier.py:90-303) and the OpenCV calls it makes:
//   _classify_road_type   :128-202  gray, Canny(50, 150), centre edge density, HoughLinesP(1, pi/180, 100, 100, 10),
//                                   detection counts, BGR2HSV + inRange green ratio, lane presence, normalised scores
//   _analyze_conditions   :231-259  np.mean(gray), Laplacian(CV_64F).var()
//   _estimate_lane_count  :261-280  lane width at the bottom row
//   _smooth_tags          :282-298  majority vote over the last 5 road types
//
// Pipeline per call:
//   scene_prep     clears the pixel sums, writes the Canny thresholds (50, 150) and the full-frame ROI rows
//   scene_front    ONE read of the BGR frame: gray into the lane workspace (view 0), gray sum, HSV green count
//                  (OpenCV's RGB2HSV_b fixed-point arithmetic), sum and sum of squares of the 3x3 Laplacian
//                  (BORDER_REFLECT_101) -- exact integers combined with atomics, so the order does not matter
//   lane chain     av_lane_detect, AV_LANE_GIVEN_GRAY | AV_LANE_PIXELS_ONLY: Canny (Sobel, NMS, union-find hysteresis) of that gray image,
//                  full-frame ROI, row-major edge point list
//   scene_center   edge points inside the centre third (read before the PPHT, which reorders the point list)
//   lane chain     av_lane_detect, AV_LANE_HOUGH_ONLY: the PPHT with the scene's settings into the segment list
//   scene_decide   one thread per stream: line statistics (np.mean in NumPy's pairwise order), scores and rules
#include "common.h"

#include <cmath>

namespace {

constexpr int FT_W = 256, FT_R = 32;        // scene_front tile: 256 columns x 32 rows, one column per thread
constexpr int ST_WORDS = 8;                 // u64 pixel sums per stream: gray, green, lap, lap^2, centre, spare
constexpr int ST_INTS = AV_SCENE_STATE_BYTES / 4;
constexpr int HIST = 5;                     // smoothing_window (:88)

struct SceneWs {
    size_t lane, stats, lstate, poly, pts, info, conf, roi, total;
};

__host__ inline size_t al256(size_t v) { return (v + 255) & ~size_t(255); }

__host__ SceneWs scene_layout(int S, int h, int w, int max_segments) {
    SceneWs L{};
    size_t o = 0;
    L.lane = o, o = al256(o + av_lane_workspace_bytes(S, h, w, max_segments));
    L.stats = o, o = al256(o + (size_t)S * ST_WORDS * 8);
    L.lstate = o, o = al256(o + (size_t)S * 8 * 8);           // lane outputs the scene stage does not read
    L.poly = o, o = al256(o + (size_t)S * 6 * 8);
    L.pts = o, o = al256(o + (size_t)S * 200 * 4);
    L.info = o, o = al256(o + (size_t)S * 8 * 4);
    L.conf = o, o = al256(o + (size_t)S * 2 * 8);
    L.roi = o, o = al256(o + (size_t)h * 2 * 4);
    L.total = o;
    return L;
}

__device__ __forceinline__ int reflect101_once(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p); }

template <typename T>
__device__ __forceinline__ T wave_sum_t(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(256) scene_prep_kernel(int S, int h, int w, unsigned long long* __restrict__ stats,
                                                         double* __restrict__ thr, int* __restrict__ roi) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < S) {
        for (int k = 0; k < ST_WORDS; ++k) stats[(size_t)i * ST_WORDS + k] = 0ull;
        double* t = thr + (size_t)i * 4;
        t[0] = 50.0, t[1] = 150.0, t[2] = 0.0, t[3] = 0.0;          // cv2.Canny(gray, 50, 150)  :143
    }
    if (i < h) roi[2 * i] = 0, roi[2 * i + 1] = w - 1;
}

__global__ void __launch_bounds__(256) scene_front_kernel(const uint8_t* __restrict__ bgr, int h, int w, uint8_t* __restrict__ gray,
                                                          unsigned long long* __restrict__ stats) {
    __shared__ uint8_t g[FT_R + 2][FT_W + 2 + 2];
    __shared__ int sdiv[256], hdiv[256];
    const int s = blockIdx.z, x0 = blockIdx.x * FT_W, y0 = blockIdx.y * FT_R, tid = threadIdx.x;
    // OpenCV RGB2HSV_b tables: round((255 << 12) / v) and round((180 << 12) / (6 d)); no quotient is a tie, so the
    // integer forms (2 n + d) / (2 d) are the rounded values
    sdiv[tid] = tid ? (2 * (255 << 12) + tid) / (2 * tid) : 0;
    hdiv[tid] = tid ? (2 * (30 << 12) + tid) / (2 * tid) : 0;
    __syncthreads();
    const uint8_t* img = bgr + (size_t)s * h * w * 3;
    unsigned gsum = 0, gcnt = 0;
    for (int i = tid; i < (FT_R + 2) * (FT_W + 2); i += 256) {
        const int r = i / (FT_W + 2), c = i - r * (FT_W + 2);
        const int yi = y0 + r - 1, xi = x0 + c - 1;              // rows -1 .. h and columns -1 .. w are needed
        if (yi > h || xi > w) continue;
        const int yy = reflect101_once(yi, h), xx = reflect101_once(xi, w);
        const uint8_t* p = img + ((size_t)yy * w + xx) * 3;
        const int b = p[0], gg = p[1], rr = p[2];
        const int gy = (1868 * b + 9617 * gg + 4899 * rr + 8192) >> 14;     // COLOR_BGR2GRAY
        g[r][c] = (uint8_t)gy;
        if (r >= 1 && r <= FT_R && c >= 1 && c <= FT_W && yi < h && xi < w) {
            gray[((size_t)s * h + yi) * w + xi] = (uint8_t)gy;
            gsum += (unsigned)gy;
            const int v = max(b, max(gg, rr)), vmin = min(b, min(gg, rr));
            const int diff = v - vmin;
            const int vr = v == rr ? -1 : 0, vg = v == gg ? -1 : 0;
            const int sat = (diff * sdiv[v] + (1 << 11)) >> 12;
            int hue = (vr & (gg - b)) + (~vr & ((vg & (b - rr + 2 * diff)) + ((~vg) & (rr - gg + 4 * diff))));
            hue = (hue * hdiv[diff] + (1 << 11)) >> 12;
            hue += hue < 0 ? 180 : 0;
            gcnt += (hue >= 35 && hue <= 85 && sat >= 40 && v >= 40) ? 1u : 0u;   // inRange((35,40,40), (85,255,255))
        }
    }
    __syncthreads();
    long long lsum = 0;
    unsigned long long lsq = 0;
    const int c = tid + 1, xi = x0 + tid;
    if (xi < w) {
        for (int r = 1; r <= FT_R && y0 + r - 1 < h; ++r) {
            const int l = (int)g[r - 1][c] + (int)g[r + 1][c] + (int)g[r][c - 1] + (int)g[r][c + 1] - 4 * (int)g[r][c];
            lsum += l;
            lsq += (unsigned long long)(l * l);
        }
    }
    const unsigned long long a = wave_sum_t<unsigned long long>(gsum), bq = wave_sum_t<unsigned long long>(gcnt);
    const unsigned long long cl = wave_sum_t<unsigned long long>((unsigned long long)lsum), dq = wave_sum_t<unsigned long long>(lsq);
    if ((tid & 63) == 0) {
        unsigned long long* st = stats + (size_t)s * ST_WORDS;
        atomicAdd(&st[0], a);
        atomicAdd(&st[1], bq);
        atomicAdd(&st[2], cl);                                      // two's complement: the sum of signed terms
        atomicAdd(&st[3], dq);
    }
}

// edge points of the centre region [h//3, 2h//3) x [w//3, 2w//3) (:146-147), from the lane chain's point list (x | y << 16)
__global__ void __launch_bounds__(256) scene_center_kernel(int h, int w, const unsigned* __restrict__ nz_all, const int* __restrict__ npts,
                                                           unsigned long long* __restrict__ stats) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const int n = npts[s];
    const unsigned* nz = nz_all + (size_t)s * h * w;
    const int ya = h / 3, yb = 2 * h / 3, xa = w / 3, xb = 2 * w / 3;
    unsigned cnt = 0;
    for (int i = blockIdx.y * 256 + tid; i < n; i += gridDim.y * 256) {
        const unsigned p = nz[i];
        const int x = (int)(p & 0xffffu), y = (int)(p >> 16);
        cnt += (y >= ya && y < yb && x >= xa && x < xb) ? 1u : 0u;
    }
    const unsigned long long t = wave_sum_t<unsigned long long>(cnt);
    if ((tid & 63) == 0 && t) atomicAdd(&stats[(size_t)s * ST_WORDS + 4], t);
}

__device__ __forceinline__ double seg_len(const int* sg, int i) {
    const int dx = sg[4 * i + 2] - sg[4 * i], dy = sg[4 * i + 3] - sg[4 * i + 1];
    return sqrt((double)(dx * dx + dy * dy));                      // np.sqrt of the int32 sum of squares  :155
}

// numpy's pairwise_sum over n <= 128 values: < 8 in order; else 8 running partial sums, combined as a tree, then the tail
__device__ double pw_leaf(const int* sg, int lo, int n) {
    if (n < 8) {
        double res = -0.0;
        for (int i = 0; i < n; ++i) res += seg_len(sg, lo + i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = seg_len(sg, lo + j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += seg_len(sg, lo + i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += seg_len(sg, lo + i);
    return res;
}

// np.add.reduce of the n line lengths: pairwise_sum(a, n) = pw(a, n2) + pw(a + n2, n - n2), n2 = n / 2 rounded down to a
// multiple of 8, down to blocks of <= 128 (the recursion, unrolled onto an explicit stack)
__device__ double pw_sum(const int* sg, int n) {
    int lo_[32], n_[32], st_[32];
    double acc_[32];
    int sp = 0;
    lo_[0] = 0, n_[0] = n, st_[0] = 0;
    for (;;) {
        const int lo = lo_[sp], m = n_[sp];
        if (m > 128) {
            int m2 = m / 2;
            m2 -= m2 % 8;
            st_[sp] = 0;
            ++sp;
            lo_[sp] = lo, n_[sp] = m2, st_[sp] = 0;
            continue;
        }
        double ret = pw_leaf(sg, lo, m);
        for (;;) {
            if (sp == 0) return ret;
            --sp;
            if (st_[sp] == 0) {                                    // left half done: keep it, evaluate the right half
                acc_[sp] = ret, st_[sp] = 1;
                int m2 = n_[sp] / 2;
                m2 -= m2 % 8;
                const int plo = lo_[sp], pn = n_[sp];
                ++sp;
                lo_[sp] = plo + m2, n_[sp] = pn - m2, st_[sp] = 0;
                break;
            }
            ret = acc_[sp] + ret;
        }
    }
}

__global__ void __launch_bounds__(64) scene_decide_kernel(int S, int h, int w, int cap, const unsigned long long* __restrict__ stats,
                                                          const int* __restrict__ segs, const int* __restrict__ nseg,
                                                          const int* __restrict__ det_n, const int* __restrict__ det_cls, int max_det,
                                                          const uint8_t* __restrict__ cat, int n_cat, const double* __restrict__ speed,
                                                          const double* __restrict__ lanes, const int* __restrict__ lane_info,
                                                          const double* __restrict__ lane_poly, int* __restrict__ state,
                                                          av_scene_row* __restrict__ rows) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const unsigned long long* st = stats + (size_t)s * ST_WORDS;
    av_scene_row o;
    memset(&o, 0, sizeof(o));
    o.gray_sum = st[0], o.green_count = st[1], o.lap_sum = (long long)st[2], o.lap_sumsq = st[3];
    o.center_count = (int)st[4];
    const unsigned long long n = (unsigned long long)h * (unsigned long long)w;
    const double nd = (double)n;
    o.mean = (double)o.gray_sum / nd;                                // np.mean(gray): exact float64 sum / size   :236
    o.green_ratio = (double)o.green_count / nd;                      // :185
    const long long csize = (long long)(2 * h / 3 - h / 3) * (long long)(2 * w / 3 - w / 3);
    o.center_density = (double)o.center_count / (double)csize;      // :147
    {
        // variance from the exact sums: (n * sum(x^2) - sum(x)^2) / n^2, the numerator in 128 bits
        const unsigned long long m = n, q = o.lap_sumsq;
        const unsigned long long c = (unsigned long long)(o.lap_sum < 0 ? -o.lap_sum : o.lap_sum);
        const unsigned long long lo1 = m * q, hi1 = __umul64hi(m, q), lo2 = c * c, hi2 = __umul64hi(c, c);
        const unsigned long long lo = lo1 - lo2, hi = hi1 - hi2 - (lo1 < lo2 ? 1ull : 0ull);
        o.lap_var = ((double)hi * 18446744073709551616.0 + (double)lo) / (nd * nd);
    }
    // ---- road type (:128-202) --------------------------------------------------------------------------------------
    const int ns = nseg[s];
    o.overflow = ns >= cap ? 1 : 0;
    const int nl = ns < cap ? ns : cap;
    o.n_lines = nl;
    const int* sg = segs + (size_t)s * cap * 4;
    o.avg_length = nl > 0 ? pw_sum(sg, nl) / (double)nl : 0.0;
    double sc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                 // RoadType order
    if (o.center_density > 0.15) sc[1] += 0.4;
    if (nl > 5 && o.avg_length > 150.0) sc[2] += 0.5;
    int nd_ = det_n ? det_n[s] : 0;
    if (nd_ > max_det) nd_ = max_det;
    int n_traffic = 0, n_vehicle = 0, n_ped = 0;
    for (int k = 0; k < nd_; ++k) {
        const int cl = det_cls[(size_t)s * max_det + k];
        const int cb = (cl >= 0 && cl < n_cat) ? cat[cl] : 0;
        n_traffic += (cb & AV_SCENE_CAT_TRAFFIC) ? 1 : 0;
        n_vehicle += (cb & AV_SCENE_CAT_VEHICLE) ? 1 : 0;
        n_ped += (cb & AV_SCENE_CAT_PEDESTRIAN) ? 1 : 0;
    }
    if (nd_ > 0) {                                                   // `if detections:`  :164
        if (n_traffic > 0) sc[1] += 0.3, sc[3] += 0.2;
        if (n_vehicle > 3) sc[3] += 0.3, sc[2] += 0.2;
        else if (n_vehicle <= 1) sc[4] += 0.3;
        o.n_traffic = n_traffic;
        o.has_pedestrian = n_ped > 0 ? 1 : 0;
    }
    if (o.green_ratio > 0.15) sc[4] += 0.3;
    int mode = 0;
    double lx = 0.0, rx = 0.0;
    if (lane_info) {
        const int* li = lane_info + (size_t)s * 8;
        mode = (li[0] && li[1]) ? 2 : 1;
        const double* pp = lane_poly + (size_t)s * 6, y = (double)h;
        lx = (pp[0] * y + pp[1]) * y + pp[2];
        rx = (pp[3] * y + pp[4]) * y + pp[5];
    } else if (lanes) {
        const double* ln = lanes + (size_t)s * 4;
        mode = (int)ln[0], lx = ln[1], rx = ln[2];
    }
    if (mode == 2) sc[2] += 0.2, sc[3] += 0.1;
    double total = 0.0;
    for (int k = 0; k < 6; ++k) total += sc[k];
    total += 0.001;
    int best = 0;
    for (int k = 0; k < 6; ++k) {
        o.scores[k] = sc[k] / total;
        if (o.scores[k] > o.scores[best]) best = k;                  // max(): the first of equal scores
    }
    double conf = o.scores[best];
    if (conf < 0.3) best = 3, conf = 0.3;                            // URBAN  :198-200
    o.road_type_raw = best, o.confidence = conf;
    // ---- conditions (:231-259) -------------------------------------------------------------------------------------
    int nc = 0;
    if (o.mean < 60.0) o.conditions[nc] = 2, o.condition_conf[nc++] = 0.8;
    else if (o.mean > 120.0) o.conditions[nc] = 3, o.condition_conf[nc++] = 0.8;
    else o.conditions[nc] = 3, o.condition_conf[nc++] = 0.5;
    if (speed) {
        const double v = speed[s];
        if (v < 2.0) o.conditions[nc] = 1, o.condition_conf[nc++] = 0.7;
        else if (v > 15.0) o.conditions[nc] = 0, o.condition_conf[nc++] = 0.7;
    }
    if (o.lap_var < 100.0) o.conditions[nc] = 5, o.condition_conf[nc++] = 0.3;
    o.n_conditions = nc;
    // ---- lane count (:261-280) -------------------------------------------------------------------------------------
    if (mode == 1) o.lane_count = 2;
    else if (mode == 2) {
        const double lw = fabs(rx - lx);
        o.lane_count = lw > 200.0 ? 3 : (lw > 100.0 ? 2 : 1);
    }
    // ---- history and vote (:116-125, :282-298) ---------------------------------------------------------------------
    int* sv = state + (size_t)s * ST_INTS;
    const int fc = sv[0];
    int len = sv[1];
    int hist[HIST];
    for (int k = 0; k < HIST; ++k) hist[k] = sv[2 + k];
    if (len < HIST) hist[len++] = best;
    else {
        for (int k = 0; k + 1 < HIST; ++k) hist[k] = hist[k + 1];
        hist[HIST - 1] = best;
    }
    int cur = best;
    if (len >= 2) {
        int cnt[6] = {0, 0, 0, 0, 0, 0}, first[6] = {HIST, HIST, HIST, HIST, HIST, HIST};
        for (int k = 0; k < len; ++k) {
            ++cnt[hist[k]];
            if (first[hist[k]] == HIST) first[hist[k]] = k;
        }
        int win = hist[0];                                           // dict order = first appearance; max() keeps the first
        for (int t = 0; t < 6; ++t)
            if (cnt[t] > cnt[win] || (cnt[t] == cnt[win] && cnt[t] > 0 && first[t] < first[win])) win = t;
        if (cnt[win] > len / 2) cur = win;
    }
    hist[len - 1] = cur;                                             // _smooth_tags mutates the object already in history
    sv[0] = fc + 1, sv[1] = len;
    for (int k = 0; k < HIST; ++k) sv[2 + k] = hist[k];
    o.road_type = cur;
    o.timestamp = (double)fc / 30.0;                                 // :109
    o.frame_count = fc;
    o.history_len = len;
    for (int k = 0; k < HIST; ++k) o.history[k] = k < len ? hist[k] : -1;
    rows[s] = o;
}

}  // namespace

extern "C" {

size_t av_scene_state_bytes(int n_streams) { return n_streams > 0 ? (size_t)n_streams * AV_SCENE_STATE_BYTES : 0; }

int av_scene_reset(av_ctx* ctx, av_stream_t stream, int n_streams, void* state) {
    AV_REQUIRE(ctx && state && n_streams > 0, AV_EINVAL, "av_scene_reset: bad argument");
    AV_HIP(hipMemsetAsync(state, 0, av_scene_state_bytes(n_streams), as_stream(stream)));
    return AV_OK;
}

size_t av_scene_workspace_bytes(int n_streams, int h, int w, int max_segments) {
    if (n_streams <= 0 || h <= 0 || w <= 0 || max_segments <= 0) return 0;
    return scene_layout(n_streams, h, w, max_segments).total;
}

int av_scene_workspace_init(av_ctx* ctx, av_stream_t stream, int n_streams, int h, int w, int max_segments, void* workspace) {
    AV_REQUIRE(ctx && workspace && n_streams > 0 && h > 0 && w > 0 && max_segments > 0, AV_EINVAL,
               "av_scene_workspace_init: bad argument");
    AV_HIP(hipMemsetAsync(workspace, 0, scene_layout(n_streams, h, w, max_segments).total, as_stream(stream)));
    return AV_OK;
}

int av_scene_classify(av_ctx* ctx, av_stream_t stream, int n_streams, int h, int w, const uint8_t* bgr, void* workspace,
                      int max_segments, const int32_t* det_n, const int32_t* det_cls, int max_det, const uint8_t* cat, int n_cat,
                      const double* speed, const double* lanes, const int32_t* lane_info, const double* lane_poly, void* state,
                      av_scene_row* rows) {
    AV_REQUIRE(ctx && bgr && workspace && state && rows, AV_EINVAL, "av_scene_classify: null argument");
    AV_REQUIRE(n_streams > 0 && h >= 8 && w >= 8 && h < 32768 && w < 32768, AV_EINVAL, "av_scene_classify: bad frame size %dx%d", w, h);
    AV_REQUIRE(max_segments > 0, AV_EINVAL, "av_scene_classify: bad segment capacity");
    AV_REQUIRE(!det_n || (det_cls && max_det > 0 && (cat || n_cat == 0) && n_cat >= 0), AV_EINVAL,
               "av_scene_classify: detections need det_cls, max_det and the category table");
    AV_REQUIRE(!lane_info || lane_poly, AV_EINVAL, "av_scene_classify: lane_info needs lane_poly");
    hipStream_t st = as_stream(stream);
    const SceneWs L = scene_layout(n_streams, h, w, max_segments);
    unsigned char* ws = (unsigned char*)workspace;
    unsigned char* lws = ws + L.lane;
    size_t off_gray, off_thr, off_nz, off_npts, off_segs, off_nseg, nb;
    int rc;
    if ((rc = av_lane_workspace_view(AV_LANE_VIEW_BLUR, n_streams, h, w, max_segments, &off_gray, &nb)) ||
        (rc = av_lane_workspace_view(AV_LANE_VIEW_THRESHOLDS, n_streams, h, w, max_segments, &off_thr, &nb)) ||
        (rc = av_lane_workspace_view(AV_LANE_VIEW_POINTS, n_streams, h, w, max_segments, &off_nz, &nb)) ||
        (rc = av_lane_workspace_view(AV_LANE_VIEW_NPOINTS, n_streams, h, w, max_segments, &off_npts, &nb)) ||
        (rc = av_lane_workspace_view(AV_LANE_VIEW_SEGMENTS, n_streams, h, w, max_segments, &off_segs, &nb)) ||
        (rc = av_lane_workspace_view(AV_LANE_VIEW_NSEG, n_streams, h, w, max_segments, &off_nseg, &nb)))
        return rc;
    unsigned long long* stats = (unsigned long long*)(ws + L.stats);
    int* roi = (int*)(ws + L.roi);
    const int np = n_streams > h ? n_streams : h;
    hipLaunchKernelGGL(scene_prep_kernel, dim3((np + 255) / 256), dim3(256), 0, st, n_streams, h, w, stats, (double*)(lws + off_thr), roi);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(scene_front_kernel, dim3((w + FT_W - 1) / FT_W, (h + FT_R - 1) / FT_R, n_streams), dim3(256), 0, st, bgr, h, w,
                       lws + off_gray, stats);
    AV_LAUNCH_CHECK();
    const av_lane_cfg lc{100, 100, 10, max_segments, 0.7};           // HoughLinesP(edges, 1, pi/180, 100, 100, 10)  :151
    double* lstate = (double*)(ws + L.lstate);
    double* poly = (double*)(ws + L.poly);
    int32_t* pts = (int32_t*)(ws + L.pts);
    int32_t* info = (int32_t*)(ws + L.info);
    double* conf = (double*)(ws + L.conf);
    if ((rc = av_lane_detect(ctx, stream, &lc, n_streams, h, w, bgr, roi, lws, lstate, poly, pts, info, conf,
                             AV_LANE_GIVEN_GRAY | AV_LANE_PIXELS_ONLY)))
        return rc;
    hipLaunchKernelGGL(scene_center_kernel, dim3(n_streams, 8), dim3(256), 0, st, h, w, (const unsigned*)(lws + off_nz),
                       (const int*)(lws + off_npts), stats);
    AV_LAUNCH_CHECK();
    if ((rc = av_lane_detect(ctx, stream, &lc, n_streams, h, w, bgr, roi, lws, lstate, poly, pts, info, conf, AV_LANE_HOUGH_ONLY)))
        return rc;
    hipLaunchKernelGGL(scene_decide_kernel, dim3((n_streams + 63) / 64), dim3(64), 0, st, n_streams, h, w, max_segments, stats,
                       (const int*)(lws + off_segs), (const int*)(lws + off_nseg), det_n, det_cls, max_det, cat, n_cat, speed, lanes,
                       lane_info, lane_poly, (int*)state, rows);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"
