// The camera half's outputs as the hot half's inputs: av_dets_to_tracker and av_lane_paths.
//
// The YOLO-mode detector leaves float32 boxes, float32 confidences and the model's own class ids (COCO's 80) in HBM, up to 300 per
// frame in confidence-descending order; the tracker takes int32 boxes, float64 confidences and the reference's eight class ids, at
// most 64 per frame.  The reference crosses that gap on the host (ObjectDetector._detect_yolo, detector.py:103-123:
// x1, y1, x2, y2 = map(int, box.xyxy[0]), conf = float(box.conf[0]), cls = int(box.cls[0])).  av_dets_to_tracker does it on the
// device and adds the class table the reference leaves to the model file: an entry whose class has no reference id is skipped.
//
// The lane detector leaves one second-order fit x(y) per side in image coordinates; the planner takes a reference path in its own
// frame and the maneuver tagger a lateral offset in metres (get_lane_center_offset, lane_detector.py:253-272).  av_lane_paths
// samples the centre line between the two fits at the reference's own rows (lane_detector.py:164: from the bottom of the frame up
// to 0.6 h) and places every sample the way av_track_obstacles places a track's centre, with the same av_obstacle_cfg scales, so
// tracks and lanes land in one road plane.  av_lane_paths_ground is the same kernel body with the samples sent through a camera's
// ground-plane homography instead (lane_paths_kernel<VIA>, as obstacles.hip chooses its placement).
//
// Mapping (both, as obstacles.hip): one wave per frame / stream, lane = list entry, rounds of 64; kept entries are compacted in
// list order by ballot + prefix count.  float64 in the operation order include/avhot.h states (-ffp-contract=off: no FMA).
#include "common.h"
#include "ground_dev.h"

#include <cmath>
#include <type_traits>

namespace {

// int(x) of a Python float that fits, saturated where it does not; NaN -> 0 (the float -> int conversion of the hardware, spelled
// out: the C++ conversion is undefined outside the int range)
__device__ __forceinline__ int32_t trunc_sat(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (int32_t)(-2147483647 - 1);
    return (int32_t)x;
}

__global__ void __launch_bounds__(256) dets_to_tracker_kernel(int n_frames, int max_det, const int32_t* __restrict__ src_n,
                                                              const float* __restrict__ src_box, const float* __restrict__ src_conf,
                                                              const int32_t* __restrict__ src_cls,
                                                              const int32_t* __restrict__ class_map, int n_map, int dcap,
                                                              int32_t* __restrict__ det_n, int32_t* __restrict__ det_box,
                                                              int32_t* __restrict__ det_cls, double* __restrict__ det_conf,
                                                              int32_t* __restrict__ dropped) {
    const int lane = threadIdx.x & 63;
    const long long fl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fl >= n_frames) return;
    const size_t f = (size_t)fl;
    int n = src_n[f];
    n = n < 0 ? 0 : (n > max_det ? max_det : n);
    const size_t in0 = f * (size_t)max_det, out0 = f * (size_t)dcap;
    int count = 0;                                                  // kept entries of the rounds before this one
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        bool keep = false;
        int cls = 0;
        if (i < n) {
            cls = src_cls[in0 + i];
            if (class_map) {
                const int m = (cls >= 0 && cls < n_map) ? class_map[cls] : -1;
                keep = m >= 0;
                cls = m;
            } else {
                keep = true;
            }
        }
        const unsigned long long m = __ballot(keep);
        const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < dcap) {                                   // pos < dcap: inside this frame's rows
            const float* sb = src_box + (in0 + i) * 4;
            int32_t* ob = det_box + (out0 + pos) * 4;
            ob[0] = trunc_sat(sb[0]), ob[1] = trunc_sat(sb[1]), ob[2] = trunc_sat(sb[2]), ob[3] = trunc_sat(sb[3]);
            det_cls[out0 + pos] = cls;
            det_conf[out0 + pos] = (double)src_conf[in0 + i];
        }
        count += __popcll(m);
    }
    if (lane == 0) {
        const int kept = count < dcap ? count : dcap;
        det_n[f] = kept;
        if (dropped) dropped[f] = count - kept;
    }
}

// One wave per stream, lane = sample.  VIA says how a sample (xc, y) of the centre line becomes (lateral, forward) metres:
// av_obstacle_cfg, the linear scales of av_track_obstacles; or const av_ground_cfg*, the ground-plane homography of the stream's
// camera, where the path is cut at the first sample that leaves the road (horizon, range).
template <typename VIA>
__global__ void __launch_bounds__(256) lane_paths_kernel(VIA via, int n_streams, int h, int w, int n_points,
                                                         const double* __restrict__ poly, const int32_t* __restrict__ pts,
                                                         const int32_t* __restrict__ info, const double* __restrict__ plan_state,
                                                         int ref_stride, int rcap, double* __restrict__ ref_path,
                                                         int32_t* __restrict__ n_ref, double* __restrict__ lane_offset) {
    constexpr bool GROUND = std::is_same<VIA, const av_ground_cfg*>::value;
    const int lane = threadIdx.x & 63;
    const long long sl = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sl >= n_streams) return;
    const size_t s = (size_t)sl;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool valid = info[s * 8] != 0 && info[s * 8 + 1] != 0;
    if (!valid) {
        if (lane == 0) {
            n_ref[s] = 0;
            if (lane_offset) lane_offset[s] = nan;
        }
        return;
    }
    if (lane == 0 && lane_offset) {
        const int32_t* p = pts + s * 200;                           // [2][50][2]: x of point 49 of either side
        const long long sum = (long long)p[49 * 2] + (long long)p[100 + 49 * 2];
        if constexpr (GROUND) {
            const grounddev::RoadPoint a = grounddev::project(via[s].g, via[s].max_range, (double)w / 2.0, (double)h);
            const grounddev::RoadPoint b = grounddev::project(via[s].g, via[s].max_range, (double)sum / 2.0, (double)h);
            lane_offset[s] = (a.on_road && b.on_road) ? a.l - b.l : nan;
        } else {
            lane_offset[s] = ((double)w / 2.0 - (double)sum / 2.0) * via.x_scale;
        }
    }
    const double* pl = poly + s * 6;
    const double step = (0.4 * (double)h) / (double)(n_points - 1);
    const double y = (double)h - (double)lane * step;
    const double xl = (pl[0] * y + pl[1]) * y + pl[2];
    const double xr = (pl[3] * y + pl[4]) * y + pl[5];
    const double xc = (xl + xr) / 2.0;
    double l, fw;
    int m = n_points;
    if constexpr (GROUND) {
        const grounddev::RoadPoint q = grounddev::project(via[s].g, via[s].max_range, xc, y);
        // the longest prefix of samples that are all on the road: the lanes below the first that is not (every lane votes)
        const unsigned long long bad = __ballot(lane < n_points && !q.on_road);
        m = bad ? __ffsll((long long)bad) - 1 : n_points;
        m = m >= 2 ? m : 0;
        l = q.l, fw = q.f;
    } else {
        l = (xc - via.x_center) * via.x_scale, fw = via.y_far - y * via.y_scale;
    }
    if (lane == 0) n_ref[s] = m;
    if (lane >= m) return;
    const double* st = plan_state + s * (size_t)ref_stride * 4;     // the first frame of the stream's window
    const double x0 = st[0], y0 = st[1], hd = st[2];
    double sn, cs, s2, c2;
    sincos(hd, &sn, &cs);
    sincos(hd + 1.5707963267948966, &s2, &c2);                      // heading + np.pi/2  (motion_planner.py:179)
    double* o = ref_path + (s * (size_t)rcap + lane) * 2;           // lane < m <= n_points <= rcap
    o[0] = (x0 + fw * cs) + l * c2;
    o[1] = (y0 + fw * sn) + l * s2;
}

// `given` is the caller's pointer: the scales are host memory and go to the kernel by value, the ground table is on the device
inline av_obstacle_cfg kernel_arg(const av_obstacle_cfg* cfg) { return *cfg; }
inline const av_ground_cfg* kernel_arg(const av_ground_cfg* ground) { return ground; }

template <typename GIVEN>
int lane_paths_launch(const char* who, av_ctx* ctx, av_stream_t stream, const GIVEN* given, int n_streams, int h, int w, int n_points,
                      const double* poly, const int32_t* pts, const int32_t* info, const double* plan_state, int ref_stride, int rcap,
                      double* ref_path, int32_t* n_ref, double* lane_offset) {
    AV_REQUIRE(ctx && given && poly && pts && info && plan_state && ref_path && n_ref, AV_EINVAL, "%s: null argument", who);
    AV_REQUIRE(n_streams > 0 && h > 0 && w > 0 && ref_stride > 0, AV_EINVAL, "%s: n_streams, h, w and ref_stride must be > 0", who);
    AV_REQUIRE(n_points >= 2 && n_points <= 64 && n_points <= rcap, AV_EINVAL,
               "%s: n_points %d not in [2, min(64, rcap %d)] (one wave per stream)", who, n_points, rcap);
    using VIA = decltype(kernel_arg(given));
    hipLaunchKernelGGL(lane_paths_kernel<VIA>, dim3((n_streams + 3) / 4), dim3(256), 0, as_stream(stream), kernel_arg(given), n_streams,
                       h, w, n_points, poly, pts, info, plan_state, ref_stride, rcap, ref_path, n_ref, lane_offset);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // namespace

extern "C" int av_dets_to_tracker(av_ctx* ctx, av_stream_t stream, int n_frames, int max_det, const int32_t* src_n,
                                  const float* src_box, const float* src_conf, const int32_t* src_cls, const int32_t* class_map,
                                  int n_map, int dcap, int32_t* det_n, int32_t* det_box, int32_t* det_cls, double* det_conf,
                                  int32_t* dropped) {
    AV_REQUIRE(ctx && src_n && src_box && src_conf && src_cls && det_n && det_box && det_cls && det_conf, AV_EINVAL,
               "av_dets_to_tracker: null argument");
    AV_REQUIRE(n_frames > 0 && max_det >= 1, AV_EINVAL, "av_dets_to_tracker: n_frames and max_det must be > 0");
    AV_REQUIRE(dcap >= 1 && dcap <= 64, AV_EINVAL, "av_dets_to_tracker: dcap %d not in [1,64] (the tracker's limit)", dcap);
    hipLaunchKernelGGL(dets_to_tracker_kernel, dim3((n_frames + 3) / 4), dim3(256), 0, as_stream(stream), n_frames, max_det, src_n,
                       src_box, src_conf, src_cls, class_map, n_map, dcap, det_n, det_box, det_cls, det_conf, dropped);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_lane_paths(av_ctx* ctx, av_stream_t stream, const av_obstacle_cfg* cfg, int n_streams, int h, int w, int n_points,
                             const double* poly, const int32_t* pts, const int32_t* info, const double* plan_state, int ref_stride,
                             int rcap, double* ref_path, int32_t* n_ref, double* lane_offset) {
    return lane_paths_launch("av_lane_paths", ctx, stream, cfg, n_streams, h, w, n_points, poly, pts, info, plan_state, ref_stride, rcap,
                             ref_path, n_ref, lane_offset);
}

extern "C" int av_lane_paths_ground(av_ctx* ctx, av_stream_t stream, const av_ground_cfg* ground, int n_streams, int h, int w,
                                    int n_points, const double* poly, const int32_t* pts, const int32_t* info, const double* plan_state,
                                    int ref_stride, int rcap, double* ref_path, int32_t* n_ref, double* lane_offset) {
    return lane_paths_launch("av_lane_paths_ground", ctx, stream, ground, n_streams, h, w, n_points, poly, pts, info, plan_state,
                             ref_stride, rcap, ref_path, n_ref, lane_offset);
}
