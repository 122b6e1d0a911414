// K1-K3: batched IoU tracker: the kernels, the launch plan and the entry points.  tracker_body, which every tracker_kernel runs, is in
// tracker_dev.h with the reference, the mapping and the LDS layout.
//
// Host side: av_tracker_update validates, asks tracker_plan for the launch -- chunk length, replica waves or not, trailing wave or not,
// the instantiation (one table of seven), block size, dynamic LDS (tracker_lds_bytes: what the layout takes; what is claimed), wave map
// -- and launches it.  The environment is read in one function, for two test hooks (AVHOT_TRACKER_REP, AVHOT_TRACKER_PIPE).
#include "tracker_dev.h"

#include <mutex>

namespace {

template <bool MULTIWAVE, int DREG, int REP, int PIPE = 0>
__global__ void __launch_bounds__(1024) tracker_kernel(av_tracker_cfg cfg, int n_frames, int dcap, const int32_t* __restrict__ det_n,
                               const int32_t* __restrict__ det_box, const int32_t* __restrict__ det_cls,
                               const double* __restrict__ det_conf, int tcap, unsigned char* __restrict__ state_all,
                               av_track_row* __restrict__ snap, int32_t* __restrict__ snap_n,
                               int32_t* __restrict__ det2trk, int chunk_frames, unsigned long long wave_map) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    tracker_body<MULTIWAVE, DREG, REP, PIPE>(cfg, n_frames, dcap, det_n, det_box, det_cls, det_conf, tcap, state_all, snap, snap_n,
                                              det2trk, chunk_frames, blockIdx.x, smem, wave_map);
}

__global__ void tracker_reset_kernel(int n_streams, size_t bytes_per_stream, unsigned char* state) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    int* hdr = reinterpret_cast<int*>(state + (size_t)s * bytes_per_stream);
    for (int i = 0; i < HDR_INTS; ++i) hdr[i] = 0;
    hdr[1] = 1;     // next_id starts at 1 (multi_object_tracker.py:81)
}

// Every tracker_kernel instantiation there is.  tracker_plan finds its kernel here and nowhere else; lds_raised: the devices on which
// the kernel's dynamic-LDS limit has been raised above the default 64 KB (av_tracker_update).
using TrackerKernel = void (*)(av_tracker_cfg, int, int, const int32_t*, const int32_t*, const int32_t*, const double*, int,
                               unsigned char*, av_track_row*, int32_t*, int32_t*, int, unsigned long long);
struct TrackerInst { bool multiwave; int dreg, rep, pipe; TrackerKernel fn; unsigned long long lds_raised; };
#define AV_TRK_INST(MW, DR, RP, PP) {MW, DR, RP, PP, tracker_kernel<MW, DR, RP, PP>, 0}
TrackerInst tracker_insts[] = {
    AV_TRK_INST(false, 8, 1, 0), AV_TRK_INST(false, 16, 1, 0), AV_TRK_INST(false, 0, 1, 0),     // one wave (tcap 64): dcap <= 8, <= 16, any
    AV_TRK_INST(true, 8, 1, 0),  AV_TRK_INST(true, 0, 1, 0),                                    // a wave per 64 rows: dcap <= 8, any
    AV_TRK_INST(false, 8, 8, 0), AV_TRK_INST(false, 8, 8, 1),                                   // eight column waves; + the trailing wave
};
#undef AV_TRK_INST

// Test hooks, read from the environment on every call (the tests change them between two trackers of one process to pin the replica
// kernel against the one-wave kernel and the trailing wave against the in-place update).  The only environment this file reads.
struct TrackerHooks { bool one_wave; int pipe; };       // pipe: -1 = not set
TrackerHooks read_tracker_hooks() {
    const char* rep_env = getenv("AVHOT_TRACKER_REP");       // <= 1: no replica waves
    const char* pipe_env = getenv("AVHOT_TRACKER_PIPE");     // 0 / non-zero: without / with the trailing wave, whatever the window
    return {rep_env && atoi(rep_env) <= 1, pipe_env ? (atoi(pipe_env) != 0 ? 1 : 0) : -1};
}

// Everything a launch of the tracker is decided by, decided in one place.
struct TrackerPlan {
    int fc, block;                     // frames whose detections are staged in LDS at once; threads per workgroup
    bool replica;                      // eight column waves (REP == 8) ...
    int pipe;                          // ... 1: and the trailing wave
    TrackerInst* inst;
    size_t lds_need, lds_claim;        // dynamic LDS: what the layout takes, what the launch asks for
    unsigned long long wave_map;       // hardware wave -> role, a nibble each
};
TrackerPlan tracker_plan(const av_tracker_cfg& cfg, int n_frames, int dcap, int tcap) {
    const TrackerHooks hk = read_tracker_hooks();
    TrackerPlan p{};
    // chunk of frames whose detections are staged in LDS at once (~16 KB)
    p.fc = (int)(16384 / (4 + (size_t)dcap * (16 + 4 + 8 + 8)));
    p.fc = p.fc < 1 ? 1 : (p.fc > 64 ? 64 : p.fc);
    if (p.fc > n_frames) p.fc = n_frames;
    // replica waves (one per detection column) for the common table size; windows also get the trailing ninth wave
    p.replica = tcap == 64 && dcap <= 8 && cfg.iou_threshold > 0.0 && !hk.one_wave;
    p.pipe = !p.replica ? 0 : (hk.pipe >= 0 ? hk.pipe : (n_frames >= 16 ? 1 : 0));
    const bool multiwave = tcap > 64;
    const int dreg = dcap <= 8 ? 8 : (dcap <= 16 && !multiwave ? 16 : 0), rep = p.replica ? 8 : 1;
    for (TrackerInst& k : tracker_insts)
        if (k.multiwave == multiwave && k.dreg == dreg && k.rep == rep && k.pipe == p.pipe) p.inst = &k;
    p.block = p.replica ? 64 * (8 + p.pipe) : tcap;
    p.lds_need = p.lds_claim = tracker_lds_bytes(tcap, dcap, p.fc, p.replica, p.pipe);
    // A window of frames is a long per-stream latency chain on one CU per stream; whatever else lands on that CU competes
    // with it for issue slots and for the CU's memory pipeline.  In the batched step the HBM-bound planner runs on the
    // other stream: claiming (almost) the whole LDS keeps its workgroups (38 KB each) off the tracker's 64 CUs -- config 4
    // 0.380 -> 0.352 ms per step (100 KB: no change, two planner workgroups still fit; 125 / 150 KB: 0.357 / 0.352).
    // 156 KB also keeps the Kalman kernel's one-wave workgroups (8.4 KB of LDS each) off these CUs: 0.306-0.310 against
    // 0.310-0.313 ms per step.
    if (p.replica && n_frames >= 16 && p.lds_need < (size_t)156 * 1024) p.lds_claim = (size_t)156 * 1024;
    // SIMD of hardware wave h = h % 4.  With the trailing wave: SIMD 0 = column 0 + columns 6, 7; SIMD 1 = the trailing wave +
    // column 3; SIMD 2 = columns 1, 4; SIMD 3 = columns 2, 5 (0.268 -> 0.260 ms per 64 x 256 frames).  Identity otherwise.
    p.wave_map = p.pipe ? 0x754362180ull : 0xFEDCBA9876543210ull;
    return p;
}

}  // namespace

extern "C" {

size_t av_tracker_state_bytes(int tcap, int trajectory_length) {
    if (tcap <= 0 || trajectory_length <= 0) return 0;
    return state_bytes(tcap, trajectory_length);
}

int av_tracker_reset(av_ctx* ctx, av_stream_t stream, int n_streams, int tcap, int trajectory_length, void* state) {
    AV_REQUIRE(ctx && state, AV_EINVAL, "av_tracker_reset: null argument");
    AV_REQUIRE(n_streams > 0 && tcap > 0 && trajectory_length > 0, AV_EINVAL, "av_tracker_reset: bad sizes");
    hipLaunchKernelGGL(tracker_reset_kernel, dim3((n_streams + 63) / 64), dim3(64), 0, as_stream(stream), n_streams,
                       state_bytes(tcap, trajectory_length), (unsigned char*)state);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_tracker_update(av_ctx* ctx, av_stream_t stream, const av_tracker_cfg* cfg, int n_streams, int n_frames,
                      int dcap, const int32_t* det_n, const int32_t* det_box, const int32_t* det_cls,
                      const double* det_conf, int tcap, void* state, av_track_row* snap, int32_t* snap_n,
                      int32_t* det2trk) {
    AV_REQUIRE(ctx && cfg && det_n && det_box && det_cls && det_conf && state, AV_EINVAL,
               "av_tracker_update: null argument");
    AV_REQUIRE(n_streams > 0 && n_frames > 0, AV_EINVAL, "av_tracker_update: n_streams/n_frames must be > 0");
    AV_REQUIRE(tcap >= 64 && tcap <= 1024 && (tcap % 64) == 0, AV_EINVAL,
               "av_tracker_update: tcap %d must be a multiple of 64 in [64,1024]", tcap);
    AV_REQUIRE(dcap >= 1 && dcap <= 64, AV_EINVAL, "av_tracker_update: dcap %d not in [1,64]", dcap);
    AV_REQUIRE(cfg->trajectory_length >= 1, AV_EINVAL, "av_tracker_update: trajectory_length must be >= 1");
    AV_REQUIRE(cfg->iou_threshold >= 0.0, AV_EINVAL,
               "av_tracker_update: iou_threshold < 0 never terminates in the reference either");
    AV_REQUIRE((snap == nullptr) == (snap_n == nullptr), AV_EINVAL, "av_tracker_update: snap and snap_n go together");
    const TrackerPlan p = tracker_plan(*cfg, n_frames, dcap, tcap);
    if (p.replica) {
        AV_REQUIRE(p.lds_need <= 160 * 1024, AV_EINVAL, "av_tracker_update: %zu bytes of LDS", p.lds_need);
        if (p.lds_claim > 64 * 1024) {
            // needs the attribute, once for each device this process launches the kernel on (it belongs to the device's copy of the function)
            static std::mutex mu;
            int dev = 0;
            AV_HIP(hipGetDevice(&dev));
            std::lock_guard<std::mutex> lk(mu);
            if (dev < 0 || dev >= 64 || !((p.inst->lds_raised >> dev) & 1ull)) {
                AV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(p.inst->fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
                if (dev >= 0 && dev < 64) p.inst->lds_raised |= 1ull << dev;
            }
        }
    }
    hipLaunchKernelGGL(p.inst->fn, dim3(n_streams), dim3(p.block), p.lds_claim, as_stream(stream), *cfg, n_frames, dcap, det_n, det_box,
                       det_cls, det_conf, tcap, (unsigned char*)state, snap, snap_n, det2trk, p.fc, p.wave_map);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"
