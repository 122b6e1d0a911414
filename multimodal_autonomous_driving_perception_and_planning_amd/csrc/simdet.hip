// D1: simulated detector on device: the kernels and the entry points.  The device code they run (the MT19937 restatement, the
// draw table's row, simdet_frame) is in simdet_dev.h, with the reference it restates.
#include "simdet_dev.h"

namespace {

__global__ void __launch_bounds__(64) simdet_table_kernel(SimRow* __restrict__ tab) {
    const int seed = blockIdx.x * blockDim.x + threadIdx.x;
    if (seed >= 1000) return;
    Mt m;
    mt_seed(m, (uint32_t)seed);
    SimRow r;
    r.n = mt_randint(m, 3, 8);
    for (int i = 0; i < 7; ++i) {
        SimVehicle v{};
        if (i < r.n) {                                  // draw order per vehicle: uniform, randint, randint, choice, uniform
            v.depth = mt_uniform(m, 0.3, 1.0 - 0.3);
            v.r1 = mt_randint(m, -10, 10);
            v.r2 = mt_randint(m, -5, 5);
            v.u = mt_double(m);
            v.conf = mt_uniform(m, 0.75, 0.98 - 0.75);
        }
        r.v[i] = v;
    }
    r.overflow = (int32_t)m.overflow;
    tab[seed] = r;
}

// thread = (stream, frame).  ADVANCE: the launch holds one frame per stream, so the thread that read the counter
// also writes it back (no second launch).
template <bool ADVANCE>
__global__ void __launch_bounds__(64) simdet_kernel(int n_streams, int n_frames, int h, int w, int dcap,
                                                    int32_t* __restrict__ frame_count, const SimRow* __restrict__ tab,
                                                    const double* __restrict__ cdf, int32_t* __restrict__ det_n,
                                                    int32_t* __restrict__ det_box, int32_t* __restrict__ det_cls,
                                                    double* __restrict__ det_conf, int32_t* __restrict__ status) {
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_streams * n_frames) return;
    simdet_frame<ADVANCE>(gid, (int)(gid / n_frames), (int)(gid % n_frames), h, w, dcap, frame_count, tab, cdf, det_n, det_box, det_cls,
                          det_conf, status);
}

__global__ void advance_counter_kernel(int n_streams, int n_frames, int32_t* frame_count) {
    int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_streams) frame_count[s] += n_frames;
}

}  // namespace

// called by av_ctx_create / av_ctx_destroy (ctx.hip)
int av_simdet_ctx_init(av_ctx* ctx) {
    AV_HIP(hipMalloc(&ctx->d_simtab, 1000 * sizeof(SimRow)));
    hipLaunchKernelGGL(simdet_table_kernel, dim3(16), dim3(64), 0, nullptr, (SimRow*)ctx->d_simtab);
    AV_LAUNCH_CHECK();
    AV_HIP(hipDeviceSynchronize());
    return AV_OK;
}

extern "C" int av_simdet_generate(av_ctx* ctx, av_stream_t stream, int n_streams, int n_frames, int h, int w,
                                  int dcap, int32_t* frame_count, int32_t* det_n, int32_t* det_box,
                                  int32_t* det_cls, double* det_conf, int32_t* status) {
    AV_REQUIRE(ctx && frame_count && det_n && det_box && det_cls && det_conf, AV_EINVAL,
               "av_simdet_generate: null argument");
    AV_REQUIRE(n_streams > 0 && n_frames > 0, AV_EINVAL, "av_simdet_generate: n_streams/n_frames must be > 0");
    AV_REQUIRE(dcap >= 7 && dcap <= 64, AV_EINVAL, "av_simdet_generate: dcap %d not in [7,64]", dcap);
    AV_REQUIRE(h > 0 && w > 121, AV_EINVAL, "av_simdet_generate: frame %dx%d too small (w - box_w must stay > 0)", w, h);
    AV_REQUIRE(ctx->d_simtab, AV_ESTATE, "av_simdet_generate: context has no draw table");
    const long long total = (long long)n_streams * n_frames;
    const int grid = (int)((total + 63) / 64);
    const SimRow* tab = (const SimRow*)ctx->d_simtab;
    if (n_frames == 1) {
        hipLaunchKernelGGL(simdet_kernel<true>, dim3(grid), dim3(64), 0, as_stream(stream), n_streams, n_frames, h, w, dcap,
                           frame_count, tab, ctx->d_cdf, det_n, det_box, det_cls, det_conf, status);
        AV_LAUNCH_CHECK();
        return AV_OK;
    }
    hipLaunchKernelGGL(simdet_kernel<false>, dim3(grid), dim3(64), 0, as_stream(stream), n_streams, n_frames, h, w, dcap,
                       frame_count, tab, ctx->d_cdf, det_n, det_box, det_cls, det_conf, status);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(advance_counter_kernel, dim3((n_streams + 63) / 64), dim3(64), 0, as_stream(stream), n_streams,
                       n_frames, frame_count);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
