// D2: YOLOv8 detector (yolov8.yaml's Detect models of scales n, s and m with 1 - 256 classes; default n, 80), MFMA convolution path.
//
// Reference call site: ObjectDetector._detect_yolo (src/perception/detector.py:103-123) ->
// ultralytics YOLO(model_path)(frame), "yolov8n.pt" by default (third party, not vendored; topology restated in
// oracle/yolo_ref.py at scale n, which also defines the parameter order this file consumes; av_yolo_model and
// build_graph state it for every scale).
//
// Layout: activations are NHWC half with an explicit channel stride, so a producer can write straight
// into a channel slice of a concat buffer (every Concat / chunk of the graph is free) and a consumer can
// read a slice.  Convolution = implicit GEMM on v_mfma_f32_16x16x32_f16 with the *weights* as the A
// operand (rows = output channels) and the gathered input patch as B (columns = output pixels): the
// accumulator then holds 4 consecutive channels of one pixel per lane, i.e. an 8-byte NHWC store.
// BatchNorm (eval) is folded into weights/bias on the host; SiLU, the Bottleneck residual and the
// half conversion are fused into the epilogue.  K = taps*Cin is padded to a multiple of 32; Cin is
// always a multiple of 8, so one lane's 8-element fragment never straddles a filter tap.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

namespace {

// Element type of activations and weights: IEEE half (11 significant bits, float32 accumulation in the MFMA).  ultralytics'
// own GPU inference mode is half precision; bf16 (8 bits) was measured first and moved boxes by several pixels against the
// fp32 restatement (tests/test_gpu_yolo.py: end-to-end parity), at the same MFMA rate.
typedef _Float16 half_t;
using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half2v = __attribute__((ext_vector_type(2))) _Float16;
using f32x4 = __attribute__((ext_vector_type(4))) float;
struct alignas(8) half4 { half_t x, y, z, w; };

constexpr int NC = 80, REG_MAX = 16, MAX_CAND = 8192;

__host__ __device__ inline half_t f2h(float f) { return (half_t)f; }          // round to nearest even (v_cvt_f16_f32)
__device__ inline float h2f(half_t b) { return (float)b; }
__device__ inline half4 make_half4(float a, float b, float c, float d) { return half4{f2h(a), f2h(b), f2h(c), f2h(d)}; }

struct ConvArgs {
    const half_t* in;   int in_cs, in_coff, cin, H, W;        // input NHWC (batch folded into pixels via n)
    const half_t* wgt;  const float* bias; int kpad, kreal, ksz, stride;
    half_t* out;        float* out32; int out_cs, out_coff, cout, Ho, Wo;
    const half_t* res;  int res_cs, res_coff;                 // optional residual (added after the activation)
    int act, npix;                                            // npix = B*Ho*Wo
    // virtual Upsample + Concat in front of a 1x1 convolution (the neck's C2f cv1 at P4 / P3): input channels [0, k1) are `in` read at
    // HALF resolution (pixel (y >> 1, x >> 1): nearest-neighbour x2), channels [k1, cin) are `in2` at full resolution.  in2 = NULL:
    // one ordinary input.  The upsampled copy (63 / 126 MB per 64 frames) is then neither written nor read.
    const half_t* in2;  int in2_cs, in2_coff, k1;
};

// SiLU with v_rcp_f32 (1 ulp) instead of an IEEE divide: the result is rounded to half anyway, and the epilogue of
// these small convolutions is as long as their K loop.
// The product is made opaque before it can meet a conversion to half: hipcc 7.2 otherwise folds "multiply, then round to half" into one
// v_fma_mixlo_f16 (a single rounding) in SOME kernels and keeps v_mul_f32 + v_cvt_f16_f32 (two roundings) in others -- one half-precision ulp
// apart on 1 element in 15 000, which is what made c2f32_head_kernel differ from the launches it replaces before this line was added.
__device__ __forceinline__ float silu(float v) {
    float r = v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
    asm("" : "+v"(r));
    return r;
}


// Progress-ordered wave priority for the persistent tile loops (lane.hip, front_pack, and DESIGN.md section 4 "front end"): waves of
// equal priority are served oldest first, so workgroups that share a CU finish one after the other and the last one runs at low
// occupancy.  A workgroup lowers its priority as its tiles go by (3 -> 0).
__device__ __forceinline__ void progress_prio(int t, int n_tiles) {
    const int q = (4 * t) / (n_tiles > 0 ? n_tiles : 1);            // t runs over the whole grid's tiles: same fraction for every workgroup
    if (q <= 0) __builtin_amdgcn_s_setprio(3);
    else if (q == 1) __builtin_amdgcn_s_setprio(2);
    else if (q == 2) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

template <int MT, int NT>
__global__ void __launch_bounds__(256) conv_mfma_kernel(ConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pix_base = (blockIdx.x * 4 + wave) * 16 * NT;
    const int ch_base = blockIdx.y * 16 * MT;
    if (pix_base >= a.npix) return;
    const int l15 = lane & 15, h = lane >> 4, pad = a.ksz >> 1;
    int iy0[NT], ix0[NT], nb[NT];
    bool pv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int p = pix_base + nt * 16 + l15;
        pv[nt] = p < a.npix;
        const int pp = pv[nt] ? p : 0;
        const int n = pp / (a.Ho * a.Wo), r = pp - n * a.Ho * a.Wo;
        const int oy = r / a.Wo, ox = r - oy * a.Wo;
        iy0[nt] = oy * a.stride - pad, ix0[nt] = ox * a.stride - pad, nb[nt] = n * a.H;
    }
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // bias now, consumed once before the first store: gfx9's single in-order vmcnt would otherwise make every bias wait in
    // the epilogue a wait for the stores before it
    float4 bsv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) bsv[mt] = *reinterpret_cast<const float4*>(a.bias + ch_base + mt * 16 + 4 * h);
    int k = 8 * h, tap = k / a.cin, ci = k - tap * a.cin;
    const half_t* wrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) wrow[mt] = a.wgt + (size_t)(ch_base + mt * 16 + l15) * a.kpad + 8 * h;
    // Operands come straight from global memory (weights: L2), so a K step's latency is a memory latency: a ring of D steps is
    // kept in flight -- step s + D is requested right after step s's MFMAs (the stride-2 layers at P4/P5 have 18-36 steps and
    // about one workgroup per CU: without the ring every step paid the latency in turn, 52 us for 9 GFLOP).
    constexpr int D = MT >= 4 ? 4 : 6;
    half8 A[D][MT], Bf[D][NT];
    const int nsteps = a.kpad / 32;
    int ld_step = 0;                                        // next step to request; tap / ci follow it
    auto request = [&](int slot) {
        const int k0 = ld_step * 32;
        const int ky = a.ksz == 1 ? 0 : tap / 3, kx = a.ksz == 1 ? 0 : tap - ky * 3;
        const bool kv = (k0 + 8 * h) < a.kreal;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) A[slot][mt] = *reinterpret_cast<const half8*>(wrow[mt] + k0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int iy = iy0[nt] + ky, ix = ix0[nt] + kx;
            const bool ok = kv && pv[nt] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (ok) v = *reinterpret_cast<const half8*>(a.in + ((size_t)(nb[nt] + iy) * a.W + ix) * a.in_cs + a.in_coff + ci);
            Bf[slot][nt] = v;
        }
        ci += 32;
        while (ci >= a.cin) ci -= a.cin, ++tap;
        ++ld_step;
    };
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < nsteps) request(d);
    for (int s0 = 0; s0 < nsteps; s0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (s0 + d < nsteps) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[d][mt], Bf[d][nt], acc[mt][nt], 0, 0, 0);
                if (ld_step < nsteps) request(d);
            }
        }
    }
    // epilogue: lane holds channels ch_base + mt*16 + 4h + {0..3} of pixel pix_base + nt*16 + l15
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) asm volatile("" ::"v"(bsv[mt].x), "v"(bsv[mt].y), "v"(bsv[mt].z), "v"(bsv[mt].w));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int ch = ch_base + mt * 16 + 4 * h;
        const float4 bs = bsv[mt];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (!pv[nt]) continue;
            const size_t p = (size_t)(pix_base + nt * 16 + l15);
            float v[4] = {acc[mt][nt][0] + bs.x, acc[mt][nt][1] + bs.y, acc[mt][nt][2] + bs.z, acc[mt][nt][3] + bs.w};
            if (a.act)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = silu(v[q]);
            if (a.res) {
                const half4 rr = *reinterpret_cast<const half4*>(a.res + p * a.res_cs + a.res_coff + ch);
                v[0] += h2f(rr.x), v[1] += h2f(rr.y), v[2] += h2f(rr.z), v[3] += h2f(rr.w);
            }
            if (a.out32) *reinterpret_cast<float4*>(a.out32 + p * a.out_cs + a.out_coff + ch) = make_float4(v[0], v[1], v[2], v[3]);
            else
                *reinterpret_cast<half4*>(a.out + p * a.out_cs + a.out_coff + ch) = make_half4(v[0], v[1], v[2], v[3]);
        }
    }
}

// GEMM form for the long-K 3x3 layers on small maps (cin = 128, stride 2: P4 -> P5 in the backbone and in the neck; K = 1152).
// conv_mfma_kernel gives every wave its own 147-KB stream of weights from L2 for 32 pixels (5.5 % MFMA busy, 52.6 / 41.6 + 29.1 us
// per 64 frames); here a workgroup of four waves owns 64 flattened output pixels x 128 output channels and walks K half a TAP (64
// input channels: two 32-wide MFMA steps, 16 MFMAs per wave) per barrier through double-buffered LDS slabs (weights 128 rows x
// 128 B, pixels 64 rows x 128 B, 160-byte rows = 32 mod 64: conflict-free ds_read_b128; 60 KB: two workgroups per CU cover each
// other's waits).  A step's six 16-byte pieces per thread are requested at the top of the step before the previous one (ahead of
// that step's MFMAs) and go to LDS at the top of the previous step, behind its barrier.  22.0 + 18.2 us per 64 frames.
// Two earlier forms, for the record: 32 channels per barrier with a three-deep register ring -- the compiler reused the ring's
// registers as address temporaries and waited for every load right behind its issue (28-35 us per layer); a whole tap per barrier
// (110 KB of LDS, one workgroup per CU, 32.8 + 19.4 us).  A select on a loaded value (`ok ? v : 0`) placed at the load makes the
// compiler wait for ALL loads there (vmcnt(0)): out-of-image pieces are zeroed when they go to LDS instead.
// Same K order (tap outer, 32-channel chunk inner), same zero padding, same epilogue as conv_mfma_kernel: bit-identical outputs
// (tests/test_gpu_yolo.py::test_gemm_form_stride2_layers_equal_streaming_kernel).
// Also takes 1 x 1 convolutions (one tap, cin / 64 steps): plain GEMMs, same chunk order as conv1x1_ws_kernel / conv_lds_kernel.
constexpr int CG_SC = 64, CG_ROWB = CG_SC * 2 + 32;     // channels per barrier step (cin % 64 == 0; 60 KB of LDS: two workgroups per CU
                                                        // cover each other's load latency); bytes per LDS row
__global__ void __launch_bounds__(256) conv_gemm128_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cg_smem[];
    unsigned char* As = cg_smem;                              // [2][128 rows]
    unsigned char* Bs = cg_smem + 2 * 128 * CG_ROWB;          // [2][64 rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    const int wm = wave & 1, wn = wave >> 1;       // this wave's 64 output channels / 32 pixels of the workgroup's 128 x 64
    const int pix_base = blockIdx.x * 64, ch_base = blockIdx.y * 128;
    // ---- what this thread stages per step: 64 bytes of one weight row and 32 bytes of one pixel's channels ------------------------
    const int arow_s = tid >> 1, ahalf = tid & 1, brow_s = tid >> 2, bq = tid & 3;
    const half_t* wsrc = a.wgt + (size_t)(ch_base + arow_s) * a.kpad + ahalf * 32;
    const int sp = pix_base + brow_s;
    const bool spv = sp < a.npix;
    const int spp = spv ? sp : 0;
    const int sn = spp / (a.Ho * a.Wo), sr = spp - sn * a.Ho * a.Wo, soy = sr / a.Wo, sox = sr - soy * a.Wo;
    const int pad = a.ksz >> 1;
    const int iy0 = soy * a.stride - pad, ix0 = sox * a.stride - pad;
    // (named registers, not arrays: as arrays written in one lambda and read in another they ended up in scratch)
    uint4 ra0, ra1, ra2, ra3, rb0, rb1;
    unsigned rm = 0;
    const int SPT = a.cin / CG_SC, NSTEP = a.ksz * a.ksz * SPT;      // steps per tap, steps
    auto gload = [&](int st) {
        const int tap = st / SPT, part = st - tap * SPT, ky = a.ksz == 3 ? tap / 3 : 0, kx = tap - ky * 3;
        const uint4* wp = reinterpret_cast<const uint4*>(wsrc + (size_t)st * CG_SC);
        ra0 = wp[0], ra1 = wp[1], ra2 = wp[2], ra3 = wp[3];
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = spv && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        // (clamped to pixel (0, 0) when outside: always readable; zeroed when the pieces go to LDS)
        const int cy = ok ? iy : 0, cx = ok ? ix : 0, c0 = part * CG_SC + bq * 16;
        const half_t* src = a.in + ((size_t)(sn * a.H + cy) * a.W + cx) * a.in_cs + a.in_coff + c0;
        if (a.in2) {     // virtual Upsample + Concat (1 x 1 only; k1 a multiple of 64): channels below k1 from `in` at half resolution
            if (part * CG_SC >= a.k1) src = a.in2 + ((size_t)(sn * a.H + cy) * a.W + cx) * a.in2_cs + a.in2_coff + c0 - a.k1;
            else src = a.in + ((size_t)(sn * (a.H >> 1) + (cy >> 1)) * (a.W >> 1) + (cx >> 1)) * a.in_cs + a.in_coff + c0;
        }
        const uint4* bp = reinterpret_cast<const uint4*>(src);
        rb0 = bp[0], rb1 = bp[1];
        rm = ok ? ~0u : 0u;
    };
    auto msk = [&](const uint4& v) { return make_uint4(v.x & rm, v.y & rm, v.z & rm, v.w & rm); };
    auto lstore = [&](int buf) {
        uint4* da = reinterpret_cast<uint4*>(As + (size_t)(buf * 128 + arow_s) * CG_ROWB + ahalf * 64);
        da[0] = ra0, da[1] = ra1, da[2] = ra2, da[3] = ra3;
        uint4* db = reinterpret_cast<uint4*>(Bs + (size_t)(buf * 64 + brow_s) * CG_ROWB + bq * 32);
        db[0] = msk(rb0), db[1] = msk(rb1);
    };
    f32x4 acc[4][2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 bsv[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) bsv[mt] = *reinterpret_cast<const float4*>(a.bias + ch_base + wm * 64 + mt * 16 + 4 * h);
    gload(0);
    lstore(0);
    if (NSTEP > 1) gload(1);                       // (cin = 64 with one tap is a single step: nothing behind it to request)
#pragma unroll 1
    for (int tap = 0; tap < NSTEP; ++tap) {        // (`tap` counts steps: half taps)
        __syncthreads();                           // the step's slab is in LDS; the other buffer's readers (step - 1) are done
        const unsigned char* arow = As + (size_t)((tap & 1) * 128 + wm * 64 + l15) * CG_ROWB + 16 * h;
        const unsigned char* brow = Bs + (size_t)((tap & 1) * 64 + wn * 32 + l15) * CG_ROWB + 16 * h;
        if (tap + 1 < NSTEP) lstore((tap + 1) & 1);  // requested a whole step ago
        if (tap + 2 < NSTEP) gload(tap + 2);         // in flight during this step's MFMAs; goes to LDS at the top of the next step
#pragma unroll
        for (int c = 0; c < CG_SC / 32; ++c) {
            half8 A[4], B[2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) A[mt] = *reinterpret_cast<const half8*>(arow + mt * 16 * CG_ROWB + c * 64);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) B[nt] = *reinterpret_cast<const half8*>(brow + nt * 16 * CG_ROWB + c * 64);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[mt], B[nt], acc[mt][nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) asm volatile("" ::"v"(bsv[mt].x), "v"(bsv[mt].y), "v"(bsv[mt].z), "v"(bsv[mt].w));
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int ch = ch_base + wm * 64 + mt * 16 + 4 * h;
        const float4 bs = bsv[mt];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int pi = pix_base + wn * 32 + nt * 16 + l15;
            if (pi >= a.npix) continue;
            const size_t p = (size_t)pi;
            float v[4] = {acc[mt][nt][0] + bs.x, acc[mt][nt][1] + bs.y, acc[mt][nt][2] + bs.z, acc[mt][nt][3] + bs.w};
            if (a.act)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = silu(v[q]);
            if (a.out32) *reinterpret_cast<float4*>(a.out32 + p * a.out_cs + a.out_coff + ch) = make_float4(v[0], v[1], v[2], v[3]);
            else
                *reinterpret_cast<half4*>(a.out + p * a.out_cs + a.out_coff + ch) = make_half4(v[0], v[1], v[2], v[3]);
        }
    }
}

// LDS-tiled variant for Cin % 32 == 0 (all but the first few layers).  A workgroup (4 waves) owns an 8x16
// output tile of one image and 16*MT output channels.  Per 32-channel chunk of the input it stages
//   patch [PH*PW pixels][32 ch]   (the tile's receptive field incl. halo, zero outside the image)
//   wts   [16*MT rows][taps*32]   (this chunk's slice of the folded weights)
// in LDS with 32 bytes of padding per pixel / row (96- and 608-byte strides, = 32 mod 64: every ds_read_b128 of
// one of the instruction's 16-lane groups lands on distinct banks), then runs taps MFMA steps per chunk entirely out of LDS: the
// input is fetched once per tile instead of once per tap and the weights once per workgroup instead of
// once per wave.  Wave w computes output rows 2w, 2w+1 of the tile (16 columns each).
constexpr int LT_H = 8, LT_W = 16, LT_CK = 32, LT_PIXB = LT_CK * 2 + 32;   // row strides = 32 mod 64 bytes: ds_read_b128's four 16-lane groups
// ({0-3,12-15,20-27}, ...: MI355X_MICROARCH.md LDS) then touch every bank once; with 16 bytes of padding 7 of 8 slots collided 2-way
constexpr int lt_pixb(int stride) { return stride == 1 ? LT_PIXB : LT_CK * 2 + 16; }   // stride 2: neighbouring lanes read pixels two apart, so the
// pixel stride is = 16 mod 32 bytes (twice that = 32 mod 64), as in conv3x3_ws_kernel

template <int MT, int KS, int S = 1>     // KS: kernel size (1 or 3); S: stride.  (A stride-2 instance for the two cin = 128 stride-2 layers -- 17 x 33
// patch per chunk -- was measured in round 3: 62.6 / 34.3 us against conv_mfma_kernel's 53.8 / 29.3 us; not kept for them.  S = 2 serves the
// stride-2 layers of the wider scales that neither conv3x3_ws_kernel (weights past the LDS) nor conv_gemm128_kernel (cin % 64, cout % 128)
// takes: scale m's 96 -> 192, 384 -> 576 and 192 -> 192.)
__global__ void __launch_bounds__(256) conv_lds_kernel(ConvArgs a, int tiles_x, int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    constexpr int taps = KS * KS, pad = KS >> 1, s = S, PIXB = lt_pixb(S);
    constexpr int PH = (LT_H - 1) * S + KS, PW = (LT_W - 1) * S + KS;
    constexpr int wrowb = taps * LT_CK * 2 + 32;
    unsigned char* patch = lsm;
    unsigned char* wts = lsm + (((size_t)PH * PW * PIXB + 15) & ~size_t(15));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y, n = bid / tiles_y;
    const int oy0 = ty * LT_H, ox0 = tx * LT_W;
    const int ch_base = blockIdx.y * 16 * MT;
    const int iy_org = oy0 * s - pad, ix_org = ox0 * s - pad;
    f32x4 acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt][0] = acc[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Staging plan of this thread, fixed for the whole K loop: which 16-byte pieces of the input patch and
    // of the weight slab it moves, as global element offsets (chunk offset c0 added per trip) and LDS byte
    // offsets.  The divisions live here, once; the K loop then only issues loads, and the NEXT chunk's
    // loads are in flight (in registers) while the current chunk's MFMAs run.
    constexpr int NP = (PH * PW * 4 + 255) / 256, NW = (16 * MT * taps * 4 + 255) / 256;
    const int part8 = (tid & 3) * 8;           // every piece of this thread is the same 8-channel part of a chunk
    int p_g[NP], p_l[NP], w_g[NW], w_l[NW];
    int p_g2[KS == 1 ? NP : 1];                // second source of a virtual Upsample + Concat (1x1 only): offset into a.in2, minus k1
    const bool dual = KS == 1 && a.in2 != nullptr;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int i = tid + k * 256;
        p_g[k] = -1, p_l[k] = -1;
        if (KS == 1) p_g2[k] = -1;
        if (i < PH * PW * 4) {
            const int pix = i >> 2, part = i & 3;
            const int py = pix / PW, px = pix - py * PW;
            const int iy = iy_org + py, ix = ix_org + px;
            p_l[k] = pix * PIXB + part * 16;
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                if (dual) {
                    p_g[k] = ((n * (a.H >> 1) + (iy >> 1)) * (a.W >> 1) + (ix >> 1)) * a.in_cs + a.in_coff + part * 8;
                    if (KS == 1) p_g2[k] = ((n * a.H + iy) * a.W + ix) * a.in2_cs + a.in2_coff + part * 8 - a.k1;
                } else {
                    p_g[k] = ((n * a.H + iy) * a.W + ix) * a.in_cs + a.in_coff + part * 8;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const int i = tid + k * 256;
        w_g[k] = -1, w_l[k] = 0;
        if (i < 16 * MT * taps * 4) {
            const int row = i / (taps * 4), rem = i - row * taps * 4, tap = rem >> 2, part = rem & 3;
            w_l[k] = row * wrowb + (tap * LT_CK + part * 8) * 2;
            w_g[k] = (ch_base + row) * a.kpad + tap * a.cin + part * 8;
        }
    }
    uint4 pv[NP], wv[NW];
    auto gload = [&](int c0) {
        const bool inch = c0 + part8 < a.cin;  // cin need not be a multiple of the chunk: the tail is zero-filled
        const bool second = KS == 1 && dual && c0 >= a.k1;         // (k1 is a multiple of the chunk: a chunk comes from one source)
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const half_t* src = second ? a.in2 + (size_t)p_g2[KS == 1 ? k : 0] : a.in + (size_t)p_g[k];
            pv[k] = (p_g[k] >= 0 && inch) ? *reinterpret_cast<const uint4*>(src + c0) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < NW; ++k)
            wv[k] = (w_g[k] >= 0 && inch) ? *reinterpret_cast<const uint4*>(a.wgt + (size_t)w_g[k] + c0) : make_uint4(0, 0, 0, 0);
    };
    gload(0);
    // bias and residual of this lane's outputs are fetched now: in the epilogue their latency would be exposed
    float4 bsv[MT];
    uint2 resv[MT][2];                                   // raw halves; outside the map: pixel 0, never used
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int ch = ch_base + mt * 16 + 4 * h;
        bsv[mt] = *reinterpret_cast<const float4*>(a.bias + ch);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            resv[mt][nt] = make_uint2(0, 0);
            const int oy = oy0 + 2 * wave + nt, ox = ox0 + l15;
            const size_t rp = (oy < a.Ho && ox < a.Wo) ? ((size_t)n * a.Ho + oy) * a.Wo + ox : 0;
            if (a.res) resv[mt][nt] = *reinterpret_cast<const uint2*>(a.res + rp * a.res_cs + a.res_coff + ch);
        }
    }
    for (int c0 = 0; c0 < a.cin; c0 += LT_CK) {
        __syncthreads();                        // every wave is done reading the previous chunk
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (p_l[k] >= 0) *reinterpret_cast<uint4*>(patch + p_l[k]) = pv[k];
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (w_g[k] >= 0) *reinterpret_cast<uint4*>(wts + w_l[k]) = wv[k];
        __syncthreads();
        if (c0 + LT_CK < a.cin) gload(c0 + LT_CK);
        for (int tap = 0; tap < taps; ++tap) {
            const int ky = KS == 1 ? 0 : tap / 3, kx = KS == 1 ? 0 : tap - ky * 3;
            half8 A[MT], B[2];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                A[mt] = *reinterpret_cast<const half8*>(wts + (size_t)(mt * 16 + l15) * wrowb + (tap * LT_CK + 8 * h) * 2);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                B[nt] = *reinterpret_cast<const half8*>(patch + (size_t)(((2 * wave + nt) * s + ky) * PW + l15 * s + kx) * PIXB + 16 * h);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[mt], B[nt], acc[mt][nt], 0, 0, 0);
        }
    }
    // one wait for bias and residual before the first store (see conv3x3_ws_kernel)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        asm volatile("" ::"v"(bsv[mt].x), "v"(bsv[mt].y), "v"(bsv[mt].z), "v"(bsv[mt].w));
        asm volatile("" ::"v"(resv[mt][0].x), "v"(resv[mt][0].y), "v"(resv[mt][1].x), "v"(resv[mt][1].y));
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int ch = ch_base + mt * 16 + 4 * h;
        const float4 bs = bsv[mt];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int oy = oy0 + 2 * wave + nt, ox = ox0 + l15;
            if (oy >= a.Ho || ox >= a.Wo) continue;
            const size_t p = ((size_t)n * a.Ho + oy) * a.Wo + ox;
            float v[4] = {acc[mt][nt][0] + bs.x, acc[mt][nt][1] + bs.y, acc[mt][nt][2] + bs.z, acc[mt][nt][3] + bs.w};
            if (a.act)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = silu(v[q]);
            if (a.res) {
                const half4 rr = *reinterpret_cast<const half4*>(&resv[mt][nt]);
                v[0] += h2f(rr.x), v[1] += h2f(rr.y), v[2] += h2f(rr.z), v[3] += h2f(rr.w);
            }
            if (a.out32) *reinterpret_cast<float4*>(a.out32 + p * a.out_cs + a.out_coff + ch) = make_float4(v[0], v[1], v[2], v[3]);
            else
                *reinterpret_cast<half4*>(a.out + p * a.out_cs + a.out_coff + ch) = make_half4(v[0], v[1], v[2], v[3]);
        }
    }
}

// Weight-stationary persistent variant for the 3x3 stride-1 layers whose whole folded weight matrix fits the LDS beside one
// input patch (cin 16/32/64/80, cout <= 80: the C2f bottlenecks at P2-P4 and the 3x3 layers of the Detect head).  A workgroup
// of NW = 8 waves loads the layer's weights ONCE ([cout][tap][cin] rows), then walks output tiles of NW NT rows x 16 columns.
// Per tile the input patch with ALL channels goes through LDS in one piece, so a tile costs one barrier pair instead of one
// per 32-channel chunk and conv_lds_kernel's per-chunk weight slab traffic disappears.  What the measurements asked for
// (tools/wmfma.hip, profiles/README.md):
//  * two waves per SIMD: ONE wave issues a 16x16x32 MFMA only every ~32 cycles (53 % of the matrix peak), two interleave;
//  * operands of K step s+1 are requested before the MFMAs of step s (sched_barrier keeps them there): the compiler otherwise
//    sinks every ds_read next to its use and each group of MFMAs pays the LDS latency;
//  * gfx9 counts loads AND stores in one in-order vmcnt: a wait for a bias/residual load placed between the epilogue's stores
//    waits for those stores as well.  Bias and residual registers are therefore consumed once, before the first store, and the
//    next tile's patch (registers) and residual loads are issued AFTER the epilogue's stores and consumed after the next
//    tile's MFMAs;
//  * LDS row strides = 32 mod 64 bytes (ws_stride): ds_read_b128's four 16-lane groups then touch every bank once.
// Same K order (chunk outer, tap inner), zero padding and epilogue as conv_lds_kernel: bit-identical outputs, cin = 80 included
// (tests/test_gpu_yolo.py::test_cin80_layers_equal_generic_kernels).
// row stride of an LDS image: the bytes rounded up to = 32 mod 64 (conflict-free ds_read_b128, see conv_lds_kernel)
constexpr int ws_stride(int bytes) { return bytes + (32 - bytes % 64 + 64) % 64; }

// S: stride (1 or 2).  With stride 2 neighbouring lanes read pixels two apart, so the pixel stride is = 16 mod 32 bytes
// (twice that = 32 mod 64) for the same conflict-free reads; the tile is 8 rows x 16 columns of OUTPUT pixels, its patch 17 x 33.
template <int MT, int NT, int NW, int CINP, bool RES, int S = 1>   // NW waves, NT output rows each: tile = NW NT rows x 16 columns
__global__ void __launch_bounds__(NW * 64) conv3x3_ws_kernel(ConvArgs a, int tiles_x, int tiles_y, int n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    constexpr int PH = (NW * NT - 1) * S + 3, PW = (LT_W - 1) * S + 3, NTH = NW * 64;
    constexpr int cinp = CINP, pixb = S == 1 ? ws_stride(cinp * 2) : cinp * 2 + 16, wrowb = ws_stride(9 * cinp * 2), parts = cinp >> 3;   // 16-byte pieces per pixel
    unsigned char* wts = lsm;
    unsigned char* patch = lsm + (((size_t)16 * MT * wrowb + 15) & ~size_t(15));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    const int ch_base = blockIdx.y * 16 * MT;
    // ---- patch pieces of this thread: piece i = pixel i / parts of the patch, channels 8 (i % parts) .. +7; the position inside
    // the patch never changes, so the decomposition is done once ------------------------------------------------------------
    constexpr int npieces = PH * PW * parts, NP = (npieces + NTH - 1) / NTH;
    int p_rel[NP], p_yx[NP];                      // element offset relative to the patch origin; py << 16 | px (-1: no piece)
    uint4 pv[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int i = tid + k * NTH;
        const int pix = i / parts, part = i - pix * parts, py = pix / PW, px = pix - py * PW;
        p_rel[k] = (py * a.W + px) * a.in_cs + part * 8;
        p_yx[k] = (i < npieces && part * 8 < a.cin) ? (py << 16 | px) : -1;
    }
    auto tile_origin = [&](int t, int& n, int& oy0, int& ox0) {
        const int tx = t % tiles_x, r = t / tiles_x;
        n = r / tiles_y, oy0 = (r % tiles_y) * NW * NT, ox0 = tx * LT_W;
    };
    auto gload = [&](int t) {
        int n, oy0, ox0;
        tile_origin(t, n, oy0, ox0);
        const half_t* base = a.in + ((long)(n * a.H + oy0 * S - 1) * a.W + ox0 * S - 1) * a.in_cs + a.in_coff;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int iy = oy0 * S - 1 + (p_yx[k] >> 16), ix = ox0 * S - 1 + (p_yx[k] & 0xFFFF);
            pv[k] = make_uint4(0, 0, 0, 0);
            if (p_yx[k] >= 0 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                pv[k] = *reinterpret_cast<const uint4*>(base + p_rel[k]);
        }
    };
    int t = blockIdx.x;
    if (t < n_tiles) gload(t);
    // ---- the weights, once: global row [tap][cin] -> LDS row [tap][cinp], channels cin .. cinp-1 zero.  Loads are issued in
    // batches of WB before the first LDS store: one exposed L2 latency per batch instead of one per piece -----------------
    {
        constexpr int WP = 16 * MT * 9 * parts, WB = 9;
        for (int i0 = 0; i0 < WP; i0 += NTH * WB) {
            uint4 wv[WB];
#pragma unroll
            for (int k = 0; k < WB; ++k) {
                const int i = i0 + k * NTH + tid;
                const int row = i / (9 * parts), rem = i - row * 9 * parts, tap = rem / parts, part = rem - tap * parts;
                wv[k] = make_uint4(0, 0, 0, 0);
                if (i < WP && part * 8 < a.cin)
                    wv[k] = *reinterpret_cast<const uint4*>(a.wgt + (size_t)(ch_base + row) * a.kpad + tap * a.cin + part * 8);
            }
#pragma unroll
            for (int k = 0; k < WB; ++k) {
                const int i = i0 + k * NTH + tid;
                const int row = i / (9 * parts), rem = i - row * 9 * parts, tap = rem / parts, part = rem - tap * parts;
                if (i < WP) *reinterpret_cast<uint4*>(wts + (size_t)row * wrowb + (tap * cinp + part * 8) * 2) = wv[k];
            }
        }
    }
    float4 bsv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) bsv[mt] = *reinterpret_cast<const float4*>(a.bias + ch_base + mt * 16 + 4 * h);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) asm volatile("" ::"v"(bsv[mt].x), "v"(bsv[mt].y), "v"(bsv[mt].z), "v"(bsv[mt].w));   // waited for here, once
    // this lane's outputs of a tile: pixel (oy0 + NT wave + nt, ox0 + l15), channels ch_base + 16 mt + 4 h .. +3
    uint2 resv[MT][NT];                                               // residual (raw halves) of the tile about to be computed
    auto rload = [&](int tt) {
        int n, oy0, ox0;
        tile_origin(tt, n, oy0, ox0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int oy = oy0 + NT * wave + nt, ox = ox0 + l15;
            const bool ok = oy < a.Ho && ox < a.Wo;
            const long p = ok ? ((long)n * a.Ho + oy) * a.Wo + ox : 0;          // pixel 0: always addressable, value unused
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                resv[mt][nt] = *reinterpret_cast<const uint2*>(a.res + p * a.res_cs + a.res_coff + ch_base + mt * 16 + 4 * h);
        }
    };
    const unsigned char* arow = wts + (size_t)l15 * wrowb;
    const unsigned char* brow = patch + (size_t)(NT * wave * S * PW + l15 * S) * pixb;
    // K steps: chunk outer, tap inner (conv_lds_kernel's order); 32 channels per step, a last chunk of 16 (cin = 80) is a K = 32
    // step zero-padded in registers
    constexpr int NK32 = cinp / LT_CK, NSTEP = 9 * (NK32 + (cinp % LT_CK ? 1 : 0));
    auto ld_ab = [&](half8* A, half8* B, int step) {
        const int chunk = step / 9, c0 = chunk * LT_CK, tap = step % 9, ky = tap / 3, kx = tap - ky * 3;
        if (chunk < NK32) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) A[mt] = *reinterpret_cast<const half8*>(arow + mt * 16 * wrowb + (tap * cinp + c0) * 2 + 16 * h);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) B[nt] = *reinterpret_cast<const half8*>(brow + ((nt * S + ky) * PW + kx) * pixb + c0 * 2 + 16 * h);
        } else {
            // last chunk of 16 channels (cin = 80): a K = 32 step whose upper 16 k are zeros in BOTH operands -- lane groups 0, 1
            // hold channels c0 + 8h .. +7, groups 2, 3 zeros (their loads repeat group h & 1's address and are discarded).  Exactly
            // conv_lds_kernel's zero-filled partial chunk, so the two kernels stay bit-identical for cin = 80 too.  (A K = 16 MFMA
            // accumulating onto a K = 32 MFMA's result was used here before: hipcc 7.2 inserts no wait states between the two
            // different-length MFMAs and the second can read a stale accumulator -- DESIGN.md section 6.)
            const half8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
            const int ho = 16 * (h & 1);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const half8 v = *reinterpret_cast<const half8*>(arow + mt * 16 * wrowb + (tap * cinp + c0) * 2 + ho);
                A[mt] = h < 2 ? v : z8;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const half8 v = *reinterpret_cast<const half8*>(brow + ((nt * S + ky) * PW + kx) * pixb + c0 * 2 + ho);
                B[nt] = h < 2 ? v : z8;
            }
        }
    };
    auto mma = [&](f32x4 (&acc)[MT][NT], const half8* A, const half8* B, int) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[mt], B[nt], acc[mt][nt], 0, 0, 0);
    };
    // ---- pipeline: the patch of tile t is put into LDS one iteration ahead, the loads of tile t+1 (patch -> registers) and the
    // residual of tile t are issued just before tile t's MFMAs and consumed right after them ------------------------------
    __syncthreads();                                                   // weights in
    if (t < n_tiles) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = tid + k * NTH;
            const int pix = i / parts, part = i - pix * parts;
            if (i < npieces) *reinterpret_cast<uint4*>(patch + pix * pixb + part * 16) = pv[k];
        }
        if (t + (int)gridDim.x < n_tiles) gload(t + gridDim.x);
        if (RES) rload(t);
    }
    for (; t < n_tiles; t += gridDim.x) {
        progress_prio(t, n_tiles);
        __syncthreads();                                               // patch of tile t visible
        f32x4 acc[MT][NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            // operands of step s+1 are requested before the MFMAs of step s are issued (one wave per SIMD: nobody else hides
            // the LDS latency); sched_barrier keeps the compiler from sinking the reads back to their first use
            half8 A0[MT], B0[NT], A1[MT], B1[NT];
            ld_ab(A0, B0, 0);
#pragma unroll
            for (int st = 0; st < NSTEP; st += 2) {
                if (st + 1 < NSTEP) ld_ab(A1, B1, st + 1);
                __builtin_amdgcn_sched_barrier(0);
                mma(acc, A0, B0, st);
                __builtin_amdgcn_sched_barrier(0);
                if (st + 1 < NSTEP) {
                    if (st + 2 < NSTEP) ld_ab(A0, B0, st + 2);
                    __builtin_amdgcn_sched_barrier(0);
                    mma(acc, A1, B1, st + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();                                               // every wave is done reading the patch of tile t
        const bool more = t + (int)gridDim.x < n_tiles;
        if (more) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int i = tid + k * NTH;
                const int pix = i / parts, part = i - pix * parts;
                if (i < npieces) *reinterpret_cast<uint4*>(patch + pix * pixb + part * 16) = pv[k];
            }
        }
        // gfx9 counts loads and stores in one in-order counter: a wait for a residual load placed between the epilogue's stores
        // would also wait for the stores before it.  Consuming every residual register here makes that ONE wait, for loads that
        // were issued before the MFMAs; the stores below are then never waited for inside the epilogue.
        if (RES) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) asm volatile("" ::"v"(resv[mt][nt].x), "v"(resv[mt][nt].y));
        }
        {
            int n, oy0, ox0;
            tile_origin(t, n, oy0, ox0);
            const int ox = ox0 + l15;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int oy = oy0 + NT * wave + nt;
                const bool ok = oy < a.Ho && ox < a.Wo;
                const long p = ((long)n * a.Ho + oy) * a.Wo + ox;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int ch = ch_base + mt * 16 + 4 * h;
                    const float4 bs = bsv[mt];
                    float v[4] = {acc[mt][nt][0] + bs.x, acc[mt][nt][1] + bs.y, acc[mt][nt][2] + bs.z, acc[mt][nt][3] + bs.w};
                    if (a.act)
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = silu(v[q]);
                    if (RES) {
                        const half4 rr = *reinterpret_cast<const half4*>(&resv[mt][nt]);
                        v[0] += h2f(rr.x), v[1] += h2f(rr.y), v[2] += h2f(rr.z), v[3] += h2f(rr.w);
                    }
                    if (ok) {
                        if (a.out32) *reinterpret_cast<float4*>(a.out32 + p * a.out_cs + a.out_coff + ch) = make_float4(v[0], v[1], v[2], v[3]);
                        else *reinterpret_cast<half4*>(a.out + p * a.out_cs + a.out_coff + ch) = make_half4(v[0], v[1], v[2], v[3]);
                    }
                }
            }
        }
        if (more) {
            if (t + 2 * (int)gridDim.x < n_tiles) gload(t + 2 * gridDim.x);
            if (RES) rload(t + gridDim.x);
        }
    }
}

// 1x1 convolutions (C2f cv1/cv2, SPPF, the head's last layer before the decode): a plain GEMM [pixels x cin] x [cin x cout] with no
// halo, so the pixel operand needs no LDS at all -- a lane's MFMA B fragment (pixel l15, channels 32 k + 8 h .. +7) is 16
// contiguous bytes of the NHWC input and the four lane groups of a pixel cover one 64-byte segment.  The workgroup keeps its
// 16 MT output channels' weights in LDS for its whole life ([16 MT][cin] rows, stride = 32 mod 64 bytes), each wave then walks
// 32-pixel tiles on its own: all KS = cin / 32 fragments of a tile are requested at once (one exposed latency per tile instead
// of conv_lds_kernel's one per 32-channel chunk, and no barrier after the weight load); two to four waves per SIMD cover it.
// Same K order and epilogue as conv_lds_kernel: bit-identical outputs.
// DEC: the Detect head's decode in the epilogue of its last convolutions, so that the float32 logits (185 MB per 64 frames) are
// neither written nor read again.  1: box branch (64 = 4 sides x 16 bins): the tile's logits take a per-wave detour through LDS
// so that lane group h holds all 16 bins of side h of its pixel, then decode_kernel's arithmetic to the letter (sequential
// max / exp / sums over the bins, IEEE divide) and one box coordinate per lane.  2: class branch (80 classes): first maximum
// (lowest class among equals, as decode_kernel's scan) over the lane's 20 values and across the four lane groups, sigmoid.
// Candidates equal decode_kernel's bit for bit (test_fused_decode_equals_decode_kernel).  3: the class branch of any other model --
// dec.nc classes at run time in 16 MT >= nc output channels (the rest are zero filters: logits of exactly 0.0f, stored with the kept
// logits but never a candidate for the maximum); the 80-class instantiation (2) keeps its compile-time count.
struct DecArgs { float* cbox; float* cconf; int* ccls; int A, aoff, stride, keep_logits, nc; };      // nc: read by DEC = 3 only
constexpr int DEC_ROW = 68;                        // floats per pixel row of the box detour (64 + 4: conflict-free b128 rows)

template <int MT, int KS, bool TAIL16 = false, int DEC = 0>      // TAIL16: 16 more input channels after the KS whole steps (cin = 80), as a zero-padded K = 32 step
__global__ void __launch_bounds__(DEC == 1 ? 128 : 256) conv1x1_ws_kernel(ConvArgs a, int n_tiles, DecArgs dec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    constexpr int NT = 2, cin = KS * 32 + (TAIL16 ? 16 : 0), wrowb = ws_stride(cin * 2), parts = cin >> 3;
    // waves per workgroup: two for the box decode, whose per-wave LDS detour would otherwise push the workgroup past the 19 KB
    // that stay free on a CU beside the other head lane's 144-KB 3x3 kernel
    constexpr int NWV = DEC == 1 ? 2 : 4, NTH = NWV * 64;
    static_assert(DEC == 0 || (DEC == 1 && MT == 4) || (DEC == 2 && MT == 5) || DEC == 3, "decode epilogues belong to the 64- and 80-channel head outputs, or take nc at run time");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    const int ch_base = blockIdx.y * 16 * MT;
    {
        constexpr int WP = 16 * MT * parts, WB = WP >= 8 * NTH ? 8 : (WP + NTH - 1) / NTH;
        for (int i0 = 0; i0 < WP; i0 += NTH * WB) {
            uint4 wv[WB];
#pragma unroll
            for (int k = 0; k < WB; ++k) {
                const int i = i0 + k * NTH + tid, row = i / parts, part = i - row * parts;
                wv[k] = make_uint4(0, 0, 0, 0);
                if (i < WP) wv[k] = *reinterpret_cast<const uint4*>(a.wgt + (size_t)(ch_base + row) * a.kpad + part * 8);
            }
#pragma unroll
            for (int k = 0; k < WB; ++k) {
                const int i = i0 + k * NTH + tid, row = i / parts, part = i - row * parts;
                if (i < WP) *reinterpret_cast<uint4*>(lsm + (size_t)row * wrowb + part * 16) = wv[k];
            }
        }
    }
    float4 bsv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) bsv[mt] = *reinterpret_cast<const float4*>(a.bias + ch_base + mt * 16 + 4 * h);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) asm volatile("" ::"v"(bsv[mt].x), "v"(bsv[mt].y), "v"(bsv[mt].z), "v"(bsv[mt].w));
    __syncthreads();
    const unsigned char* arow = lsm + (size_t)l15 * wrowb + 16 * h;
    // a wave's tile: pixels 32 t .. 32 t + 31 (fragment nt: pixels 32 t + 16 nt + l15); tiles strided over all waves of the grid
    const int wstride = gridDim.x * NWV;
    for (int t = blockIdx.x * NWV + wave; t < n_tiles; t += wstride) {
        progress_prio(t, n_tiles);
        half8 B[KS][NT];
        half8 Bt[NT];
        long pix[NT];
        const half8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const long p = (long)t * 32 + nt * 16 + l15;
            pix[nt] = p;
            const half_t* px0 = a.in + (p < a.npix ? p : 0) * a.in_cs + a.in_coff;              // beyond the end: pixel 0, never stored
            const half_t* src = px0 + 8 * h;
#pragma unroll
            for (int k = 0; k < KS; ++k) B[k][nt] = *reinterpret_cast<const half8*>(src + k * 32);
            if (TAIL16) Bt[nt] = *reinterpret_cast<const half8*>(px0 + KS * 32 + 8 * (h & 1));
        }
        f32x4 acc[MT][NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            half8 A[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) A[mt] = *reinterpret_cast<const half8*>(arow + mt * 16 * wrowb + k * 64);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[mt], B[k][nt], acc[mt][nt], 0, 0, 0);
        }
        if (TAIL16) {            // the last 16 channels as a K = 32 step zero-padded in registers (lane groups 2, 3): conv_mfma_kernel's padded
            // K to the bit, and no K = 16 MFMA behind a K = 32 one (see conv3x3_ws_kernel)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const half8 av = *reinterpret_cast<const half8*>(lsm + (size_t)(mt * 16 + l15) * wrowb + KS * 64 + 16 * (h & 1));
                const half8 a8 = h < 2 ? av : z8;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a8, h < 2 ? Bt[nt] : z8, acc[mt][nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const long p = pix[nt];
            float vv[MT][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int ch = ch_base + mt * 16 + 4 * h;
                const float4 bs = bsv[mt];
                float v[4] = {acc[mt][nt][0] + bs.x, acc[mt][nt][1] + bs.y, acc[mt][nt][2] + bs.z, acc[mt][nt][3] + bs.w};
                if (a.act)
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = silu(v[q]);
#pragma unroll
                for (int q = 0; q < 4; ++q) vv[mt][q] = v[q];
                if (p < a.npix && (DEC == 0 || dec.keep_logits)) {
                    if (a.out32) *reinterpret_cast<float4*>(a.out32 + p * a.out_cs + a.out_coff + ch) = make_float4(v[0], v[1], v[2], v[3]);
                    else *reinterpret_cast<half4*>(a.out + p * a.out_cs + a.out_coff + ch) = make_half4(v[0], v[1], v[2], v[3]);
                }
            }
            if (DEC) {
                const int hw = a.Ho * a.Wo;
                const long pc = p < a.npix ? p : 0;
                const int n = (int)(pc / hw), r = (int)(pc - (long)n * hw), y = r / a.Wo, x = r - y * a.Wo;
                const size_t ci = (size_t)n * dec.A + dec.aoff + r;                      // candidate index, as decode_kernel's
                if (DEC == 1) {
                    float* sc = reinterpret_cast<float*>(lsm + (((size_t)16 * MT * wrowb + 15) & ~size_t(15))) + wave * 16 * DEC_ROW;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        *reinterpret_cast<float4*>(sc + l15 * DEC_ROW + mt * 16 + 4 * h) = make_float4(vv[mt][0], vv[mt][1], vv[mt][2], vv[mt][3]);
                    float b[REG_MAX];                    // side h of pixel l15 (LDS operations of one wave complete in order)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float4 t4 = *reinterpret_cast<const float4*>(sc + l15 * DEC_ROW + h * 16 + 4 * k);
                        b[4 * k] = t4.x, b[4 * k + 1] = t4.y, b[4 * k + 2] = t4.z, b[4 * k + 3] = t4.w;
                    }
                    float mx = -INFINITY;
#pragma unroll
                    for (int j = 0; j < REG_MAX; ++j) mx = fmaxf(mx, b[j]);
                    float sum = 0.f, ex = 0.f;
#pragma unroll
                    for (int j = 0; j < REG_MAX; ++j) {
                        const float e = __expf(b[j] - mx);
                        sum += e, ex += e * (float)j;
                    }
                    const float d = ex / sum;
                    const float ac = (h & 1) ? (float)y + 0.5f : (float)x + 0.5f, st = (float)dec.stride;
                    if (p < a.npix) dec.cbox[ci * 4 + h] = (h < 2 ? ac - d : ac + d) * st;
                } else {
                    float best = -INFINITY;
                    int bj = 0;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (vv[mt][q] > best && (DEC == 2 || mt * 16 + 4 * h + q < dec.nc)) best = vv[mt][q], bj = mt * 16 + 4 * h + q;
#pragma unroll
                    for (int off = 16; off < 64; off <<= 1) {
                        const float ob = __shfl_xor(best, off, 64);
                        const int oj = __shfl_xor(bj, off, 64);
                        if (ob > best || (ob == best && oj < bj)) best = ob, bj = oj;
                    }
                    if (p < a.npix && h == 0) {
                        dec.cconf[ci] = 1.f / (1.f + expf(-best));
                        dec.ccls[ci] = bj;
                    }
                }
            }
        }
    }
}

// Fused C2f block with 16 hidden channels, one bottleneck, shortcut (layer 2 of the network, the 1/4-resolution map: 983k
// pixels per 64 frames).  Its four convolutions (cv1 1x1 32->32, 3x3 16->16, 3x3 16->16 + residual, cv2 1x1 48->32) move
// 63 + 63 MB when fused; as four launches they moved 440 MB and took 130 us, every one of them HBM-bound.  A workgroup owns a
// 16x16 output tile: the input patch with a 2-pixel halo (20x20x32) goes to LDS once, cv1 runs in place on it (y0 | y1),
// the first 3x3 writes its 18x18x16 result to a second LDS image, the second 3x3's result (y2) takes a 512-byte per-wave
// detour through LDS into operand layout, and cv2 consumes y0 | y1 | y2.  All four weight matrices stay in LDS for the
// workgroup's life.  The arithmetic is the unfused layers' to the bit: the same K = 32 MFMA steps in the same order (16-channel
// operands zero-padded to 32 exactly as conv3x3_ws_kernel / conv_mfma_kernel pad them), the same epilogue expressions,
// intermediates rounded to half at the same points; positions outside the image hold zeros (the 3x3 convolutions' padding).
// tests/test_gpu_yolo.py compares the two paths bit for bit.
struct C2f16Args {
    const half_t* in;  int in_cs, in_coff;
    half_t* out;       int out_cs, out_coff;
    int H, W, tiles_x, tiles_y, n_tiles;
    const half_t *w_cv1, *w_b1, *w_b2, *w_cv2;      // [32][32], [16][kb], [16][kb], [32][kc]: global row strides 32, kb, kb, kc
    const float *bs_cv1, *bs_b1, *bs_b2, *bs_cv2;
    int kb, kc;
};

constexpr int C2F_XW = 20, C2F_TW = 18, C2F_XS = 96, C2F_TS = 32;           // patch widths and pixel strides (bytes, = 32 mod 64)
constexpr int C2F_NW = 8, C2F_NTH = C2F_NW * 64;                              // waves per workgroup: the MFMA chains of the 3x3 stages are
// dependent (9 taps onto one accumulator), so the SIMDs need several waves each to stay busy
constexpr int C2F_W1S = 96, C2F_WBS = 608, C2F_W2S = 160;                    // weight row strides in LDS (= 32 mod 64)
constexpr int C2F_OFF_T1 = 400 * C2F_XS, C2F_OFF_W1 = C2F_OFF_T1 + 324 * C2F_TS, C2F_OFF_WB1 = C2F_OFF_W1 + 32 * C2F_W1S,
              C2F_OFF_WB2 = C2F_OFF_WB1 + 16 * C2F_WBS, C2F_OFF_W2 = C2F_OFF_WB2 + 16 * C2F_WBS, C2F_OFF_Y2 = C2F_OFF_W2 + 32 * C2F_W2S,
              C2F_OFF_Z = C2F_OFF_Y2 + C2F_NW * 16 * 32, C2F_LDS = C2F_OFF_Z + 64;    // Z: 64 zero bytes
static_assert(2 * C2F_LDS <= 160 * 1024, "two workgroups per CU");

__global__ void __launch_bounds__(C2F_NTH, 4) c2f16_fused_kernel(C2f16Args a) {      // (second argument = waves per SIMD: 4 = two 8-wave workgroups per CU)
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    unsigned char* XY = lsm;                                  // [400][32 ch]: input patch, then cv1's output in place
    unsigned char* T1 = lsm + C2F_OFF_T1;                     // [324][16 ch]
    unsigned char* W1 = lsm + C2F_OFF_W1;                     // cv1 [32][32]
    unsigned char* WB1 = lsm + C2F_OFF_WB1;                   // 3x3 #1 [16][9 taps][16 ch + 16 zeros]
    unsigned char* WB2 = lsm + C2F_OFF_WB2;
    unsigned char* W2 = lsm + C2F_OFF_W2;                     // cv2 [32][48 + 16 zeros]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    unsigned char* Y2 = lsm + C2F_OFF_Y2 + wave * 512;        // this wave's [16 px][16 ch]
    // ---- weights, once ---------------------------------------------------------------------------------------------------
    for (int i = tid; i < 32 * 4; i += C2F_NTH) *reinterpret_cast<uint4*>(W1 + (i >> 2) * C2F_W1S + (i & 3) * 16) = *reinterpret_cast<const uint4*>(a.w_cv1 + (i >> 2) * 32 + (i & 3) * 8);
    for (int i = tid; i < 16 * 9 * 4; i += C2F_NTH) {             // piece = 8 channels of one tap; pieces 2, 3 of a tap are the zero padding
        const int row = i / 36, rem = i - row * 36, tap = rem >> 2, part = rem & 3;
        uint4 v1 = make_uint4(0, 0, 0, 0), v2 = v1;
        if (part < 2) {
            v1 = *reinterpret_cast<const uint4*>(a.w_b1 + row * a.kb + tap * 16 + part * 8);
            v2 = *reinterpret_cast<const uint4*>(a.w_b2 + row * a.kb + tap * 16 + part * 8);
        }
        *reinterpret_cast<uint4*>(WB1 + row * C2F_WBS + tap * 64 + part * 16) = v1;
        *reinterpret_cast<uint4*>(WB2 + row * C2F_WBS + tap * 64 + part * 16) = v2;
    }
    for (int i = tid; i < 32 * 8; i += C2F_NTH) {
        const int row = i >> 3, part = i & 7;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (part < 6) v = *reinterpret_cast<const uint4*>(a.w_cv2 + row * a.kc + part * 8);
        *reinterpret_cast<uint4*>(W2 + row * C2F_W2S + part * 16) = v;
    }
    const float4 bs1a = *reinterpret_cast<const float4*>(a.bs_cv1 + 4 * h), bs1b = *reinterpret_cast<const float4*>(a.bs_cv1 + 16 + 4 * h);
    const float4 bsb1 = *reinterpret_cast<const float4*>(a.bs_b1 + 4 * h), bsb2 = *reinterpret_cast<const float4*>(a.bs_b2 + 4 * h);
    const float4 bs2a = *reinterpret_cast<const float4*>(a.bs_cv2 + 4 * h), bs2b = *reinterpret_cast<const float4*>(a.bs_cv2 + 16 + 4 * h);
#define C2F_USE(b) asm volatile("" ::"v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w))
    C2F_USE(bs1a); C2F_USE(bs1b); C2F_USE(bsb1); C2F_USE(bsb2); C2F_USE(bs2a); C2F_USE(bs2b);              // waited for here, once
#undef C2F_USE
    // ---- input patch pieces of this thread: 400 pixels x 4 pieces of 8 channels -----------------------------------------------
    constexpr int NP = (400 * 4 + C2F_NTH - 1) / C2F_NTH;
    uint4 pv[NP];
    auto origin = [&](int t, int& n, int& oy0, int& ox0) {
        const int tx = t % a.tiles_x, r = t / a.tiles_x;
        n = r / a.tiles_y, oy0 = (r % a.tiles_y) * 16, ox0 = tx * 16;
    };
    auto gload = [&](int t) {
        int n, oy0, ox0;
        origin(t, n, oy0, ox0);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = tid + k * C2F_NTH, pix = i >> 2, part = i & 3;
            const int py = pix / C2F_XW, px = pix - py * C2F_XW, iy = oy0 - 2 + py, ix = ox0 - 2 + px;
            pv[k] = make_uint4(0, 0, 0, 0);
            if (i < 1600 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                pv[k] = *reinterpret_cast<const uint4*>(a.in + ((size_t)(n * a.H + iy) * a.W + ix) * a.in_cs + a.in_coff + part * 8);
        }
    };
    if (tid < 4) *reinterpret_cast<uint4*>(lsm + C2F_OFF_Z + tid * 16) = make_uint4(0, 0, 0, 0);
    // 16 channels at p as the B operand of a K = 32 step: lane groups 0, 1 hold them, groups 2, 3 the zero padding -- read from
    // the zero bytes, so that the load is unconditional and the nine taps' operands can be requested together
    const unsigned char* zsrc = lsm + C2F_OFF_Z;
    auto b16 = [&](const unsigned char* p) { return *reinterpret_cast<const half8*>(h < 2 ? p + 16 * h : zsrc); };
    int t = blockIdx.x;
    if (t < a.n_tiles) gload(t);
    for (; t < a.n_tiles; t += gridDim.x) {
        progress_prio(t, a.n_tiles);
        int n, oy0, ox0;
        origin(t, n, oy0, ox0);
        __syncthreads();                                       // previous tile done with XY / T1 (and the weights are in)
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = tid + k * C2F_NTH;
            if (i < 1600) *reinterpret_cast<uint4*>(XY + (i >> 2) * C2F_XS + (i & 3) * 16) = pv[k];
        }
        __syncthreads();
        if (t + (int)gridDim.x < a.n_tiles) gload(t + gridDim.x);          // next tile's patch in flight during this tile
        // ---- cv1 in place: 25 groups of 16 patch pixels, each wave its own ------------------------------------------------
        for (int g = wave; g < 25; g += C2F_NW) {
            const int pix = g * 16 + l15;
            const int py = pix / C2F_XW, px = pix - py * C2F_XW;
            const bool inside = (unsigned)(oy0 - 2 + py) < (unsigned)a.H && (unsigned)(ox0 - 2 + px) < (unsigned)a.W;
            unsigned char* xp = XY + pix * C2F_XS;
            const half8 b = *reinterpret_cast<const half8*>(xp + 16 * h);
            f32x4 acc[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const half8 w = *reinterpret_cast<const half8*>(W1 + (mt * 16 + l15) * C2F_W1S + 16 * h);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            }
            // the MFMAs have read all 32 channels of these 16 pixels (every lane of the wave): in place is safe
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float4 bs = mt ? bs1b : bs1a;
                float v[4] = {acc[mt][0] + bs.x, acc[mt][1] + bs.y, acc[mt][2] + bs.z, acc[mt][3] + bs.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = inside ? silu(v[q]) : 0.f;      // outside the image: the 3x3 convolutions' zero padding
                *reinterpret_cast<half4*>(xp + mt * 32 + 8 * h) = make_half4(v[0], v[1], v[2], v[3]);
            }
        }
        __syncthreads();
        // ---- 3x3 #1 on y1 (channels 16..31): 18x18 outputs = 21 groups of 16 -------------------------------------------------
        for (int g = wave; g < 21; g += C2F_NW) {
            const int q = g * 16 + l15, qq = q < 324 ? q : 323;
            const int ty = qq / C2F_TW, tx = qq - ty * C2F_TW;
            const bool inside = (unsigned)(oy0 - 1 + ty) < (unsigned)a.H && (unsigned)(ox0 - 1 + tx) < (unsigned)a.W;
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            half8 bv[9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) bv[tap] = b16(XY + ((ty + tap / 3) * C2F_XW + tx + tap % 3) * C2F_XS + 32);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const half8 wv = *reinterpret_cast<const half8*>(WB1 + l15 * C2F_WBS + tap * 64 + 16 * h);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv, bv[tap], c, 0, 0, 0);
            }
            float v[4] = {c[0] + bsb1.x, c[1] + bsb1.y, c[2] + bsb1.z, c[3] + bsb1.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = inside ? silu(v[k]) : 0.f;
            if (q < 324) *reinterpret_cast<half4*>(T1 + q * C2F_TS + 8 * h) = make_half4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        // ---- 3x3 #2 + shortcut -> y2, then cv2 on [y0 | y1 | y2]: one output row of 16 pixels per step ----------------------------
        for (int r = wave; r < 16; r += C2F_NW) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
            half8 bv[9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) bv[tap] = b16(T1 + ((r + tap / 3) * C2F_TW + l15 + tap % 3) * C2F_TS);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const half8 wv = *reinterpret_cast<const half8*>(WB2 + l15 * C2F_WBS + tap * 64 + 16 * h);
                c = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv, bv[tap], c, 0, 0, 0);
            }
            const unsigned char* xp = XY + ((r + 2) * C2F_XW + l15 + 2) * C2F_XS;
            {
                const half4 rr = *reinterpret_cast<const half4*>(xp + 32 + 8 * h);          // the shortcut: y1
                float v[4] = {c[0] + bsb2.x, c[1] + bsb2.y, c[2] + bsb2.z, c[3] + bsb2.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = silu(v[k]);
                v[0] += h2f(rr.x), v[1] += h2f(rr.y), v[2] += h2f(rr.z), v[3] += h2f(rr.w);
                *reinterpret_cast<half4*>(Y2 + l15 * 32 + 8 * h) = make_half4(v[0], v[1], v[2], v[3]);
            }
            const half8 b01 = *reinterpret_cast<const half8*>(xp + 16 * h);
            const half8 b2v = b16(Y2 + l15 * 32);               // same wave wrote it: LDS operations of a wave complete in order
            const int oy = oy0 + r, ox = ox0 + l15;
            const bool ok = oy < a.H && ox < a.W;
            half_t* op = a.out + ((size_t)(n * a.H + oy) * a.W + ox) * a.out_cs + a.out_coff + 4 * h;
            f32x4 o[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const half8 wa = *reinterpret_cast<const half8*>(W2 + (mt * 16 + l15) * C2F_W2S + 16 * h);
                o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, b01, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const half8 wb = *reinterpret_cast<const half8*>(W2 + (mt * 16 + l15) * C2F_W2S + 64 + 16 * h);
                o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb, b2v, o[mt], 0, 0, 0);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float4 bs = mt ? bs2b : bs2a;
                float v[4] = {o[mt][0] + bs.x, o[mt][1] + bs.y, o[mt][2] + bs.z, o[mt][3] + bs.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = silu(v[k]);
                if (ok) *reinterpret_cast<half4*>(op + mt * 16) = make_half4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

// Fused C2f blocks with 32 hidden channels (the 1/8-resolution map, P3: layer 4 with two bottlenecks and shortcuts, layer 15 with
// one and none).  Two kernels on 16 x 16 output tiles with a 2-pixel halo, 16 waves per workgroup, every weight matrix they use
// resident in LDS; with 32 channels a 3x3 tap is exactly one K = 32 MFMA step.
//   c2f32_head_kernel:             cv1 (1x1 64 -> 64, in place on the patch) -> 3x3 -> 3x3 + shortcut; writes y0 | y1 | y2 into the
//                                  block's concat buffer (layer 4's first half: three launches in one)
//   c2f32_tail_kernel<KCAT, RES>:  3x3 -> 3x3 (+ shortcut) on the concat buffer's last 32 channels, then cv2 (1x1 KCAT + 32 -> 64)
//                                  whose first KCAT input channels come straight from the concat buffer in global memory (no halo:
//                                  conv1x1_ws_kernel's operand loads) and whose last 32 from this tile through a per-wave LDS detour
//                                  (layer 4's second half: KCAT 96, shortcut; layer 15 behind its cv1: KCAT 64, no shortcut)
// Same K steps in the same order, same epilogue expressions and the same half roundings as conv1x1_ws_kernel / conv3x3_ws_kernel /
// conv_lds_kernel: bit-identical outputs (tests/test_gpu_yolo.py: fused == separate launches); positions outside the image hold
// zeros (the 3x3 convolutions' padding).  Layer 4: 6 launches, 107 us -> 2; layer 15: 4 launches -> 2.
struct C2f32Args {
    const half_t* in;  int in_cs, in_coff;           // head: cv1's input (64 ch); tail: the pair's input = concat channels [KCAT - 32, KCAT)
    half_t* cat;       int cat_cs, cat_coff;         // the block's concat buffer (head: written; tail: cv2's first KCAT channels)
    half_t* out;       int out_cs, out_coff;         // tail: cv2's output (64 ch)
    int H, W, tiles_x, tiles_y, n_tiles;
    const half_t *w_cv1, *w_b1, *w_b2, *w_cv2;
    const float *bs_cv1, *bs_b1, *bs_b2, *bs_cv2;
    int k1, kb, kc;                                  // global row strides of cv1, the 3x3 layers, cv2
};
constexpr int F32_NW = 8, F32_NTH = F32_NW * 64, F32_XW = 20, F32_TW = 18, F32_PS = 96;      // strides = 32 mod 64 bytes
constexpr int F32H_XS = 160, F32H_W1S = 160;                                                    // head: 64-channel patch / cv1 rows
constexpr int F32H_OFF_T1 = 400 * F32H_XS, F32H_OFF_W1 = F32H_OFF_T1 + 324 * F32_PS, F32H_LDS = F32H_OFF_W1 + 64 * F32H_W1S;
constexpr int f32t_w2s(int kcat) { return ws_stride((kcat + 32) * 2); }
constexpr int F32T_OFF_T1 = 400 * F32_PS, F32T_OFF_W2 = F32T_OFF_T1 + 324 * F32_PS;
constexpr int f32t_lds(int kcat) { return F32T_OFF_W2 + 64 * f32t_w2s(kcat) + F32_NW * 16 * F32_PS; }
static_assert(F32H_LDS <= 160 * 1024 && f32t_lds(96) <= 160 * 1024, "fits the LDS");

// A 3x3 layer's 32 x 288 weight matrix as MFMA A operands, held in REGISTERS for the workgroup's whole life: fragment (tap, mt) of
// a lane = 8 halves of row 16 mt + l15 at k = 32 tap + 8 h; 18 fragments = 72 registers per layer and lane, the whole matrix per wave.
// With 32 channels a B fragment serves only two MFMAs, so with the weights in LDS (the first version of these kernels) every MFMA
// cost 1.5 KB of LDS reads -- three times what the CU's 128 bytes per clock deliver in an MFMA's time; from registers only the
// pixel operands cross the LDS (0.5 KB per MFMA).
struct F32W { half8 f[18]; };
__device__ __forceinline__ void f32_load_w(F32W& w, const half_t* g, int kb, int l15, int h) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) w.f[tap * 2 + mt] = *reinterpret_cast<const half8*>(g + (size_t)(mt * 16 + l15) * kb + tap * 32 + 8 * h);
}

// first 3x3 of the pair: 18 x 18 outputs (the second 3x3's input incl. halo) in 21 groups of 16, from channels [coff, coff + 32) of the
// 20 x 20 patch XP (pixel stride xs bytes) into T1; zero outside the image
__device__ __forceinline__ void f32_conv_a(const unsigned char* XP, int xs, int coff_bytes, const F32W& w, unsigned char* T1,
                                           const float* bias, int oy0, int ox0, int H, int W, int wave, int l15, int h) {
    for (int g = wave; g < 21; g += F32_NW) {
        const int q = g * 16 + l15, qq = q < 324 ? q : 323;
        const int ty = qq / F32_TW, tx = qq - ty * F32_TW;
        const bool inside = (unsigned)(oy0 - 1 + ty) < (unsigned)H && (unsigned)(ox0 - 1 + tx) < (unsigned)W;
        half8 bv[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            bv[tap] = *reinterpret_cast<const half8*>(XP + ((ty + tap / 3) * F32_XW + tx + tap % 3) * xs + coff_bytes + 16 * h);
        f32x4 c[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) c[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.f[tap * 2 + mt], bv[tap], c[mt], 0, 0, 0);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const float4 bs = *reinterpret_cast<const float4*>(bias + mt * 16 + 4 * h);          // (LDS copy of the bias)
            float v[4] = {c[mt][0] + bs.x, c[mt][1] + bs.y, c[mt][2] + bs.z, c[mt][3] + bs.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = inside ? silu(v[k]) : 0.f;
            if (q < 324) *reinterpret_cast<half4*>(T1 + q * F32_PS + mt * 32 + 8 * h) = make_half4(v[0], v[1], v[2], v[3]);
        }
    }
}

// second 3x3 of the pair for output row r (16 pixels, lane l15 = column): accumulators of the 32 output channels
__device__ __forceinline__ void f32_conv_b(const unsigned char* T1, const F32W& w, int r, int l15, int h, f32x4 (&c)[2]) {
    half8 bv[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) bv[tap] = *reinterpret_cast<const half8*>(T1 + ((r + tap / 3) * F32_TW + l15 + tap % 3) * F32_PS + 16 * h);
    c[0] = c[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) c[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.f[tap * 2 + mt], bv[tap], c[mt], 0, 0, 0);
}

// biases in LDS (read where they are used: the weight fragments need the registers): [cv1 64 | b1 32 | b2 32 | cv2 64] floats
constexpr int F32_BIAS_BYTES = 192 * 4;
__device__ __forceinline__ void f32_load_bias(const C2f32Args& a, float* bl, int tid, bool cv1, bool cv2) {
    if (tid < 64) bl[tid] = cv1 ? a.bs_cv1[tid] : 0.f;
    else if (tid < 96) bl[tid] = a.bs_b1[tid - 64];
    else if (tid < 128) bl[tid] = a.bs_b2[tid - 96];
    else if (tid < 192) bl[tid] = cv2 ? a.bs_cv2[tid - 128] : 0.f;
}

__global__ void __launch_bounds__(F32_NTH) c2f32_head_kernel(C2f32Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    unsigned char* XY = lsm;                                  // [400][64 ch]: input patch, then cv1's output y0 | y1 in place
    unsigned char* T1 = lsm + F32H_OFF_T1;                    // [324][32 ch]
    unsigned char* W1 = lsm + F32H_OFF_W1;                    // cv1 [64][64]
    __shared__ __attribute__((aligned(16))) float bl[192];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    for (int i = tid; i < 64 * 8; i += F32_NTH)
        *reinterpret_cast<uint4*>(W1 + (i >> 3) * F32H_W1S + (i & 7) * 16) = *reinterpret_cast<const uint4*>(a.w_cv1 + (size_t)(i >> 3) * a.k1 + (i & 7) * 8);
    f32_load_bias(a, bl, tid, true, false);
    F32W wa, wb;
    f32_load_w(wa, a.w_b1, a.kb, l15, h);
    f32_load_w(wb, a.w_b2, a.kb, l15, h);
    constexpr int NP = (400 * 8 + F32_NTH - 1) / F32_NTH;         // 16-byte pieces of the 64-channel patch per thread
    auto origin = [&](int t, int& n, int& oy0, int& ox0) {
        const int tx = t % a.tiles_x, r = t / a.tiles_x;
        n = r / a.tiles_y, oy0 = (r % a.tiles_y) * 16, ox0 = tx * 16;
    };
    for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        progress_prio(t, a.n_tiles);
        int n, oy0, ox0;
        origin(t, n, oy0, ox0);
        __syncthreads();                                       // previous tile done with XY / T1 (and the weights are in)
        {   // the patch: all loads first, then the LDS stores (the weight fragments leave no registers to prefetch the next tile's patch)
            uint4 pv[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int i = tid + k * F32_NTH, pix = i >> 3, part = i & 7;
                const int py = pix / F32_XW, px = pix - py * F32_XW, iy = oy0 - 2 + py, ix = ox0 - 2 + px;
                pv[k] = make_uint4(0, 0, 0, 0);
                if (i < 3200 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                    pv[k] = *reinterpret_cast<const uint4*>(a.in + ((size_t)(n * a.H + iy) * a.W + ix) * a.in_cs + a.in_coff + part * 8);
            }
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int i = tid + k * F32_NTH;
                if (i < 3200) *reinterpret_cast<uint4*>(XY + (i >> 3) * F32H_XS + (i & 7) * 16) = pv[k];
            }
        }
        __syncthreads();
        // ---- cv1 in place: 25 groups of 16 patch pixels, two at a time per wave (one read of a weight fragment serves both) ------------
        for (int g0 = 2 * wave; g0 < 25; g0 += 2 * F32_NW) {
            const bool two = g0 + 1 < 25;
            unsigned char* xp[2];
            bool inside[2];
            half8 b[2][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int pix = (g0 + (two ? j : 0)) * 16 + l15;
                const int py = pix / F32_XW, px = pix - py * F32_XW;
                inside[j] = (unsigned)(oy0 - 2 + py) < (unsigned)a.H && (unsigned)(ox0 - 2 + px) < (unsigned)a.W;
                xp[j] = XY + pix * F32H_XS;
                b[j][0] = *reinterpret_cast<const half8*>(xp[j] + 16 * h), b[j][1] = *reinterpret_cast<const half8*>(xp[j] + 64 + 16 * h);
            }
            f32x4 acc[2][4];
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const half8 w = *reinterpret_cast<const half8*>(W1 + (mt * 16 + l15) * F32H_W1S + k * 64 + 16 * h);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[j][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, b[j][k], k ? acc[j][mt] : f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                }
            // the MFMAs have read all 64 channels of these pixels (every lane of the wave): in place is safe
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j && !two) break;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const float4 bs = *reinterpret_cast<const float4*>(bl + mt * 16 + 4 * h);
                    float v[4] = {acc[j][mt][0] + bs.x, acc[j][mt][1] + bs.y, acc[j][mt][2] + bs.z, acc[j][mt][3] + bs.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = inside[j] ? silu(v[q]) : 0.f;
                    *reinterpret_cast<half4*>(xp[j] + mt * 32 + 8 * h) = make_half4(v[0], v[1], v[2], v[3]);
                }
            }
        }
        __syncthreads();
        // ---- y0 | y1 of the tile's own pixels -> concat channels [0, 64) -------------------------------------------------------------------
        for (int i = tid; i < 256 * 8; i += F32_NTH) {
            const int pix = i >> 3, part = i & 7, r = pix >> 4, cx = pix & 15, oy = oy0 + r, ox = ox0 + cx;
            if (oy < a.H && ox < a.W)
                *reinterpret_cast<uint4*>(a.cat + ((size_t)(n * a.H + oy) * a.W + ox) * a.cat_cs + a.cat_coff + part * 8) =
                    *reinterpret_cast<const uint4*>(XY + ((r + 2) * F32_XW + cx + 2) * F32H_XS + part * 16);
        }
        f32_conv_a(XY, F32H_XS, 64, wa, T1, bl + 64, oy0, ox0, a.H, a.W, wave, l15, h);      // on y1 = channels 32..63
        __syncthreads();
        // ---- second 3x3 + shortcut -> y2 = concat channels [64, 96): two output rows per wave ----------------------------------------------
        for (int r = wave; r < 16; r += F32_NW) {
            f32x4 c[2];
            f32_conv_b(T1, wb, r, l15, h, c);
            const unsigned char* xp = XY + ((r + 2) * F32_XW + l15 + 2) * F32H_XS;
            const int oy = oy0 + r, ox = ox0 + l15;
            half_t* op = a.cat + ((size_t)(n * a.H + oy) * a.W + ox) * a.cat_cs + a.cat_coff + 64 + 4 * h;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const half4 rr = *reinterpret_cast<const half4*>(xp + 64 + mt * 32 + 8 * h);          // the shortcut: y1
                const float4 bs = *reinterpret_cast<const float4*>(bl + 96 + mt * 16 + 4 * h);
                float v[4] = {c[mt][0] + bs.x, c[mt][1] + bs.y, c[mt][2] + bs.z, c[mt][3] + bs.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = silu(v[k]);
                v[0] += h2f(rr.x), v[1] += h2f(rr.y), v[2] += h2f(rr.z), v[3] += h2f(rr.w);
                if (oy < a.H && ox < a.W) *reinterpret_cast<half4*>(op + mt * 16) = make_half4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

template <int KCAT, bool SHORTCUT>
__global__ void __launch_bounds__(F32_NTH) c2f32_tail_kernel(C2f32Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    constexpr int W2S = f32t_w2s(KCAT), NKG = KCAT / 32, OFF_Y = F32T_OFF_W2 + 64 * W2S;
    unsigned char* XP = lsm;                                  // [400][32 ch]: the pair's input incl. halo
    unsigned char* T1 = lsm + F32T_OFF_T1;
    unsigned char* W2 = lsm + F32T_OFF_W2;                    // cv2 [64][KCAT + 32]
    __shared__ __attribute__((aligned(16))) float bl[192];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    unsigned char* Y = lsm + OFF_Y + wave * 16 * F32_PS;      // this wave's [16 px][32 ch] detour
    for (int i = tid; i < 64 * (KCAT + 32) / 8; i += F32_NTH) {
        const int row = i / ((KCAT + 32) / 8), piece = i - row * ((KCAT + 32) / 8);
        *reinterpret_cast<uint4*>(W2 + row * W2S + piece * 16) = *reinterpret_cast<const uint4*>(a.w_cv2 + (size_t)row * a.kc + piece * 8);
    }
    f32_load_bias(a, bl, tid, false, true);
    F32W wa, wb;
    f32_load_w(wa, a.w_b1, a.kb, l15, h);
    f32_load_w(wb, a.w_b2, a.kb, l15, h);
    constexpr int NP = (400 * 4 + F32_NTH - 1) / F32_NTH;
    auto origin = [&](int t, int& n, int& oy0, int& ox0) {
        const int tx = t % a.tiles_x, r = t / a.tiles_x;
        n = r / a.tiles_y, oy0 = (r % a.tiles_y) * 16, ox0 = tx * 16;
    };
    for (int t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        progress_prio(t, a.n_tiles);
        int n, oy0, ox0;
        origin(t, n, oy0, ox0);
        __syncthreads();
        {
            uint4 pv[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int i = tid + k * F32_NTH, pix = i >> 2, part = i & 3;
                const int py = pix / F32_XW, px = pix - py * F32_XW, iy = oy0 - 2 + py, ix = ox0 - 2 + px;
                pv[k] = make_uint4(0, 0, 0, 0);
                if (i < 1600 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                    pv[k] = *reinterpret_cast<const uint4*>(a.in + ((size_t)(n * a.H + iy) * a.W + ix) * a.in_cs + a.in_coff + part * 8);
            }
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int i = tid + k * F32_NTH;
                if (i < 1600) *reinterpret_cast<uint4*>(XP + (i >> 2) * F32_PS + (i & 3) * 16) = pv[k];
            }
        }
        __syncthreads();
        f32_conv_a(XP, F32_PS, 0, wa, T1, bl + 64, oy0, ox0, a.H, a.W, wave, l15, h);
        __syncthreads();
        for (int r = wave; r < 16; r += F32_NW) {
            // cv2's operands from the concat buffer (this output row): requested before the second 3x3, used after it
            const int oy = oy0 + r, ox = ox0 + l15;
            const bool ok = oy < a.H && ox < a.W;
            const size_t pix = ok ? (size_t)(n * a.H + oy) * a.W + ox : 0;             // outside: pixel 0, never stored
            half8 bc[NKG];
#pragma unroll
            for (int k = 0; k < NKG; ++k) bc[k] = *reinterpret_cast<const half8*>(a.cat + pix * a.cat_cs + a.cat_coff + k * 32 + 8 * h);
            f32x4 c[2];
            f32_conv_b(T1, wb, r, l15, h, c);
            const unsigned char* xp = XP + ((r + 2) * F32_XW + l15 + 2) * F32_PS;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float4 bs = *reinterpret_cast<const float4*>(bl + 96 + mt * 16 + 4 * h);
                float v[4] = {c[mt][0] + bs.x, c[mt][1] + bs.y, c[mt][2] + bs.z, c[mt][3] + bs.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = silu(v[k]);
                if (SHORTCUT) {
                    const half4 rr = *reinterpret_cast<const half4*>(xp + mt * 32 + 8 * h);
                    v[0] += h2f(rr.x), v[1] += h2f(rr.y), v[2] += h2f(rr.z), v[3] += h2f(rr.w);
                }
                *reinterpret_cast<half4*>(Y + l15 * F32_PS + mt * 32 + 8 * h) = make_half4(v[0], v[1], v[2], v[3]);
            }
            const half8 by = *reinterpret_cast<const half8*>(Y + l15 * F32_PS + 16 * h);    // same wave wrote it: LDS operations of a wave complete in order
            f32x4 o[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int k = 0; k <= NKG; ++k)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const half8 wv = *reinterpret_cast<const half8*>(W2 + (mt * 16 + l15) * W2S + k * 64 + 16 * h);
                    o[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv, k < NKG ? bc[k < NKG ? k : 0] : by, o[mt], 0, 0, 0);
                }
            half_t* op = a.out + pix * a.out_cs + a.out_coff + 4 * h;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float4 bs = *reinterpret_cast<const float4*>(bl + 128 + mt * 16 + 4 * h);
                float v[4] = {o[mt][0] + bs.x, o[mt][1] + bs.y, o[mt][2] + bs.z, o[mt][3] + bs.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = silu(v[k]);
                if (ok) *reinterpret_cast<half4*>(op + mt * 16) = make_half4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

// Stem: 3x3 stride-2 convolution 3 -> 16 channels on the framed NHWC4 input.  K is laid out as [ky][kx 0..3][c 0..3]
// (kx = 3 and c = 3 carry zero weights; 48 -> 64): an 8-element B operand is then two horizontally adjacent input
// pixels = one aligned 16-byte load (the frame makes column 2*ox + kx even and every load in bounds), and the whole
// receptive field is two MFMA steps.  Half the bytes of the 8-channel layout on both sides of the kernel.
// TILED: more than 16 output channels (scales s and m: 32, 48), blockIdx.y = the 16-channel tile; false: the 16-channel stem as it was.
template <bool TILED>
__global__ void __launch_bounds__(256) stem_conv_kernel(ConvArgs a, int npix) {
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, h = lane >> 4;
    const int ch_base = TILED ? blockIdx.y * 16 : 0;
    const half8 A0 = *reinterpret_cast<const half8*>(a.wgt + (ch_base + l15) * 64 + 8 * h);
    const half8 A1 = *reinterpret_cast<const half8*>(a.wgt + (ch_base + l15) * 64 + 32 + 8 * h);
    const float4 bs = *reinterpret_cast<const float4*>(a.bias + ch_base + 4 * h);
    const int pitch = (a.W + 2) * 4, hw = a.Ho * a.Wo;                           // elements per framed input row
    // k-step 0: group h = (ky, kx) = (h >> 1, 2 (h & 1)); k-step 1: ky = 2, groups 2 and 3 have zero weights
    const int off0 = (h >> 1) * pitch + (h & 1) * 8, off1 = 2 * pitch + (h & 1) * 8;
    constexpr int TPV = 4;                                                        // 16-pixel tiles per wave
    const int tile0 = (blockIdx.x * 4 + (tid >> 6)) * TPV;
#pragma unroll
    for (int i = 0; i < TPV; ++i) {
        const int p = (tile0 + i) * 16 + l15;
        const int pc = p < npix ? p : npix - 1;
        const int n = pc / hw, r = pc - n * hw, oy = r / a.Wo, ox = r - oy * a.Wo;
        const half_t* base = a.in + ((size_t)(n * (a.H + 2) + 2 * oy) * (a.W + 2) + 2 * ox) * 4;
        const half8 B0 = *reinterpret_cast<const half8*>(base + off0);
        const half8 B1 = *reinterpret_cast<const half8*>(base + off1);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, B0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1, B1, acc, 0, 0, 0);
        if (p < npix)
            *reinterpret_cast<half4*>(a.out + (size_t)p * a.out_cs + a.out_coff + ch_base + 4 * h) =
                make_half4(silu(acc[0] + bs.x), silu(acc[1] + bs.y), silu(acc[2] + bs.z), silu(acc[3] + bs.w));
    }
}

// letterbox + bilinear resize + BGR->RGB + /255 -> NHWC4 half (channel 3 zero) inside a one-pixel frame of zeros:
// [B][H+2][W+2][4], the frame is the stem convolution's padding and is never written
__global__ void preprocess_kernel(const uint8_t* __restrict__ bgr, int B, int h, int w, int H, int W, int nh, int nw,
                                  int top, int left, half_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H * W) return;
    const int n = i / (H * W), r = i - n * H * W, y = r / W, x = r - y * W;
    float c[3] = {114.f, 114.f, 114.f};
    const int yy = y - top, xx = x - left;
    if (yy >= 0 && yy < nh && xx >= 0 && xx < nw) {
        // source coordinates in double, as the oracle computes them (oracle/yolo_ref.py: preprocess): in float they are off by up to 4e-5 at a
        // generic scale, which moved 1 value in 4 000 of a 90 x 333 frame to the neighbouring uint8 level
        const double sy = ((double)yy + 0.5) * ((double)h / (double)nh) - 0.5, sx = ((double)xx + 0.5) * ((double)w / (double)nw) - 0.5;
        const double fy = floor(sy), fx = floor(sx);
        const float wy = (float)(sy - fy), wx = (float)(sx - fx);
        int y0 = (int)fy, x0 = (int)fx, y1 = y0 + 1, x1 = x0 + 1;
        y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0), y1 = y1 < 0 ? 0 : (y1 > h - 1 ? h - 1 : y1);
        x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0), x1 = x1 < 0 ? 0 : (x1 > w - 1 ? w - 1 : x1);
        const uint8_t* im = bgr + (size_t)n * h * w * 3;
        for (int q = 0; q < 3; ++q) {
            const float p00 = im[((size_t)y0 * w + x0) * 3 + q], p01 = im[((size_t)y0 * w + x1) * 3 + q];
            const float p10 = im[((size_t)y1 * w + x0) * 3 + q], p11 = im[((size_t)y1 * w + x1) * 3 + q];
            const float ta = p00 * (1.f - wx) + p01 * wx, tb = p10 * (1.f - wx) + p11 * wx;
            c[q] = floorf(ta * (1.f - wy) + tb * wy + 0.5f);
        }
    }
    half_t o[4] = {f2h(c[2] / 255.f), f2h(c[1] / 255.f), f2h(c[0] / 255.f), (half_t)0};   // RGB
    *reinterpret_cast<uint2*>(out + (((size_t)n * (H + 2) + y + 1) * (W + 2) + x + 1) * 4) = *reinterpret_cast<const uint2*>(o);
}

// The same for frames that are exactly twice the letterboxed size (1280x720 -> 640x360): the bilinear taps of an
// output pixel are a 2x2 block with weights 1/2 (sx = 2 xx + 0.5 exactly, so the generic kernel's floats come out the
// same), a thread makes two output pixels from 12 contiguous bytes of two rows -- six dword loads instead of 24 byte
// loads.  Needs w % 4 == 0, a 4-byte aligned frame pointer, even left padding and even nw.
__global__ void preprocess2_kernel(const uint8_t* __restrict__ bgr, int B, int h, int w, int H, int W, int nh, int nw,
                                   int top, int left, half_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, W2 = W >> 1;
    if (i >= B * H * W2) return;
    const int n = i / (H * W2), r = i - n * H * W2, y = r / W2, x = (r - y * W2) * 2;
    float c[2][3] = {{114.f, 114.f, 114.f}, {114.f, 114.f, 114.f}};
    const int yy = y - top, xx = x - left;
    if (yy >= 0 && yy < nh && xx >= 0 && xx < nw) {
        const uint8_t* im = bgr + (size_t)n * h * w * 3;
        const unsigned* r0 = reinterpret_cast<const unsigned*>(im + ((size_t)(2 * yy) * w + 2 * xx) * 3);
        const unsigned* r1 = reinterpret_cast<const unsigned*>(im + ((size_t)(2 * yy + 1) * w + 2 * xx) * 3);
        const unsigned a0 = r0[0], b0 = r0[1], c0 = r0[2], a1 = r1[0], b1 = r1[1], c1 = r1[2];
        // bytes: a = B0 G0 R0 B1 | b = G1 R1 B2 G2 | c = R2 B3 G3 R3
        auto px = [](unsigned a, unsigned b, unsigned cc, int p, int q) -> float {
            const int byte = p * 3 + q;
            const unsigned word = byte < 4 ? a : (byte < 8 ? b : cc);
            return (float)((word >> (8 * (byte & 3))) & 255u);
        };
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float p00 = px(a0, b0, c0, 2 * o, q), p01 = px(a0, b0, c0, 2 * o + 1, q);
                const float p10 = px(a1, b1, c1, 2 * o, q), p11 = px(a1, b1, c1, 2 * o + 1, q);
                const float ta = p00 * (1.f - 0.5f) + p01 * 0.5f, tb = p10 * (1.f - 0.5f) + p11 * 0.5f;
                c[o][q] = floorf(ta * (1.f - 0.5f) + tb * 0.5f + 0.5f);
            }
    }
    half_t* dst = out + (((size_t)n * (H + 2) + y + 1) * (W + 2) + x + 1) * 4;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        half_t v[4] = {f2h(c[o][2] / 255.f), f2h(c[o][1] / 255.f), f2h(c[o][0] / 255.f), (half_t)0};   // RGB
        *reinterpret_cast<uint2*>(dst + o * 4) = *reinterpret_cast<const uint2*>(v);
    }
}

// Fused front end for frames that are exactly twice the letterboxed size (1280x720): 2:1 letterbox + stem (3 -> 16, k3 s2) +
// layer 1 (16 -> 32, k3 s2) in ONE launch.  As three launches the 4-channel network input (127 MB per 64 frames) and the stem's
// 1/2-resolution map (126 MB) are each written and read back -- 746 MB of traffic for 240 MB of compulsory bytes (frames in,
// 1/4-resolution map out), every one of the three HBM-bound.  A workgroup owns an 8 x 16 tile of layer 1's output: the 35 x 67
// network-input pixels under it are averaged from the frame into LDS (preprocess2_kernel's float expressions), the stem runs
// on them (17 x 33 outputs = 36 MFMA groups, stem_conv_kernel's two K steps), its SiLU'd half outputs stay in LDS, and layer 1
// reads them with conv3x3_ws_kernel<2,1,8,32,false,2>'s K steps (nine taps, 16 channels zero-padded to K = 32 in registers)
// and epilogue: the output is bit-identical to the three launches (tests/test_gpu_yolo.py).  Halo recompute: 1.10x for the stem.
struct FrontArgs {
    const uint8_t* bgr; int fh, fw;                  // frames [B][fh][fw][3]
    int H, W, top, nh;                               // network input size, letterbox rows [top, top + nh) (left = 0, nw = W)
    const half_t* w_stem; const float* bs_stem;      // [16][64], k = ky*16 + kx*4 + c
    const half_t* w_l1; const float* bs_l1; int kpad1;      // [32][kpad1], k = tap*16 + ci
    half_t* out; int out_cs, out_coff, Ho, Wo;       // layer 1's output [B][Ho][Wo][32]
    int tiles_x, tiles_y, n_tiles;
};
constexpr int FR_XR = 35, FR_XC = 68, FR_SR = 17, FR_SC = 33, FR_SPX = 48, FR_W1S = 288;
constexpr int FR_OFF_S = FR_XR * FR_XC * 8, FR_OFF_W = FR_OFF_S + ((FR_SR * FR_SC * FR_SPX + 15) & ~15), FR_OFF_LUT = FR_OFF_W + 32 * FR_W1S,
              FR_LDS = FR_OFF_LUT + 512;
constexpr int FR_NTH = 512, FR_TASKS = (FR_XR * (FR_XC / 2) + FR_NTH - 1) / FR_NTH;

__global__ void __launch_bounds__(FR_NTH, 4) front_fused_kernel(FrontArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lsm[];
    unsigned char* XL = lsm;                        // [35][68] pixels of 4 halves (R G B 0); column index = X column - (4 ox0 - 3)
    unsigned char* SL = lsm + FR_OFF_S;             // [17 * 33] stem outputs, 16 halves in 48 bytes
    unsigned char* W1 = lsm + FR_OFF_W;             // layer 1's weights [32][9 taps][16]
    half_t* LUT = reinterpret_cast<half_t*>(lsm + FR_OFF_LUT);     // byte level -> half(level / 255): preprocess2_kernel's last step, tabulated
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    for (int i = tid; i < FR_OFF_S / 16; i += FR_NTH) reinterpret_cast<uint4*>(XL)[i] = make_uint4(0, 0, 0, 0);   // the pad column stays zero
    for (int i = tid; i < 32 * 18; i += FR_NTH) {
        const int row = i / 18, piece = i - row * 18;
        *reinterpret_cast<uint4*>(W1 + row * FR_W1S + piece * 16) = *reinterpret_cast<const uint4*>(a.w_l1 + (size_t)row * a.kpad1 + piece * 8);
    }
    if (tid < 256) LUT[tid] = f2h((float)tid / 255.f);
    const half8 A0 = *reinterpret_cast<const half8*>(a.w_stem + l15 * 64 + 8 * h);
    const half8 A1 = *reinterpret_cast<const half8*>(a.w_stem + l15 * 64 + 32 + 8 * h);
    const float4 bs0 = *reinterpret_cast<const float4*>(a.bs_stem + 4 * h);
    const float4 bs1a = *reinterpret_cast<const float4*>(a.bs_l1 + 4 * h), bs1b = *reinterpret_cast<const float4*>(a.bs_l1 + 16 + 4 * h);
    asm volatile("" ::"v"(bs0.x), "v"(bs0.y), "v"(bs0.z), "v"(bs0.w), "v"(bs1a.x), "v"(bs1a.y), "v"(bs1a.z), "v"(bs1a.w), "v"(bs1b.x),
                 "v"(bs1b.y), "v"(bs1b.z), "v"(bs1b.w));
    const half_t pad114 = f2h(114.f / 255.f);
    auto origin = [&](int t, int& n, int& oy0, int& ox0) {
        const int tx = t % a.tiles_x, r = t / a.tiles_x;
        n = r / a.tiles_y, oy0 = (r % a.tiles_y) * 8, ox0 = tx * 16;
    };
    // fill task k of this thread: row ty = i / 34 of the patch, pixel pair pp = i % 34 -> X columns x, x + 1 with x = 4 ox0 - 4 + 2 pp
    // (even: the pair is 12 contiguous frame bytes of two rows, as in preprocess2_kernel)
    unsigned fr0[FR_TASKS][3], fr1[FR_TASKS][3];
    auto gload = [&](int t) {
        int n, oy0, ox0;
        origin(t, n, oy0, ox0);
        const uint8_t* im = a.bgr + (size_t)n * a.fh * a.fw * 3;
#pragma unroll
        for (int k = 0; k < FR_TASKS; ++k) {
            const int i = tid + k * FR_NTH, ty = i / 34, pp = i - ty * 34;
            const int y = 4 * oy0 - 3 + ty, x = 4 * ox0 - 4 + 2 * pp, yy = y - a.top;
            const bool ok = i < FR_XR * 34 && yy >= 0 && yy < a.nh && x >= 0 && x < a.W;
            const int yc = ok ? yy : 0, xc = ok ? x : 0;
            const unsigned* r0 = reinterpret_cast<const unsigned*>(im + ((size_t)(2 * yc) * a.fw + 2 * xc) * 3);
            const unsigned* r1 = reinterpret_cast<const unsigned*>(im + ((size_t)(2 * yc + 1) * a.fw + 2 * xc) * 3);
            fr0[k][0] = r0[0], fr0[k][1] = r0[1], fr0[k][2] = r0[2], fr1[k][0] = r1[0], fr1[k][1] = r1[1], fr1[k][2] = r1[2];
        }
    };
    int t = blockIdx.x;
    if (t < a.n_tiles) gload(t);
    for (; t < a.n_tiles; t += gridDim.x) {
        progress_prio(t, a.n_tiles);
        int n, oy0, ox0;
        origin(t, n, oy0, ox0);
        __syncthreads();                                            // the previous tile is done with XL / SL (first trip: weights, zeros)
        // ---- network-input patch.  preprocess2_kernel computes floor((p00/2 + p01/2)/2 + (p10/2 + p11/2)/2 + 0.5) in floats, every
        // step exact, i.e. (p00 + p01 + p10 + p11 + 2) >> 2, then half(level / 255): here the four-byte sums are made on packed 16-bit
        // pairs (rows added first) and the division + rounding come from a 256-entry table built with that very expression ------
#pragma unroll
        for (int k = 0; k < FR_TASKS; ++k) {
            const int i = tid + k * FR_NTH, ty = i / 34, pp = i - ty * 34;
            if (i >= FR_XR * 34) continue;
            const int y = 4 * oy0 - 3 + ty, x = 4 * ox0 - 4 + 2 * pp, yy = y - a.top;
            uint2 v0 = make_uint2(0, 0), v1 = make_uint2(0, 0);
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) {           // (x even and W even: both pixels of the pair are inside or outside)
                if (yy >= 0 && yy < a.nh) {
                    // bytes of a row: a = B0 G0 R0 B1 | b = G1 R1 B2 G2 | c = R2 B3 G3 R3; E = (byte 0, byte 2), O = (byte 1, byte 3) of both rows added
                    constexpr unsigned M = 0x00FF00FFu;
                    const unsigned Ea = (fr0[k][0] & M) + (fr1[k][0] & M), Oa = ((fr0[k][0] >> 8) & M) + ((fr1[k][0] >> 8) & M);
                    const unsigned Eb = (fr0[k][1] & M) + (fr1[k][1] & M), Ob = ((fr0[k][1] >> 8) & M) + ((fr1[k][1] >> 8) & M);
                    const unsigned Ec = (fr0[k][2] & M) + (fr1[k][2] & M), Oc = ((fr0[k][2] >> 8) & M) + ((fr1[k][2] >> 8) & M);
                    const unsigned b0 = ((Ea & 0xFFFFu) + (Oa >> 16) + 2u) >> 2, g0 = ((Oa & 0xFFFFu) + (Eb & 0xFFFFu) + 2u) >> 2, r0 = ((Ea >> 16) + (Ob & 0xFFFFu) + 2u) >> 2;
                    const unsigned b1 = ((Eb >> 16) + (Oc & 0xFFFFu) + 2u) >> 2, g1 = ((Ob >> 16) + (Ec >> 16) + 2u) >> 2, r1 = ((Ec & 0xFFFFu) + (Oc >> 16) + 2u) >> 2;
                    const unsigned short* lut = reinterpret_cast<const unsigned short*>(LUT);
                    v0 = make_uint2((unsigned)lut[r0] | ((unsigned)lut[g0] << 16), (unsigned)lut[b0]);              // R G B 0
                    v1 = make_uint2((unsigned)lut[r1] | ((unsigned)lut[g1] << 16), (unsigned)lut[b1]);
                } else {
                    const unsigned p = __builtin_bit_cast(unsigned short, pad114);
                    v0 = v1 = make_uint2(p | (p << 16), p);
                }
            }
            const int lc = 2 * pp - 1;                              // local column of the pair's first pixel (-1: not part of the patch)
            unsigned char* dst = XL + (ty * FR_XC + lc) * 8;
            if (lc >= 0) *reinterpret_cast<uint2*>(dst) = v0;
            *reinterpret_cast<uint2*>(dst + 8) = v1;
        }
        __syncthreads();
        if (t + (int)gridDim.x < a.n_tiles) gload(t + gridDim.x);   // next tile's frame bytes in flight during this tile's MFMAs
        // ---- stem: 17 x 33 outputs in 36 groups of 16 ---------------------------------------------------------------------------
        for (int g = wave; g < 36; g += FR_NTH / 64) {
            const int q = g * 16 + l15, qq = q < FR_SR * FR_SC ? q : FR_SR * FR_SC - 1;
            const int sr = qq / FR_SC, sc = qq - sr * FR_SC;
            const int sy = 2 * oy0 - 1 + sr, sx = 2 * ox0 - 1 + sc;
            const bool inside = (unsigned)sy < (unsigned)(a.H / 2) && (unsigned)sx < (unsigned)(a.W / 2);
            const unsigned char* xb = XL + ((2 * sr) * FR_XC + 2 * sc + 2 * (h & 1)) * 8;
            const half8 B0 = *reinterpret_cast<const half8*>(xb + (h >> 1) * FR_XC * 8);
            const half8 B1 = *reinterpret_cast<const half8*>(xb + 2 * FR_XC * 8);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A0, B0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A1, B1, acc, 0, 0, 0);
            half4 o = make_half4(silu(acc[0] + bs0.x), silu(acc[1] + bs0.y), silu(acc[2] + bs0.z), silu(acc[3] + bs0.w));
            if (!inside) o = half4{(half_t)0, (half_t)0, (half_t)0, (half_t)0};          // layer 1's zero padding
            if (q < FR_SR * FR_SC) *reinterpret_cast<half4*>(SL + q * FR_SPX + 8 * h) = o;
        }
        __syncthreads();
        // ---- layer 1: wave = output row, lane column; nine K = 32 steps with channels 16..31 zero ------------------------------------
        {
            const half8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
            f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
            half8 bv[9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const half8 v = *reinterpret_cast<const half8*>(SL + ((2 * wave + tap / 3) * FR_SC + 2 * l15 + tap % 3) * FR_SPX + 16 * (h & 1));
                bv[tap] = h < 2 ? v : z8;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const half8 w = *reinterpret_cast<const half8*>(W1 + (mt * 16 + l15) * FR_W1S + tap * 32 + 16 * (h & 1));
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(h < 2 ? w : z8, bv[tap], acc[mt], 0, 0, 0);
                }
            }
            const int oy = oy0 + wave, ox = ox0 + l15;
            if (oy < a.Ho && ox < a.Wo) {
                half_t* op = a.out + (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.out_cs + a.out_coff + 4 * h;
                *reinterpret_cast<half4*>(op) = make_half4(silu(acc[0][0] + bs1a.x), silu(acc[0][1] + bs1a.y), silu(acc[0][2] + bs1a.z), silu(acc[0][3] + bs1a.w));
                *reinterpret_cast<half4*>(op + 16) = make_half4(silu(acc[1][0] + bs1b.x), silu(acc[1][1] + bs1b.y), silu(acc[1][2] + bs1b.z), silu(acc[1][3] + bs1b.w));
            }
        }
    }
}

// SPPF's three chained 5x5/stride-1 max-pools (padding -inf) in one pass: pool(pool(x)) is the 9x9 window of x
// and the third the 13x13 one, so all three come from one LDS copy of the map, separably (row maxima of
// radius 2/4/6, then column maxima).  Workgroup = (image, 8-channel slab), thread = pixel, 16-byte accesses.
__device__ __forceinline__ uint4 half8_max(uint4 a, uint4 b) {
    auto mx = [](unsigned u, unsigned v) {                  // v_pk_max_f16
        const half2v r = __builtin_elementwise_max(__builtin_bit_cast(half2v, u), __builtin_bit_cast(half2v, v));
        return __builtin_bit_cast(unsigned, r);
    };
    return make_uint4(mx(a.x, b.x), mx(a.y, b.y), mx(a.z, b.z), mx(a.w, b.w));
}
__global__ void __launch_bounds__(1024) sppf_pools_kernel(const half_t* in, int cs_in, int coff_in, half_t* out, int cs_out,
                                                          int coff_out, int H, int W, int C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pool_smem[];
    uint4* s0 = reinterpret_cast<uint4*>(pool_smem);          // [HW] input
    uint4* s1 = s0 + H * W;                                   // [3][HW] row maxima of radius 2, 4, 6
    const int n = blockIdx.x, c8 = blockIdx.y, t = threadIdx.x, HW = H * W;
    const uint4 NEG = make_uint4(0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u, 0xFC00FC00u);     // half -inf x8
    const int y = t / W, x = t - y * W;
    if (t < HW) s0[t] = *reinterpret_cast<const uint4*>(in + ((size_t)n * HW + t) * cs_in + coff_in + c8 * 8);
    __syncthreads();
    if (t < HW) {
        uint4 m2 = NEG, m4 = NEG, m6 = NEG;
        for (int dx = -6; dx <= 6; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const uint4 v = s0[y * W + xx];
            const int ad = dx < 0 ? -dx : dx;
            m6 = half8_max(m6, v);
            if (ad <= 4) m4 = half8_max(m4, v);
            if (ad <= 2) m2 = half8_max(m2, v);
        }
        s1[t] = m2, s1[HW + t] = m4, s1[2 * HW + t] = m6;
    }
    __syncthreads();
    if (t < HW) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int r = 2 + 2 * k;
            uint4 m = NEG;
            for (int dy = -r; dy <= r; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
                m = half8_max(m, s1[k * HW + yy * W + x]);
            }
            *reinterpret_cast<uint4*>(out + ((size_t)n * HW + t) * cs_out + coff_out + k * C + c8 * 8) = m;
        }
    }
}

__global__ void upsample2_kernel(const half_t* in, int cs_in, int coff_in, half_t* out, int cs_out, int coff_out, int B,
                                 int H, int W, int C) {   // H, W: input size; output 2H x 2W, nearest
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int C8 = C / 8;
    if (i >= B * 4 * H * W * C8) return;
    const int c8 = i % C8, p = i / C8, n = p / (4 * H * W), r = p - n * 4 * H * W, y = r / (2 * W), x = r - y * 2 * W;
    *reinterpret_cast<uint4*>(out + (size_t)p * cs_out + coff_out + c8 * 8) =
        *reinterpret_cast<const uint4*>(in + ((size_t)(n * H + (y >> 1)) * W + (x >> 1)) * cs_in + coff_in + c8 * 8);
}

struct Level { const float* box; const float* cls; int H, W, stride, aoff; };

// DFL expectation + best class; writes candidates of every anchor.  NCT: the class count at compile time (80, the default model:
// the kernel as it was) or 0: `nc` classes in pixels of `ccs` floats (the padded stride), both at run time.
template <int NCT>
__global__ void decode_kernel(Level l0, Level l1, Level l2, int A, int B, float* __restrict__ cbox, float* __restrict__ cconf,
                              int* __restrict__ ccls, int nc, int ccs) {
    const int ncl = NCT ? NCT : nc, cstr = NCT ? NCT : ccs;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * A) return;
    const int n = i / A, a = i - n * A;
    const Level L = a < l1.aoff ? l0 : (a < l2.aoff ? l1 : l2);
    const int q = a - L.aoff, y = q / L.W, x = q - y * L.W;
    const float* bx = L.box + ((size_t)(n * L.H + y) * L.W + x) * 64;
    float d[4];
    for (int s = 0; s < 4; ++s) {
        float mx = -INFINITY;
        for (int j = 0; j < REG_MAX; ++j) mx = fmaxf(mx, bx[s * REG_MAX + j]);
        float sum = 0.f, ex = 0.f;
        for (int j = 0; j < REG_MAX; ++j) {
            const float e = __expf(bx[s * REG_MAX + j] - mx);       // v_exp_f32: arguments in [-|range of the logits|, 0], 1 ulp is far inside the 0.05 px the boxes are held to
            sum += e, ex += e * (float)j;
        }
        d[s] = ex / sum;
    }
    const float ax = (float)x + 0.5f, ay = (float)y + 0.5f, st = (float)L.stride;
    const float* cl = L.cls + ((size_t)(n * L.H + y) * L.W + x) * cstr;
    float best = -INFINITY;
    int bj = 0;
    for (int j = 0; j < ncl; ++j)
        if (cl[j] > best) best = cl[j], bj = j;
    float* o = cbox + (size_t)i * 4;
    o[0] = (ax - d[0]) * st, o[1] = (ay - d[1]) * st, o[2] = (ax + d[2]) * st, o[3] = (ay + d[3]) * st;
    cconf[i] = 1.f / (1.f + expf(-best));
    ccls[i] = bj;
}

// per image: candidates with conf > thres sorted by (conf desc, anchor asc) -> class-offset boxes.
// Stable LSD radix sort in LDS.  A confidence in (thres, 1] has float bits below 0x3F800000 and above 0x3E000000 (thres >= 2^-3 ...
// any positive threshold works: the key is v = 0x3F800000 - bits, ascending v = descending confidence, and the passes cover as
// many 8-bit digits as the largest v needs: three for thresholds >= 2^-1 ... 0.25 gives v < 2^24).  The candidates enter in anchor
// order and every pass is stable, so equal confidences leave in anchor order -- the oracle's tie rule -- without the anchor in the key.
// One pass: elements are dealt round-robin (element i = round 1024 + thread), so inside a round array order = thread order; a
// wave ranks its 64 elements per digit with eight ballots (match-any), the first lane of every digit group stores the group's size
// in cnt[digit][round][wave], an exclusive scan over that table (digit-major) turns sizes into destinations, and the element goes
// to  scan[digit][round][wave] + rank inside its group.  Round 2's bitonic network over 8192 padded 64-bit keys took 67 us (60 us
// with the keys in registers and lane exchanges: 45 of its 91 stages are wave-wide exchanges of eight 64-bit keys).
// DB: digit bits.  LDS = two (key, anchor) images of `cap` = 1024 rounds entries + the table: 8-bit digits fit up to 7 rounds (7168
// anchors), the full 8192 take 7-bit digits (one pass more).
constexpr int RS_ROUNDS = MAX_CAND / 1024;
constexpr size_t rs_lds(int rounds, int db) { return (size_t)2 * rounds * 1024 * 6 + (size_t)(1 << db) * rounds * 16 * 2; }
template <int DB>
__global__ void __launch_bounds__(1024) nms_sort_kernel(int A, int rounds, float conf_thres, const float* __restrict__ cbox,
                                                        const float* __restrict__ cconf, const int* __restrict__ ccls,
                                                        float* __restrict__ sbox, int* __restrict__ sidx, int* __restrict__ scount) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sort_smem[];
    const int cap = rounds * 1024, ncnt = (1 << DB) * rounds * 16;
    unsigned* kv = reinterpret_cast<unsigned*>(sort_smem);                    // [2][cap] keys v (ping-pong)
    unsigned short* ki = reinterpret_cast<unsigned short*>(kv + 2 * cap);     // [2][cap] anchors
    unsigned short* cnt = ki + 2 * cap;                                       // [1 << DB][rounds][16]
    __shared__ unsigned wsum[16];
    __shared__ unsigned s_n, s_vmax;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (tid == 0) s_n = 0, s_vmax = 0;
    __syncthreads();
    // ---- compaction in anchor order: valid candidates -> kv[0], ki[0] -------------------------------------------------------------
    {
        unsigned run = 0, vmax = 0;                                           // candidates are taken in blocks of 1024: block order = anchor order
        float cc[RS_ROUNDS];                                                  // all confidences of this thread first: one exposed load latency, not one per block
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; ++r) cc[r] = (r < rounds && r * 1024 + tid < A) ? cconf[(size_t)n * A + r * 1024 + tid] : 0.f;
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; ++r) {
            if (r >= rounds) break;
            const int i = r * 1024 + tid;
            const float c = cc[r];
            const bool ok = i < A && c > conf_thres && c <= 1.0f;
            const unsigned long long m = __ballot(ok);
            if (lane == 0) wsum[wid] = (unsigned)__popcll(m);
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                const unsigned v = wsum[w];
                before += w < wid ? v : 0u, total += v;
            }
            if (ok) {
                const unsigned pos = run + before + (unsigned)__popcll(m & lt), v = 0x3F800000u - __float_as_uint(c);
                kv[pos] = v, ki[pos] = (unsigned short)i;
                vmax = vmax > v ? vmax : v;
            }
            run += total;
            __syncthreads();
        }
        if (vmax) atomicMax(&s_vmax, vmax);
        if (tid == 0) s_n = run;
        __syncthreads();
    }
    const int cntv = (int)s_n;
    const unsigned vmax = s_vmax;
    int src = 0;
    for (int shift = 0; shift < 32 && (vmax >> shift) != 0; shift += DB) {
        for (int i = tid; i < ncnt / 2; i += 1024) reinterpret_cast<unsigned*>(cnt)[i] = 0;
        __syncthreads();
        const unsigned* sv = kv + src * cap;
        const unsigned short* si = ki + src * cap;
        unsigned ev[RS_ROUNDS], ei[RS_ROUNDS], erank[RS_ROUNDS];
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; ++r) {
            const int i = r * 1024 + tid;
            const bool ok = r < rounds && i < cntv;                            // wave-uniform except in the last partial wave
            ev[r] = ok ? sv[i] : 0u, ei[r] = ok ? si[i] : 0u;
            const unsigned d = (ev[r] >> shift) & ((1u << DB) - 1u);
            unsigned long long peers = __ballot(ok);
#pragma unroll
            for (int bit = 0; bit < DB; ++bit) {
                const bool one = (d >> bit) & 1u;
                const unsigned long long bal = __ballot(one);
                peers &= one ? bal : ~bal;
            }
            erank[r] = (unsigned)__popcll(peers & lt);
            if (ok && erank[r] == 0) cnt[(d * rounds + r) * 16 + wid] = (unsigned short)__popcll(peers);
        }
        __syncthreads();
        // ---- exclusive scan of cnt (digit-major): thread t owns ncnt / 1024 consecutive entries -------------------------------------
        {
            const int per = ncnt >> 10;
            unsigned sum = 0;
            for (int q = 0; q < per; ++q) sum += cnt[tid * per + q];
            unsigned inc = sum;                                                // inclusive scan over the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = (unsigned)__shfl_up((int)inc, off, 64);
                if (lane >= off) inc += o;
            }
            if (lane == 63) wsum[wid] = inc;
            __syncthreads();
            unsigned base = inc - sum;
#pragma unroll
            for (int w = 0; w < 16; ++w) base += w < wid ? wsum[w] : 0u;
            for (int q = 0; q < per; ++q) {
                const unsigned c = cnt[tid * per + q];
                cnt[tid * per + q] = (unsigned short)base, base += c;
            }
        }
        __syncthreads();
        unsigned* dv = kv + (src ^ 1) * cap;
        unsigned short* di = ki + (src ^ 1) * cap;
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; ++r) {
            const int i = r * 1024 + tid;
            if (r < rounds && i < cntv) {
                const unsigned d = (ev[r] >> shift) & ((1u << DB) - 1u);
                const unsigned pos = cnt[(d * rounds + r) * 16 + wid] + erank[r];
                dv[pos] = ev[r], di[pos] = (unsigned short)ei[r];
            }
        }
        src ^= 1;
        __syncthreads();
    }
    const unsigned short* so = ki + src * cap;
    for (int i = tid; i < cntv; i += 1024) {
        const int a = so[i];
        const float off = (float)ccls[(size_t)n * A + a] * 7680.0f;
        const float* bx = cbox + ((size_t)n * A + a) * 4;
        float* o = sbox + ((size_t)n * A + i) * 4;
        o[0] = bx[0] + off, o[1] = bx[1] + off, o[2] = bx[2] + off, o[3] = bx[3] + off;
        sidx[(size_t)n * A + i] = a;
    }
    if (tid == 0) scount[n] = cntv;
}

// Greedy class-aware NMS, one workgroup per image (torchvision.ops.nms semantics on the sorted, class-offset
// boxes).  The sorted boxes sit in LDS; only boxes that are KEPT are ever compared against the rest
// (<= max_det rows of the suppression relation instead of all of it), and the next survivor is found by
// scanning the removed bitmap.  Also maps the kept boxes back to the frame (scale_boxes) and truncation
// is left to the caller (detector.py:111).
__device__ __forceinline__ bool nms_over(const float4 a, float aa, const float4 b, float bb, float thr) {
    // a = the earlier (higher-score) box; same float32 expression and operand order as the oracle
    const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y), xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
    const float inter = fmaxf(xx2 - xx1, 0.f) * fmaxf(yy2 - yy1, 0.f);
    return inter / (aa + bb - inter) > thr;
}

// Greedy NMS over the sorted candidates, one workgroup of NMS_WAVES waves per image.  Candidates are taken 64
// at a time (lane = candidate).  A chunk is tested against the boxes kept so far (kept box k belongs to one wave; boxes
// broadcast from LDS; per-wave survivor masks AND-ed) and then resolves itself in order, in wave 0, with a ballot loop over its
// still-alive members.  The two halves are PIPELINED: while wave 0 resolves chunk c, the other fifteen waves already test chunk
// c + 1 against everything kept BEFORE chunk c; once chunk c's survivors are known, all sixteen test chunk c + 1 against just
// those (at most 64 boxes, four per wave).  Identical decisions to box-at-a-time greedy suppression (a box is dropped iff an
// earlier KEPT box overlaps it); per chunk the critical path is max(resolve, test) + a short increment instead of their sum
// (5 us -> 3.5 us; with random weights ~27 chunks are walked to keep 300 boxes).
constexpr int NMS_WAVES = 16;
__global__ void __launch_bounds__(64 * NMS_WAVES) nms_greedy_kernel(
    int A, int max_det, float iou_thres, const float* __restrict__ sbox, const int* __restrict__ scount,
    const int* __restrict__ sidx, const float* __restrict__ cbox, const float* __restrict__ cconf,
    const int* __restrict__ ccls, float gain, float padx, float pady, float fw, float fh, int* __restrict__ det_n,
    float* __restrict__ det_box, float* __restrict__ det_conf, int* __restrict__ det_cls) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_smem[];
    float4* kbx = reinterpret_cast<float4*>(nms_smem);                      // kept boxes [max_det]
    float* kar = reinterpret_cast<float*>(kbx + max_det);                   // their areas
    int* kix = reinterpret_cast<int*>(kar + max_det);                       // their position in the sorted list
    __shared__ unsigned long long m_old[NMS_WAVES], m_new[NMS_WAVES];       // survivor masks of the chunk wave 0 resolves next
    __shared__ int s_kept;
    const int n = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6, cnt = scount[n];
    const float4* sb = reinterpret_cast<const float4*>(sbox) + (size_t)n * A;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane == 0) m_old[wid] = ~0ull, m_new[wid] = ~0ull;                  // chunk 0: nothing kept yet
    int kept = 0;
    float4 b = lane < cnt ? sb[lane] : zero4;                               // chunk c
    float4 b1 = lane + 64 < cnt ? sb[lane + 64] : zero4;                    // chunk c + 1
    __syncthreads();
    for (int base = 0; base < cnt && kept < max_det; base += 64) {
        const int i = base + lane;
        const float bb = (b.z - b.x) * (b.w - b.y), bb1 = (b1.z - b1.x) * (b1.w - b1.y);
        const float4 b2 = i + 128 < cnt ? sb[i + 128] : zero4;             // chunk c + 2: in flight during this iteration
        unsigned long long early = ~0ull;
        if (wid == 0) {
            // ---- resolve chunk c -----------------------------------------------------------------------------------------------
            unsigned long long m = __ballot(i < cnt);
#pragma unroll
            for (int w = 0; w < NMS_WAVES; ++w) m &= m_old[w] & m_new[w];
            bool alive = (m >> lane) & 1ull;
            unsigned long long todo = m;
            while (todo) {
                const int li = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                float4 a;
                a.x = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(b.x), li));
                a.y = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(b.y), li));
                a.z = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(b.z), li));
                a.w = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(b.w), li));
                const float aa = (a.z - a.x) * (a.w - a.y);
                if (lane > li && alive && nms_over(a, aa, b, bb, iou_thres)) alive = false;
                m = __ballot(alive);
                todo &= m;                       // a member suppressed just now no longer suppresses anyone
            }
            const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
            if (alive && pos < max_det) kbx[pos] = b, kar[pos] = bb, kix[pos] = i;
            int nk = kept + __popcll(m);
            nk = nk > max_det ? max_det : nk;
            if (lane == 0) s_kept = nk;
        } else {
            // ---- meanwhile: chunk c + 1 against everything kept before chunk c (fifteen waves) -------------------------------------------
            bool alive1 = true;
            for (int k = wid - 1; k < kept; k += NMS_WAVES - 1)
                if (nms_over(kbx[k], kar[k], b1, bb1, iou_thres)) alive1 = false;
            early = __ballot(alive1);
        }
        __syncthreads();                         // chunk c's survivors are in kbx; wave 0 is done reading the masks
        const int kept1 = s_kept;
        {   // ---- chunk c + 1 against chunk c's survivors (all waves) ------------------------------------------------------------------
            bool alive1 = true;
            for (int k = kept + wid; k < kept1; k += NMS_WAVES)
                if (nms_over(kbx[k], kar[k], b1, bb1, iou_thres)) alive1 = false;
            const unsigned long long late = __ballot(alive1);
            if (lane == 0) m_old[wid] = early, m_new[wid] = late;
        }
        __syncthreads();
        kept = kept1;
        b = b1, b1 = b2;
    }
    // the detections, all at once (the gathers through sidx would otherwise sit in the chunk loop's critical path)
    for (int pos = threadIdx.x; pos < kept; pos += 64 * NMS_WAVES) {
        const int an = sidx[(size_t)n * A + kix[pos]];
        const float* c = cbox + ((size_t)n * A + an) * 4;
        float* o = det_box + ((size_t)n * max_det + pos) * 4;
        o[0] = fminf(fmaxf((c[0] - padx) / gain, 0.f), fw), o[1] = fminf(fmaxf((c[1] - pady) / gain, 0.f), fh);
        o[2] = fminf(fmaxf((c[2] - padx) / gain, 0.f), fw), o[3] = fminf(fmaxf((c[3] - pady) / gain, 0.f), fh);
        det_conf[(size_t)n * max_det + pos] = cconf[(size_t)n * A + an];
        det_cls[(size_t)n * max_det + pos] = ccls[(size_t)n * A + an];
    }
    if (threadIdx.x == 0) det_n[n] = kept;
}


// ---- reference-precision mode (av_yolo_create_ex(..., AV_YOLO_FP32)) ------------------------------------------------------------
// The reference runs ultralytics on torch float32 (detector.py:103-123).  The production path above takes IEEE-half operands; this
// mode keeps EVERY tensor and weight in float32 and multiplies on v_mfma_f32_16x16x4_f32 (float32 operands, float32 accumulation):
// one generic implicit-GEMM kernel for all 63 convolutions, no fusion, one lane.  It is the checker for the half-precision path
// (tests/test_gpu_yolo.py: maps and logits to 1e-5 of their maximum against the PyTorch-CPU oracle) and a second bench figure.
//
// conv_f32_kernel<MT, NT, CB>: a wave owns 16 MT output channels x 16 NT output pixels (flattened over batch, rows, columns); no LDS:
// a lane's A operand is 4 consecutive input channels of one weight row, its B operand 4 consecutive channels of one input pixel
// (both one 16-byte load from NHWC / [cout][tap][cin] memory), used for 4 MFMA steps.  Within a block of CB = 16 channels step s
// therefore contracts channels {s, 4 + s, 8 + s, 12 + s} -- a permutation of the K order, the same on both operands.  The next
// block's operands are requested before the current block's MFMAs.  CB = 4: the stem (3 image channels + a zero), one step per tap.
struct ConvArgsF {
    const float* in;  int in_cs, in_coff, cin, H, W;
    const float* wgt; const float* bias; int ksz, stride;
    float* out;       int out_cs, out_coff, cout, Ho, Wo;
    const float* res; int res_cs, res_coff;
    int act, npix;
    const float* zeros;          // 16 floats of zeros: what a tap outside the image loads (a select behind the load would make every request wait for its data)
};

template <int MT, int NT, int CB, int D = 2>     // D: operand blocks in flight (a ring of D register buffers, unrolled: indices are compile-time)
__global__ void __launch_bounds__(256) conv_f32_kernel(ConvArgsF a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, kk = lane >> 4;
    const int p0 = ((int)blockIdx.x * 4 + wave) * (16 * NT), co0 = (int)blockIdx.y * (16 * MT);
    if (p0 >= a.npix) return;
    const int taps = a.ksz * a.ksz, pad = a.ksz / 2, K = taps * a.cin;
    int pb[NT], py[NT], px[NT];
    bool pv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int p = p0 + nt * 16 + j;
        pv[nt] = p < a.npix;
        const int q = pv[nt] ? p : 0;
        pb[nt] = q / (a.Ho * a.Wo);
        const int r = q - pb[nt] * a.Ho * a.Wo;
        py[nt] = r / a.Wo, px[nt] = r - py[nt] * a.Wo;
    }
    const float* wrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) wrow[mt] = a.wgt + (size_t)(co0 + mt * 16 + j) * K + (CB == 16 ? 4 * kk : kk);
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nblk = a.cin / CB, steps = taps * nblk;
    f32x4 A[D][MT], Bv[D][NT];
    auto request = [&](int st, int buf) {
        const int tap = st / nblk, c0 = (st - tap * nblk) * CB;
        const int ky = tap / a.ksz, kx = tap - ky * a.ksz;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (CB == 16) A[buf][mt] = *reinterpret_cast<const f32x4*>(wrow[mt] + tap * a.cin + c0);
            else A[buf][mt] = f32x4{wrow[mt][tap * a.cin + c0], 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int iy = py[nt] * a.stride + ky - pad, ix = px[nt] * a.stride + kx - pad;
            const bool inb = pv[nt] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const float* src = inb ? a.in + ((size_t)(pb[nt] * a.H + iy) * a.W + ix) * a.in_cs + a.in_coff + c0 + (CB == 16 ? 4 * kk : kk) : a.zeros;
            if (CB == 16) Bv[buf][nt] = *reinterpret_cast<const f32x4*>(src);
            else Bv[buf][nt] = f32x4{*src, 0.f, 0.f, 0.f};
        }
    };
#pragma unroll
    for (int d = 0; d < D - 1; ++d)
        if (d < steps) request(d, d);
    for (int st0 = 0; st0 < steps; st0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int st = st0 + d;
            if (st + D - 1 < steps) request(st + D - 1, (d + D - 1) % D);      // the block D - 1 steps ahead, into the buffer consumed last trip
            if (st < steps) {
#pragma unroll
                for (int s4 = 0; s4 < (CB == 16 ? 4 : 1); ++s4)
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[d][mt][s4], Bv[d][nt][s4], acc[mt][nt], 0, 0, 0);
            }
        }
    }
    // D[i = 4 (lane / 16) + r][j = lane % 16]: four consecutive output channels of pixel j per lane
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (!pv[nt]) continue;
        const size_t p = (size_t)(p0 + nt * 16 + j);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int co = co0 + mt * 16 + 4 * kk;
            const f32x4 bs = *reinterpret_cast<const f32x4*>(a.bias + co);
            f32x4 v = acc[mt][nt] + bs;
            if (a.act) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] / (1.0f + expf(-v[r]));          // SiLU = x * sigmoid(x)
            }
            if (a.res) v += *reinterpret_cast<const f32x4*>(a.res + p * a.res_cs + a.res_coff + co);
            *reinterpret_cast<f32x4*>(a.out + p * a.out_cs + a.out_coff + co) = v;
        }
    }
}

// conv_gemm_f32_kernel<AR, BR, KC>: the float32 convolutions with 64 / 80 / 128 / 256 output channels as LDS-tiled GEMMs over flattened
// output pixels -- conv_gemm128_kernel's structure with float32 slabs.  A workgroup of four waves owns AR output channels x BR
// pixels (128 x 64: wave = 64 channels x 32 pixels, two across two; 64 x 128 and 80 x 128: every wave all channels x its 32 pixels)
// and walks K in steps of KC = 32 (or 16: cin = 80) channels of one tap through double-buffered LDS slabs (rows of KC floats + 32
// bytes: = 32 mod 64); a step's 16-byte pieces are requested a whole step ahead, before the MFMAs; taps outside the image come from
// the zero page.  MFMA operands: lane group h reads the float4 at channel 4 h of each 16-channel block (ds_read_b128) and uses it for
// four v_mfma_f32_16x16x4_f32 steps -- the same K permutation on both operands as in conv_f32_kernel.
template <int AR, int BR, int KC>
__global__ void __launch_bounds__(256) conv_gemm_f32_kernel(ConvArgsF a) {
    constexpr int ROWB = KC * 4 + 32, PCS = KC / 4;              // bytes per LDS row; 16-byte pieces per row
    constexpr int MT = AR == 128 ? 4 : AR / 16, NT = 2;          // wave tile: 16 MT channels x 32 pixels
    // pieces per thread and step: a divisor of the pieces per row (a thread's pieces stay inside one row); 80 rows use 160 threads
    // (16 / 32 rows: one piece per thread, the first 16 PCS / 32 PCS threads)
    constexpr int NA = AR <= 32 ? 1 : (AR == 64 ? PCS / 4 : PCS / 2), NB = BR == 64 ? PCS / 4 : PCS / 2;
    static_assert(NA >= 1 && NB >= 1 && PCS % NA == 0 && PCS % NB == 0 && AR * PCS <= 256 * NA && BR * PCS == 256 * NB, "staging shape");
    extern __shared__ __attribute__((aligned(16))) unsigned char cgf_smem[];
    unsigned char* As = cgf_smem;                                 // [2][AR rows]
    unsigned char* Bs = cgf_smem + 2 * AR * ROWB;                 // [2][BR rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, h = lane >> 4;
    const int wm = AR == 128 ? (wave & 1) : 0, wn = AR == 128 ? (wave >> 1) : wave;
    const int pix_base = blockIdx.x * BR, ch_base = blockIdx.y * AR;
    const int taps = a.ksz * a.ksz, K = taps * a.cin, pad = a.ksz >> 1;
    // ---- what this thread stages per step: NA pieces of one weight row, NB pieces of one pixel's channels -----------------------
    const int aq0 = tid * NA, arow_s = aq0 / PCS, apc = aq0 - arow_s * PCS;
    const bool a_on = arow_s < AR;
    const float* wsrc = a.wgt + (size_t)(ch_base + (a_on ? arow_s : 0)) * K + apc * 4;
    const int bq0 = tid * NB, brow_s = bq0 / PCS, bpc = bq0 - brow_s * PCS;
    const int sp = pix_base + brow_s;
    const bool spv = sp < a.npix;
    const int spp = spv ? sp : 0;
    const int sn = spp / (a.Ho * a.Wo), sr = spp - sn * a.Ho * a.Wo, soy = sr / a.Wo, sox = sr - soy * a.Wo;
    const int iy0 = soy * a.stride - pad, ix0 = sox * a.stride - pad;
    f32x4 ra[NA], rb[NB];
    const int SPT = a.cin / KC, NSTEP = taps * SPT;
    auto gload = [&](int st) {
        const int tap = st / SPT, part = st - tap * SPT, ky = tap / a.ksz, kx = tap - ky * a.ksz;
        const f32x4* wp = reinterpret_cast<const f32x4*>(wsrc + (size_t)tap * a.cin + part * KC);
#pragma unroll
        for (int q = 0; q < NA; ++q) ra[q] = wp[q];
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = spv && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const float* src = ok ? a.in + ((size_t)(sn * a.H + iy) * a.W + ix) * a.in_cs + a.in_coff + part * KC + bpc * 4 : a.zeros;
        const f32x4* bp = reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int q = 0; q < NB; ++q) rb[q] = bp[ok ? q : 0];              // (zero page: 16 floats)
    };
    auto lstore = [&](int buf) {
        if (a_on) {
            f32x4* da = reinterpret_cast<f32x4*>(As + (size_t)(buf * AR + arow_s) * ROWB + apc * 16);
#pragma unroll
            for (int q = 0; q < NA; ++q) da[q] = ra[q];
        }
        f32x4* db = reinterpret_cast<f32x4*>(Bs + (size_t)(buf * BR + brow_s) * ROWB + bpc * 16);
#pragma unroll
        for (int q = 0; q < NB; ++q) db[q] = rb[q];
    };
    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    gload(0);
    lstore(0);
    if (NSTEP > 1) gload(1);
#pragma unroll 1
    for (int st = 0; st < NSTEP; ++st) {
        __syncthreads();                           // the step's slab is in LDS; the other buffer's readers (step - 1) are done
        const unsigned char* arow = As + (size_t)((st & 1) * AR + wm * 64 + l15) * ROWB + 16 * h;
        const unsigned char* brow = Bs + (size_t)((st & 1) * BR + wn * 32 + l15) * ROWB + 16 * h;
        if (st + 1 < NSTEP) lstore((st + 1) & 1);    // requested a whole step ago
        if (st + 2 < NSTEP) gload(st + 2);           // in flight during this step's MFMAs
#pragma unroll
        for (int c = 0; c < KC / 16; ++c) {
            f32x4 A[MT], B[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) A[mt] = *reinterpret_cast<const f32x4*>(arow + mt * 16 * ROWB + c * 64);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) B[nt] = *reinterpret_cast<const f32x4*>(brow + nt * 16 * ROWB + c * 64);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[mt][s4], B[nt][s4], acc[mt][nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int pi = pix_base + wn * 32 + nt * 16 + l15;
        if (pi >= a.npix) continue;
        const size_t p = (size_t)pi;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int co = ch_base + wm * 64 + mt * 16 + 4 * h;
            f32x4 v = acc[mt][nt] + *reinterpret_cast<const f32x4*>(a.bias + co);
            if (a.act) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] / (1.0f + expf(-v[r]));          // SiLU = x * sigmoid(x)
            }
            if (a.res) v += *reinterpret_cast<const f32x4*>(a.res + p * a.res_cs + a.res_coff + co);
            *reinterpret_cast<f32x4*>(a.out + p * a.out_cs + a.out_coff + co) = v;
        }
    }
}

// letterbox + bilinear resize + BGR -> RGB + / 255 -> NHWC4 float (channel 3 zero), [B][H][W][4]: preprocess_kernel's arithmetic
__global__ void preprocess_f32_kernel(const uint8_t* __restrict__ bgr, int B, int h, int w, int H, int W, int nh, int nw,
                                      int top, int left, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H * W) return;
    const int n = i / (H * W), r = i - n * H * W, y = r / W, x = r - y * W;
    float c[3] = {114.f, 114.f, 114.f};
    const int yy = y - top, xx = x - left;
    if (yy >= 0 && yy < nh && xx >= 0 && xx < nw) {
        // source coordinates in double, as the oracle computes them (oracle/yolo_ref.py: preprocess): in float they are off by up to 4e-5 at a
        // generic scale, which moved 1 value in 4 000 of a 90 x 333 frame to the neighbouring uint8 level
        const double sy = ((double)yy + 0.5) * ((double)h / (double)nh) - 0.5, sx = ((double)xx + 0.5) * ((double)w / (double)nw) - 0.5;
        const double fy = floor(sy), fx = floor(sx);
        const float wy = (float)(sy - fy), wx = (float)(sx - fx);
        int y0 = (int)fy, x0 = (int)fx, y1 = y0 + 1, x1 = x0 + 1;
        y0 = y0 < 0 ? 0 : (y0 > h - 1 ? h - 1 : y0), y1 = y1 < 0 ? 0 : (y1 > h - 1 ? h - 1 : y1);
        x0 = x0 < 0 ? 0 : (x0 > w - 1 ? w - 1 : x0), x1 = x1 < 0 ? 0 : (x1 > w - 1 ? w - 1 : x1);
        const uint8_t* im = bgr + (size_t)n * h * w * 3;
        for (int q = 0; q < 3; ++q) {
            const float p00 = im[((size_t)y0 * w + x0) * 3 + q], p01 = im[((size_t)y0 * w + x1) * 3 + q];
            const float p10 = im[((size_t)y1 * w + x0) * 3 + q], p11 = im[((size_t)y1 * w + x1) * 3 + q];
            const float ta = p00 * (1.f - wx) + p01 * wx, tb = p10 * (1.f - wx) + p11 * wx;
            c[q] = floorf(ta * (1.f - wy) + tb * wy + 0.5f);
        }
    }
    *reinterpret_cast<f32x4*>(out + (size_t)i * 4) = f32x4{c[2] / 255.f, c[1] / 255.f, c[0] / 255.f, 0.f};   // RGB
}

__global__ void maxpool5_f32_kernel(const float* in, int cs_in, int coff_in, float* out, int cs_out, int coff_out, int B, int H, int W, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H * W * C) return;
    const int c = i % C, p = i / C, n = p / (H * W), r = p - n * H * W, y = r / W, x = r - y * W;
    float m = -INFINITY;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            m = fmaxf(m, in[((size_t)(n * H + yy) * W + xx) * cs_in + coff_in + c]);
        }
    out[(size_t)p * cs_out + coff_out + c] = m;
}

__global__ void upsample2_f32_kernel(const float* in, int cs_in, int coff_in, float* out, int cs_out, int coff_out, int B, int H, int W, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // H, W: input size; output 2H x 2W, nearest
    const int C4 = C / 4;
    if (i >= B * 4 * H * W * C4) return;
    const int c4 = i % C4, p = i / C4, n = p / (4 * H * W), r = p - n * 4 * H * W, y = r / (2 * W), x = r - y * 2 * W;
    *reinterpret_cast<f32x4*>(out + (size_t)p * cs_out + coff_out + c4 * 4) =
        *reinterpret_cast<const f32x4*>(in + ((size_t)(n * H + (y >> 1)) * W + (x >> 1)) * cs_in + coff_in + c4 * 4);
}

// ---- host side: graph of layers --------------------------------------------------------------------------------

struct Buf { half_t* p = nullptr; int C = 0, H = 0, W = 0; };     // (reference-precision mode: the same pointer holds float elements)
struct Slice { int buf, coff, c, real = 0; };     // c channels as allocated / as the kernels see them; real (0: = c): how many of them the model has,
// the rest being the zero padding of a class branch whose width is no multiple of 16

enum OpKind { OP_CONV, OP_STEM, OP_POOLS, OP_MAXPOOL, OP_UPSAMPLE, OP_CONV_F32 };     // OP_POOLS: SPPF's three pools in one launch (half); OP_MAXPOOL: one of them (float32)

// Test hooks from the environment, read once per forward (tests/test_gpu_yolo.py flips them between two forwards of one handle to
// pin a fast kernel bit for bit against a generic one).  They are the only environment this file reads.
struct Hooks {
    bool no_fuse, generic80, no_gemm, no_gemm_1x1, generic_pre;
    bool operator==(const Hooks& o) const { return memcmp(this, &o, sizeof o) == 0; }
};
Hooks read_hooks() {
    Hooks h;
    h.no_fuse = getenv("AVHOT_YOLO_NO_FUSE") != nullptr;            // one launch per layer: no front / C2f fusion, no virtual Upsample + Concat
    h.generic80 = getenv("AVHOT_CONV_GENERIC80") != nullptr;        // the cin = 80 layers on the generic kernels
    h.no_gemm = getenv("AVHOT_CONV_NO_GEMM") != nullptr;            // no conv_gemm128_kernel at all
    h.no_gemm_1x1 = getenv("AVHOT_CONV_NO_GEMM_1X1") != nullptr;    // no conv_gemm128_kernel for the 1x1 layers
    h.generic_pre = getenv("AVHOT_YOLO_GENERIC_PRE") != nullptr;    // preprocess_kernel for every frame shape
    return h;
}

// Every kernel instantiation that a launch is chosen from or that needs more dynamic LDS than the default 64 KB: the choosers below
// find their kernel here and nowhere else, and av_yolo_create_ex raises the limits from the same rows -- so a variant that is not
// listed cannot be launched, and a listed one has its limit.  lds_limit 0: the default is enough.
enum Family { K_MFMA, K_GEMM128, K_LDS, K_WS3, K_WS1, K_GEMM_F32, K_STEM_F32, K_FIXED };     // K_FIXED: launched by name from one place
struct Variant { Family fam; int p[6]; const void* fn; int lds_limit; };
#define AV_KT(fam, limit, kernel, ...) {fam, {__VA_ARGS__}, reinterpret_cast<const void*>(&kernel<__VA_ARGS__>), limit}
#define AV_K(limit, kernel) {K_FIXED, {}, reinterpret_cast<const void*>(&kernel), limit}
const Variant kVariants[] = {
    // generic fallback, any shape
    AV_KT(K_MFMA, 0, conv_mfma_kernel, 2, 2), AV_KT(K_MFMA, 0, conv_mfma_kernel, 4, 2), AV_KT(K_MFMA, 0, conv_mfma_kernel, 5, 2),
    AV_KT(K_MFMA, 0, conv_mfma_kernel, 1, 2), AV_KT(K_MFMA, 0, conv_mfma_kernel, 3, 2),
    {K_GEMM128, {}, reinterpret_cast<const void*>(&conv_gemm128_kernel), 160 * 1024},
    // <MT, KS>
    AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 4, 1), AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 4, 3), AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 5, 3),
    // the widths of scales s and m and of padded class branches: 16-, 32-, 48- and 80-channel tiles; <MT, KS, S>: stride 2
    AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 1, 1), AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 2, 1), AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 3, 1),
    AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 5, 1), AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 1, 3), AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 2, 3),
    AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 3, 3), AV_KT(K_LDS, 100 * 1024, conv_lds_kernel, 4, 3, 2),
    // <MT, NT, NW, CINP, RES, S>: stride 1 with 8 or 16 tile rows, with and without residual; stride 2
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 1, 1, 8, 32, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 1, 1, 8, 32, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 1, 2, 8, 32, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 1, 2, 8, 32, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 2, 1, 8, 32, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 2, 1, 8, 32, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 2, 2, 8, 32, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 2, 2, 8, 32, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 4, 1, 8, 64, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 4, 1, 8, 64, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 4, 2, 8, 64, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 4, 2, 8, 64, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 5, 1, 8, 64, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 5, 2, 8, 64, false, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 5, 1, 8, 80, false, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 2, 1, 8, 32, false, 2), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 4, 1, 8, 32, false, 2),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 4, 1, 8, 64, false, 2),
    // 48-channel tiles (scale m): the 48 -> 48 bottlenecks of layer 2, layer 1 (48 -> 96, stride 2)
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 3, 1, 8, 64, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 3, 1, 8, 64, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 3, 2, 8, 64, false, 1), AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 3, 2, 8, 64, true, 1),
    AV_KT(K_WS3, 160 * 1024, conv3x3_ws_kernel, 3, 1, 8, 64, false, 2),
    // <MT, KS, TAIL16, DEC>: the head's last box / class convolutions with the decode in their epilogue, then the plain ones
    AV_KT(K_WS1, 0, conv1x1_ws_kernel, 4, 2, false, 1), AV_KT(K_WS1, 0, conv1x1_ws_kernel, 5, 2, true, 2),
    AV_KT(K_WS1, 0, conv1x1_ws_kernel, 5, 2, true, 0),      // 80 -> 80 without an epilogue: scale n with nc = 65 .. 79 (hc = nc, both padded to 80)
    // DEC = 3, the class decode with nc at run time: hc = 64 (scale n, nc <= 32), 128 (s) and 192 (m) with nc <= 16 or 65 .. 80
    AV_KT(K_WS1, 0, conv1x1_ws_kernel, 1, 2, false, 3), AV_KT(K_WS1, 0, conv1x1_ws_kernel, 2, 2, false, 3),
    AV_KT(K_WS1, 0, conv1x1_ws_kernel, 1, 4, false, 3), AV_KT(K_WS1, 0, conv1x1_ws_kernel, 5, 4, false, 3),
    AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 1, 6, false, 3), AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 5, 6, false, 3),
    AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 2, 1, false, 0), AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 4, 2, false, 0),
    AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 4, 3, false, 0), AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 4, 4, false, 0),
    AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 4, 6, false, 0), AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 4, 8, false, 0),
    AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 4, 12, false, 0), AV_KT(K_WS1, 100 * 1024, conv1x1_ws_kernel, 4, 16, false, 0),
    // float32 chain <AR, BR, KC>; its stem <MT, NT, CB, D>
    AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 128, 64, 32), AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 64, 128, 32),
    AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 80, 128, 32), AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 80, 128, 16),
    AV_KT(K_GEMM_F32, 0, conv_gemm_f32_kernel, 32, 128, 32), AV_KT(K_GEMM_F32, 0, conv_gemm_f32_kernel, 32, 128, 16),
    AV_KT(K_GEMM_F32, 0, conv_gemm_f32_kernel, 16, 128, 16), AV_KT(K_GEMM_F32, 0, conv_gemm_f32_kernel, 16, 128, 32),
    AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 48, 128, 32), AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 48, 128, 16),
    // cin = 112 (scale n with nc > 96: hc padded to 112) into 128- / 256- and 192-wide padded class counts
    AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 128, 64, 16), AV_KT(K_GEMM_F32, 100 * 1024, conv_gemm_f32_kernel, 64, 128, 16),
    AV_KT(K_STEM_F32, 0, conv_f32_kernel, 1, 1, 4, 2), AV_KT(K_STEM_F32, 0, conv_f32_kernel, 1, 2, 4, 2), AV_KT(K_STEM_F32, 0, conv_f32_kernel, 1, 4, 4, 2),
    AV_K(0, stem_conv_kernel<false>), AV_K(0, stem_conv_kernel<true>), AV_K(0, decode_kernel<NC>), AV_K(0, decode_kernel<0>),
    AV_K(C2F_LDS, c2f16_fused_kernel), AV_K(FR_LDS, front_fused_kernel), AV_K(F32H_LDS, c2f32_head_kernel),
    AV_K(f32t_lds(96), (c2f32_tail_kernel<96, true>)), AV_K(f32t_lds(64), (c2f32_tail_kernel<64, false>)),
    AV_K((int)rs_lds(7, 8), nms_sort_kernel<8>), AV_K((int)rs_lds(8, 7), nms_sort_kernel<7>),
};
#undef AV_KT
#undef AV_K

const Variant* find_variant(Family fam, const int (&p)[6]) {
    for (const Variant& v : kVariants)
        if (v.fam == fam && std::equal(p, p + 6, v.p)) return &v;
    return nullptr;
}

// One launch of the network part of a forward: the kernel's address, the launch dimensions and the kernel's parameters by value, in
// its order, the way hipLaunchKernel takes them.
enum When { ALWAYS, BGR_ALIGNED, BGR_UNALIGNED };      // the frame pointer's 4-byte alignment is the one input to a choice that a call brings
template <typename T> struct as_is { using type = T; };
struct Step {
    const void* fn = nullptr;
    dim3 grid, block;
    size_t lds = 0;
    When when = ALWAYS;
    int lane = 0;                        // 1: the side stream
    bool head = false;                   // the Detect head begins here: everything before it is one dependency chain
    bool takes_bgr = false;              // the kernel's first parameter begins with the frame pointer, which every call brings
    int fam = K_FIXED, var[6] = {0, 0, 0, 0, 0, 0}, first_op = 0, n_ops = 0;       // what av_yolo_plan_step reports
    alignas(16) unsigned char params[384];
    int off[12], nargs = 0;
    template <typename... A>
    void args(const A&... a) {
        static_assert((sizeof(A) + ... + 0) + 16 * sizeof...(A) <= sizeof(Step::params) && sizeof...(A) <= 12, "parameters fit");
        size_t pos = 0;
        nargs = 0;
        auto put = [&](const auto& v) {
            static_assert(std::is_trivially_copyable<std::decay_t<decltype(v)>>::value, "kernel parameters are plain data");
            pos = (pos + alignof(decltype(v)) - 1) / alignof(decltype(v)) * alignof(decltype(v));
            memcpy(params + pos, &v, sizeof v);
            off[nargs++] = (int)pos, pos += sizeof v;
        };
        (put(a), ...);
    }
    // a kernel known by name: the parameters are converted to its own types, as a <<< >>> launch would
    template <typename... P>
    void kernel(void (*k)(P...), dim3 g, dim3 b, size_t l, const typename as_is<P>::type&... a) {
        fn = reinterpret_cast<const void*>(k), grid = g, block = b, lds = l;
        args<P...>(a...);
    }
};

struct Yolo {
    av_ctx* ctx = nullptr;
    av_yolo_model model{};
    int ncp = 0;                         // floats per pixel of the class logits: nc rounded up to a multiple of 16
    int B = 0, inH = 0, inW = 0, H = 0, W = 0, nh = 0, nw = 0, top = 0, left = 0, A = 0, words = 0;
    float gain = 1.f;
    std::vector<Buf> bufs;
    float* f32_zeros = nullptr;
    bool f32 = false;                    // reference-precision mode: float32 tensors and weights, conv_gemm_f32_kernel, no fusion
    struct Op { OpKind kind; ConvArgs ca; ConvArgsF cf; int mt; int cout_real = 0; Slice in, out; int H, W, C; int lane = 0; int fuse = 0; int dec = 0, dec_level = 0; int vcat = -1; };   // lane 1: internal side stream;
    // vcat >= 0 (an upsample op): op index of the 1x1 convolution that can read this upsample's source directly (virtual Upsample + Concat);
    // fuse 1: this op and the next three are a C2f block c2f16_fused_kernel can run in one launch; 2 / 3: 32-channel blocks (c2f32_*); dec 1 / 2: the head's last box /
    // class convolution of level dec_level (its epilogue can do the decode)
    hipStream_t side = nullptr;          // the Detect head's class branches run beside its box branches
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // deferred tail (throughput mode): decode + sort + NMS of forward k run on their own stream beside the convolutions
    // of forward k+1 -- they occupy one workgroup per image and ~0.25 ms, the latency-bound end of an otherwise
    // chip-wide chain.  Outputs are complete after av_yolo_join_tail().
    hipStream_t tail = nullptr;
    hipEvent_t ev_heads = nullptr, ev_tail = nullptr;
    bool defer_tail = false, tail_pending = false;
    bool keep_logits = false;            // test hook: also write the float32 head logits and run decode_kernel on them
    int dbg_cat = -1;                    // test hook: layer 4's concat buffer (tensor id 40)
    int head_begin = -1;                 // first op of the head
    std::vector<Op> ops;
    // the launches of a forward, and what they were planned for: rebuilt only when a hook or keep_logits changes
    std::vector<Step> plan;
    Hooks plan_hooks{};
    bool plan_keep_logits = false;
    bool decode_alone = false;           // the plan has no decode epilogue: decode_kernel makes the candidates (plan_forward)
    std::vector<void*> allocs;
    float* head_box[3] = {nullptr, nullptr, nullptr};
    float* head_cls[3] = {nullptr, nullptr, nullptr};
    int lvH[3], lvW[3];
    float *cbox = nullptr, *cconf = nullptr, *sbox = nullptr, *dbg_cbox = nullptr, *dbg_cconf = nullptr;
    int *ccls = nullptr, *sidx = nullptr, *scount = nullptr, *dbg_ccls = nullptr;
    unsigned long long* mask = nullptr;
    const float* wsrc = nullptr;
    size_t wpos = 0, wtotal = 0;
    std::vector<std::pair<int, Slice>> named;       // test hooks: tensor id -> slice
};

bool dev_alloc(Yolo& y, void** p, size_t bytes) {
    if (hipMalloc(p, bytes) != hipSuccess) return false;
    (void)hipMemset(*p, 0, bytes);
    y.allocs.push_back(*p);
    return true;
}

template <typename T>
T* upload(Yolo& y, const std::vector<T>& v) {
    T* d;
    if (!dev_alloc(y, (void**)&d, v.size() * sizeof(T))) return nullptr;
    (void)hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}

int new_buf(Yolo& y, int H, int W, int C) {
    Buf b;
    b.C = C, b.H = H, b.W = W;
    if (!dev_alloc(y, (void**)&b.p, (size_t)y.B * H * W * C * (y.f32 ? sizeof(float) : sizeof(half_t)))) return -1;
    y.bufs.push_back(b);
    return (int)y.bufs.size() - 1;
}

// the next nw weights and their bias (cout values) or BatchNorm parameters (4 cout) from the parameter blob
bool take_params(Yolo& y, size_t nw, int cout, bool bn_act, const float*& w, const float*& bp) {
    const size_t nb = bn_act ? 4 * (size_t)cout : (size_t)cout;
    if (y.wpos + nw + nb > y.wtotal) return false;
    w = y.wsrc + y.wpos, bp = w + nw;
    y.wpos += nw + nb;
    return true;
}

// BatchNorm (eval) of output channel co as a scale of its weights and a bias, in float32 as ultralytics' fuse() does; a layer
// without BatchNorm has a plain bias
void fold_bn(const float* bp, int cout, bool bn_act, int co, float& scale, float& shift) {
    scale = 1.f, shift = bp[co];
    if (bn_act) {
        const float g = bp[co], be = bp[cout + co], mu = bp[2 * cout + co], var = bp[3 * cout + co];
        scale = g / std::sqrt(var + 1e-3f);
        shift = be - mu * scale;
    }
}

// 16-channel tiles per workgroup for `cout` output channels (a multiple of 16): 64-, 80-, 48-, 32-, then 16-wide
int mt_of(int cout) { return (cout % 64 == 0) ? 4 : ((cout % 80 == 0) ? 5 : ((cout % 48 == 0) ? 3 : ((cout % 32 == 0) ? 2 : 1))); }
int pad16(int c) { return (c + 15) & ~15; }
int real_of(Slice s) { return s.real ? s.real : s.c; }

// what ConvArgs and ConvArgsF share: input, output and residual slices (an `out` without a buffer: the caller sets the output), sizes
template <typename Args>
void conv_geometry(const Yolo& y, Args& a, Slice in, Slice out, int k, int s, bool bn_act, const Slice* res) {
    using T = std::remove_pointer_t<decltype(a.out)>;
    auto at = [&](int buf) { return reinterpret_cast<T*>(y.bufs[buf].p); };
    const Buf& bi = y.bufs[in.buf];
    a.in = at(in.buf), a.in_cs = bi.C, a.in_coff = in.coff, a.cin = in.c, a.H = bi.H, a.W = bi.W;
    a.ksz = k, a.stride = s, a.cout = out.c;
    a.Ho = (bi.H + 2 * (k / 2) - k) / s + 1, a.Wo = (bi.W + 2 * (k / 2) - k) / s + 1;
    if (out.buf >= 0) a.out = at(out.buf), a.out_cs = y.bufs[out.buf].C, a.out_coff = out.coff;
    if (res) a.res = at(res->buf), a.res_cs = y.bufs[res->buf].C, a.res_coff = res->coff;
    a.act = bn_act ? 1 : 0, a.npix = y.B * a.Ho * a.Wo;
}

// consumes one conv's parameters, folds BN, uploads half [cout][kpad] + f32 bias, appends the op
bool add_conv_half(Yolo& y, Slice in, Slice out, int k, int s, bool bn_act, float* out32, int out32_cs, const Slice* res) {
    const int cin = in.c, cout = out.c, taps = k * k, cin_r = real_of(in), cout_r = real_of(out);      // (padding: zero filters, zero biases, zero columns)
    const int kreal = taps * cin, kpad = (kreal + 31) & ~31;
    const float *w, *bp;
    if (!take_params(y, (size_t)cout_r * cin_r * taps, cout_r, bn_act, w, bp)) return false;
    std::vector<half_t> wb((size_t)cout * kpad, (half_t)0);
    std::vector<float> bias(cout, 0.f);
    for (int co = 0; co < cout_r; ++co) {
        float scale;
        fold_bn(bp, cout_r, bn_act, co, scale, bias[co]);
        for (int ci = 0; ci < cin_r; ++ci)
            for (int t = 0; t < taps; ++t)
                wb[(size_t)co * kpad + t * cin + ci] = f2h(w[((size_t)co * cin_r + ci) * taps + t] * scale);
    }
    const half_t* dw = upload(y, wb);
    const float* db = upload(y, bias);
    if (!dw || !db) return false;
    Yolo::Op op{};
    op.kind = OP_CONV;
    ConvArgs& a = op.ca;
    conv_geometry(y, a, in, out, k, s, bn_act, res);
    a.wgt = dw, a.bias = db, a.kpad = kpad, a.kreal = kreal;
    if (out32) a.out = nullptr, a.out32 = out32, a.out_cs = out32_cs, a.out_coff = 0;
    op.mt = mt_of(cout), op.cout_real = cout_r;
    y.ops.push_back(op);
    return true;
}

// the same for the reference-precision chain: float32 weights [cout][tap][cin]; an input of 4 channels whose parameters have 3 (the
// stem) gets a zero fourth channel
bool add_conv_f32(Yolo& y, Slice in, Slice out, int k, int s, bool bn_act, float* out32, int out32_cs, const Slice* res) {
    const int cin = in.c, cout = out.c, taps = k * k, cout_r = real_of(out);
    const int cin_w = (cin == 4 && k == 3 && s == 2 && y.ops.empty()) ? 3 : real_of(in);
    const float *w, *bp;
    if (!take_params(y, (size_t)cout_r * cin_w * taps, cout_r, bn_act, w, bp)) return false;
    std::vector<float> wf((size_t)cout * taps * cin, 0.f), bias(cout, 0.f);
    for (int co = 0; co < cout_r; ++co) {
        float scale;
        fold_bn(bp, cout_r, bn_act, co, scale, bias[co]);
        for (int ci = 0; ci < cin_w; ++ci)
            for (int t = 0; t < taps; ++t) wf[((size_t)co * taps + t) * cin + ci] = w[((size_t)co * cin_w + ci) * taps + t] * scale;
    }
    const float* dw = upload(y, wf);
    const float* db = upload(y, bias);
    if (!dw || !db) return false;
    Yolo::Op op{};
    op.kind = OP_CONV_F32;
    ConvArgsF& a = op.cf;
    conv_geometry(y, a, in, out, k, s, bn_act, res);
    a.wgt = dw, a.bias = db;
    if (out32) a.out = out32, a.out_cs = out32_cs, a.out_coff = 0;
    if (!y.f32_zeros && !dev_alloc(y, (void**)&y.f32_zeros, 64)) return false;      // (dev_alloc clears)
    a.zeros = y.f32_zeros;
    op.mt = mt_of(cout), op.cout_real = cout_r;
    y.ops.push_back(op);
    return true;
}

bool add_conv(Yolo& y, Slice in, Slice out, int k, int s, bool bn_act, float* out32, int out32_cs, const Slice* res) {
    return y.f32 ? add_conv_f32(y, in, out, k, s, bn_act, out32, out32_cs, res) : add_conv_half(y, in, out, k, s, bn_act, out32, out32_cs, res);
}

// the stem's parameters (Conv 3 -> ch[0], k3 s2, BN, SiLU) packed for stem_conv_kernel: half [cout][64], k = ky*16 + kx*4 + c
bool add_stem(Yolo& y, Slice in, Slice out) {
    const int cout = out.c, cin_real = 3, taps = 9;
    const float *w, *bp;
    if (cout % 16 || !take_params(y, (size_t)cout * cin_real * taps, cout, true, w, bp)) return false;
    std::vector<half_t> wb((size_t)cout * 64, (half_t)0);
    std::vector<float> bias(cout);
    for (int co = 0; co < cout; ++co) {
        float scale;
        fold_bn(bp, cout, true, co, scale, bias[co]);
        for (int ci = 0; ci < cin_real; ++ci)
            for (int t = 0; t < taps; ++t)
                wb[(size_t)co * 64 + (t / 3) * 16 + (t % 3) * 4 + ci] = f2h(w[((size_t)co * cin_real + ci) * taps + t] * scale);
    }
    const half_t* dw = upload(y, wb);
    const float* db = upload(y, bias);
    if (!dw || !db) return false;
    Yolo::Op op{};
    op.kind = OP_STEM;
    ConvArgs& a = op.ca;
    a.in = y.bufs[in.buf].p, a.in_cs = 4, a.in_coff = 0, a.cin = 4, a.H = y.H, a.W = y.W;      // H, W: without the frame
    a.wgt = dw, a.bias = db, a.kpad = 64, a.kreal = 27, a.ksz = 3, a.stride = 2;
    a.Ho = (y.H - 1) / 2 + 1, a.Wo = (y.W - 1) / 2 + 1;
    a.out = y.bufs[out.buf].p, a.out32 = nullptr, a.out_cs = y.bufs[out.buf].C, a.out_coff = out.coff;
    a.cout = cout, a.res = nullptr, a.res_cs = 0, a.res_coff = 0, a.act = 1, a.npix = y.B * a.Ho * a.Wo;
    op.mt = 1, op.cout_real = cout;
    y.ops.push_back(op);
    return true;
}

// C2f(c1 -> c2, n, shortcut): input slice `in`, output slice `out`; allocates its concat + temp buffers
bool add_c2f(Yolo& y, Slice in, Slice out, int n, bool shortcut) {
    const Buf& bi = y.bufs[in.buf];
    const int c = out.c / 2, H = bi.H, W = bi.W;
    const int cat = new_buf(y, H, W, (2 + n) * c);
    if (cat < 0) return false;
    const size_t first = y.ops.size();
    if (!add_conv(y, in, Slice{cat, 0, 2 * c}, 1, 1, true, nullptr, 0, nullptr)) return false;
    for (int i = 0; i < n; ++i) {
        // a temp buffer per bottleneck (not one per block): after a forward with one launch per layer every op's input is still in
        // memory, which av_yolo_op's readers rely on.  Two blocks have n = 2 (layers 4 and 6): 2 c H W more bytes per image each,
        // 360 KB per 384 x 640 image together; the fused kernels keep this map in LDS and never touch the buffers.
        const int tmp = new_buf(y, H, W, c);
        if (tmp < 0) return false;
        const Slice src{cat, (1 + i) * c, c}, dst{cat, (2 + i) * c, c};
        if (!add_conv(y, src, Slice{tmp, 0, c}, 3, 1, true, nullptr, 0, nullptr)) return false;
        if (!add_conv(y, Slice{tmp, 0, c}, dst, 3, 1, true, nullptr, 0, shortcut ? &src : nullptr)) return false;
    }
    if (!add_conv(y, Slice{cat, 0, (2 + n) * c}, out, 1, 1, true, nullptr, 0, nullptr)) return false;
    if (c == 16 && n == 1 && shortcut && in.c == 32 && out.c == 32) y.ops[first].fuse = 1;
    if (c == 32 && n == 2 && shortcut && in.c == 64 && out.c == 64) y.ops[first].fuse = 2, y.dbg_cat = cat;        // c2f32_head_kernel + c2f32_tail_kernel<96, true>
    if (c == 32 && n == 1 && !shortcut && out.c == 64) y.ops[first].fuse = 3;                      // cv1 as it is + c2f32_tail_kernel<64, false>
    return true;
}

void add_simple(Yolo& y, OpKind kind, Slice in, Slice out, int H, int W, int C) {
    Yolo::Op op{};
    op.kind = kind, op.in = in, op.out = out, op.H = H, op.W = W, op.C = C;
    y.ops.push_back(op);
}

void letterbox(int h, int w, float& r, int& nh, int& nw, int& top, int& left, int& H, int& W) {
    const int nsz = 640, stride = 32;
    r = std::fmin((float)nsz / h, (float)nsz / w);
    nh = (int)std::lround((double)h * r), nw = (int)std::lround((double)w * r);
    const int dw = (nsz - nw) % stride, dh = (nsz - nh) % stride;
    top = (int)std::lround(dh / 2.0 - 0.1), left = (int)std::lround(dw / 2.0 - 0.1);
    const int bottom = (int)std::lround(dh / 2.0 + 0.1), right = (int)std::lround(dw / 2.0 + 0.1);
    H = nh + top + bottom, W = nw + left + right;
}

// buffers, parameters and ops of the whole network, from the model alone (yolov8.yaml layer numbers in the margin): c1..c5 the stage
// widths, a concat buffer per Concat with its producers writing their slices in place
int build_graph(Yolo& y) {
    bool ok = true;
    const av_yolo_model& m = y.model;
    const int H = y.H, W = y.W, batch = y.B;
    const int c1 = m.ch[0], c2 = m.ch[1], c3 = m.ch[2], c4 = m.ch[3], c5 = m.ch[4], nr = m.neck_rep, nc = m.nc, cs = c5 / 2;
    const int hb = std::max(16, std::max(c3 / 4, 4 * REG_MAX)), hc = std::max(c3, std::min(nc, 100));      // Detect's hidden widths
    const int hcp = pad16(hc), ncp = pad16(nc);
    y.ncp = ncp;
    auto nb = [&](int hh, int ww, int c) { const int b = new_buf(y, hh, ww, c); ok = ok && b >= 0; return b; };
    const int x0 = y.f32 ? nb(H, W, 4) : nb(H + 2, W + 2, 4), b0 = nb(H / 2, W / 2, c1), b1 = nb(H / 4, W / 4, c2), b2 = nb(H / 4, W / 4, c2);
    const int cat14 = nb(H / 8, W / 8, c4 + c3), cat11 = nb(H / 16, W / 16, c5 + c4), cat20 = nb(H / 32, W / 32, c4 + c5);
    const int cat17 = nb(H / 16, W / 16, c3 + c4);
    const int b3 = nb(H / 8, W / 8, c3), b5 = nb(H / 16, W / 16, c4), b7 = nb(H / 32, W / 32, c5), b8 = nb(H / 32, W / 32, c5);
    const int spp = nb(H / 32, W / 32, 4 * cs), p3 = nb(H / 8, W / 8, c3), p4 = nb(H / 16, W / 16, c4), p5 = nb(H / 32, W / 32, c5);
    AV_REQUIRE(ok, AV_ENOMEM, "av_yolo_create: device allocation failed");
#define CV(...) ok = ok && add_conv(y, __VA_ARGS__)
    if (y.f32) CV(Slice{x0, 0, 4}, Slice{b0, 0, c1}, 3, 2, true, nullptr, 0, nullptr);           // 0 (4-channel input, fourth channel zero)
    else ok = ok && add_stem(y, Slice{x0, 0, 4}, Slice{b0, 0, c1});                               // 0
    CV(Slice{b0, 0, c1}, Slice{b1, 0, c2}, 3, 2, true, nullptr, 0, nullptr);                      // 1
    ok = ok && add_c2f(y, Slice{b1, 0, c2}, Slice{b2, 0, c2}, m.rep[0], true);                     // 2
    CV(Slice{b2, 0, c2}, Slice{b3, 0, c3}, 3, 2, true, nullptr, 0, nullptr);                      // 3
    ok = ok && add_c2f(y, Slice{b3, 0, c3}, Slice{cat14, c4, c3}, m.rep[1], true);                 // 4 -> cat14[c4:]
    CV(Slice{cat14, c4, c3}, Slice{b5, 0, c4}, 3, 2, true, nullptr, 0, nullptr);                  // 5
    ok = ok && add_c2f(y, Slice{b5, 0, c4}, Slice{cat11, c5, c4}, m.rep[2], true);                 // 6 -> cat11[c5:]
    CV(Slice{cat11, c5, c4}, Slice{b7, 0, c5}, 3, 2, true, nullptr, 0, nullptr);                  // 7
    ok = ok && add_c2f(y, Slice{b7, 0, c5}, Slice{b8, 0, c5}, m.rep[3], true);                     // 8
    CV(Slice{b8, 0, c5}, Slice{spp, 0, cs}, 1, 1, true, nullptr, 0, nullptr);                     // 9 SPPF cv1
    if (y.f32) {
        for (int i = 0; i < 3; ++i) add_simple(y, OP_MAXPOOL, Slice{spp, cs * i, cs}, Slice{spp, cs * (i + 1), cs}, H / 32, W / 32, cs);
    } else {                                               // all three pools from one LDS copy of the map (at most 20 x 20 pixels: letterbox())
        ok = ok && (H / 32) * (W / 32) <= 1024;
        add_simple(y, OP_POOLS, Slice{spp, 0, cs}, Slice{spp, cs, 3 * cs}, H / 32, W / 32, cs);
    }
    CV(Slice{spp, 0, 4 * cs}, Slice{cat20, c4, c5}, 1, 1, true, nullptr, 0, nullptr);             // 9 SPPF cv2 -> cat20[c4:]
    add_simple(y, OP_UPSAMPLE, Slice{cat20, c4, c5}, Slice{cat11, 0, c5}, H / 32, W / 32, c5);     // 10 upsample -> cat11[:c5]
    y.ops.back().vcat = (int)y.ops.size();                                                          // (its only reader: layer 12's cv1, the next op)
    ok = ok && add_c2f(y, Slice{cat11, 0, c5 + c4}, Slice{cat17, c3, c4}, nr, false);              // 12 -> cat17[c3:]
    add_simple(y, OP_UPSAMPLE, Slice{cat17, c3, c4}, Slice{cat14, 0, c4}, H / 16, W / 16, c4);     // 13 upsample -> cat14[:c4]
    y.ops.back().vcat = (int)y.ops.size();                                                          // (layer 15's cv1)
    ok = ok && add_c2f(y, Slice{cat14, 0, c4 + c3}, Slice{p3, 0, c3}, nr, false);                  // 15
    CV(Slice{p3, 0, c3}, Slice{cat17, 0, c3}, 3, 2, true, nullptr, 0, nullptr);                   // 16 -> cat17[:c3]
    ok = ok && add_c2f(y, Slice{cat17, 0, c3 + c4}, Slice{p4, 0, c4}, nr, false);                  // 18
    CV(Slice{p4, 0, c4}, Slice{cat20, 0, c4}, 3, 2, true, nullptr, 0, nullptr);                   // 19 -> cat20[:c4]
    ok = ok && add_c2f(y, Slice{cat20, 0, c4 + c5}, Slice{p5, 0, c5}, nr, false);                  // 21
    const int pl[3] = {p3, p4, p5}, pc[3] = {c3, c4, c5}, dv[3] = {8, 16, 32};
    y.A = 0;
    for (int i = 0; i < 3 && ok; ++i) {                                                            // 22 Detect
        const int hh = H / dv[i], ww = W / dv[i];
        y.lvH[i] = hh, y.lvW[i] = ww;
        // the class branch at its padded widths: zero filters and biases behind the real ones (Slice::real), so a padded hidden
        // channel is silu(0) = 0 and a padded logit 0.0f
        const int ba = nb(hh, ww, hb), bb = nb(hh, ww, hb), ca = nb(hh, ww, hcp), cb = nb(hh, ww, hcp);
        ok = ok && dev_alloc(y, (void**)&y.head_box[i], (size_t)batch * hh * ww * 4 * REG_MAX * 4);
        ok = ok && dev_alloc(y, (void**)&y.head_cls[i], (size_t)batch * hh * ww * ncp * 4);
        if (!ok) break;
        if (i == 0) y.head_begin = (int)y.ops.size();
        CV(Slice{pl[i], 0, pc[i]}, Slice{ba, 0, hb}, 3, 1, true, nullptr, 0, nullptr);
        CV(Slice{ba, 0, hb}, Slice{bb, 0, hb}, 3, 1, true, nullptr, 0, nullptr);
        CV(Slice{bb, 0, hb}, Slice{-1, 0, 4 * REG_MAX}, 1, 1, false, y.head_box[i], 4 * REG_MAX, nullptr);
        if (ok) y.ops.back().dec = 1, y.ops.back().dec_level = i;
        const size_t cls_first = y.ops.size();
        CV(Slice{pl[i], 0, pc[i]}, Slice{ca, 0, hcp, hc}, 3, 1, true, nullptr, 0, nullptr);
        CV(Slice{ca, 0, hcp, hc}, Slice{cb, 0, hcp, hc}, 3, 1, true, nullptr, 0, nullptr);
        CV(Slice{cb, 0, hcp, hc}, Slice{-1, 0, ncp, nc}, 1, 1, false, y.head_cls[i], ncp, nullptr);
        if (ok) y.ops.back().dec = 2, y.ops.back().dec_level = i;
        for (size_t q = cls_first; q < y.ops.size(); ++q) y.ops[q].lane = 1;       // own buffers, independent of the box branch
        y.A += hh * ww;
    }
#undef CV
    ok = ok && y.wpos == y.wtotal && y.A <= MAX_CAND;
    y.words = (y.A + 63) / 64;
    ok = ok && dev_alloc(y, (void**)&y.cbox, (size_t)batch * y.A * 16) && dev_alloc(y, (void**)&y.cconf, (size_t)batch * y.A * 4) &&
         dev_alloc(y, (void**)&y.ccls, (size_t)batch * y.A * 4) && dev_alloc(y, (void**)&y.sbox, (size_t)batch * y.A * 16) &&
         dev_alloc(y, (void**)&y.sidx, (size_t)batch * y.A * 4) && dev_alloc(y, (void**)&y.scount, (size_t)batch * 4);
    y.named = {{0, Slice{x0, 0, 3}}, {1, Slice{b1, 0, c2}}, {2, Slice{b2, 0, c2}}, {4, Slice{cat14, c4, c3}},
               {6, Slice{cat11, c5, c4}}, {8, Slice{b8, 0, c5}}, {9, Slice{cat20, c4, c5}}, {12, Slice{cat17, c3, c4}},
               {15, Slice{p3, 0, c3}}, {18, Slice{p4, 0, c4}}, {21, Slice{p5, 0, c5}}, {7, Slice{b7, 0, c5}}, {19, Slice{cat20, 0, c4}}};
    if (y.dbg_cat >= 0) y.named.push_back({40, Slice{y.dbg_cat, 0, y.bufs[y.dbg_cat].C}});
    y.wsrc = nullptr;
    AV_REQUIRE(ok, AV_EINVAL, "av_yolo_create: graph construction failed (parameter blob / capacity mismatch)");
    return AV_OK;
}

// ---- host side: the plan of a forward ----------------------------------------------------------------------------

// `s` becomes a launch of variant <p...> of family `fam`; a variant that kVariants does not list, or more LDS than its limit, is an error
int use_variant(Step& s, Family fam, const int (&p)[6], dim3 grid, dim3 block, size_t lds) {
    const Variant* v = find_variant(fam, p);
    AV_REQUIRE(v, AV_EINVAL, "av_yolo: no kernel of family %d for <%d,%d,%d,%d,%d,%d>", (int)fam, p[0], p[1], p[2], p[3], p[4], p[5]);
    AV_REQUIRE(lds <= (size_t)std::max(v->lds_limit, 64 * 1024), AV_EINVAL, "av_yolo: %zu bytes of LDS for a kernel limited to %d", lds, v->lds_limit);
    s.fn = v->fn, s.grid = grid, s.block = block, s.lds = lds;
    s.fam = fam, std::copy(p, p + 6, s.var);
    return AV_OK;
}

// The launch of one stand-alone convolution of the half-precision chain: the only place that decides between conv_gemm128_kernel,
// conv1x1_ws_kernel, conv3x3_ws_kernel, conv_lds_kernel and conv_mfma_kernel.  a.in2 set (virtual Upsample + Concat: a 1x1 layer with
// mt = 4 and whole 32-channel chunks whose input is split into `in` / `in2`): only conv_gemm128_kernel and conv_lds_kernel<4,1> read that.
int choose_conv(const ConvArgs& a, int mt, int dec, const DecArgs& dec_args, int B, Hooks hk, Step& s) {
    AV_REQUIRE(a.cout % (16 * mt) == 0, AV_EINVAL, "av_yolo: convolution with %d output channels in tiles of %d", a.cout, 16 * mt);
    const int gy = a.cout / (16 * mt), n32 = (a.npix + 31) / 32;
    const bool one = a.ksz == 1 && a.stride == 1, split = a.in2 != nullptr;
    auto gemm128 = [&] { s.args(a); return use_variant(s, K_GEMM128, {}, dim3((a.npix + 63) / 64, a.cout / 128), dim3(256), (size_t)2 * (128 + 64) * CG_ROWB); };
    auto lds_tiled = [&] {
        const int tiles_x = (a.Wo + LT_W - 1) / LT_W, tiles_y = (a.Ho + LT_H - 1) / LT_H, taps = a.ksz * a.ksz;
        const int PH = (LT_H - 1) * a.stride + a.ksz, PW = (LT_W - 1) * a.stride + a.ksz;
        s.args(a, tiles_x, tiles_y);
        return use_variant(s, K_LDS, {mt, a.ksz, a.stride == 1 ? 0 : a.stride}, dim3(tiles_x * tiles_y * B, gy), dim3(256),
                           (((size_t)PH * PW * lt_pixb(a.stride) + 15) & ~size_t(15)) + (size_t)16 * mt * (taps * LT_CK * 2 + 32));
    };
    // 1x1 with cin a multiple of 64 and cout of 128 (the cv1 / cv2 of the P4 and P5 blocks, SPPF; layer 12's cv1 with both its sources): a
    // GEMM over flattened pixels.  Measured against conv1x1_ws_kernel / conv_lds_kernel on all eleven such layers at 64 frames: 7.0-15.6
    // against 8.0-20.3 us, every one faster, 22 us per forward together.
    const bool gemm1x1 = one && a.cin % CG_SC == 0 && a.cout % 128 == 0 && !a.res && !dec && a.kreal == a.cin && (!split || a.k1 % CG_SC == 0) &&
                         !hk.no_gemm && !hk.no_gemm_1x1;
    if (split) return gemm1x1 ? gemm128() : lds_tiled();
    // the head's last convolutions, with the decode in their epilogue: box 64 -> 64 (two whole steps), class 80 -> 80 (two whole steps + a
    // 16-channel tail); float32 logits only on request
    if (dec == 1 && a.cin == 64 && a.cout == 64 && mt == 4) {
        s.args(a, n32, dec_args);
        return use_variant(s, K_WS1, {4, 2, false, 1}, dim3((unsigned)std::max(1, std::min((n32 + 1) / 2, 2048))), dim3(128),
                           (((size_t)64 * ws_stride(128) + 15) & ~size_t(15)) + (size_t)2 * 16 * DEC_ROW * sizeof(float));
    }
    const bool generic80 = a.cin == 80 && hk.generic80;
    if (one && a.cin == 80 && a.cout == 80 && mt == 5 && !a.res && !generic80) {      // (dec: 2 or 0 here -- 3 needs whole 32-channel steps)
        s.args(a, n32, dec_args);
        return use_variant(s, K_WS1, {5, 2, true, dec == 2 ? 2 : 0}, dim3((unsigned)std::max(1, std::min((n32 + 3) / 4, 1024))), dim3(256),
                           (size_t)80 * ws_stride(160));
    }
    // the class branch's last convolution of any other model, nc at run time: all 16 mt >= nc output channels in one workgroup
    if (dec == 3) {
        s.args(a, n32, dec_args);
        return use_variant(s, K_WS1, {mt, a.cin / 32, false, 3}, dim3((unsigned)std::max(1, std::min((n32 + 3) / 4, 1024))), dim3(256),
                           (size_t)16 * mt * ws_stride(a.cin * 2));
    }
    if (gemm1x1) return gemm128();
    // 1x1 with whole 32-channel steps: weights resident in LDS, pixel fragments straight from global memory
    if (one && a.cin % 32 == 0 && !a.res && (mt == 2 || mt == 4)) {
        const int ks = a.cin / 32;
        const int want[6] = {mt, ks, 0, 0, 0, 0};
        const bool ks_ok = find_variant(K_WS1, want) != nullptr;       // (listed: mt 2 with ks 1; mt 4 with ks 2, 3, 4, 6, 8, 12, 16)
        // measured per layer at 64 frames (profiles/README.md): wins on the small maps (P5 any cin, P4 up to 192 channels) and for
        // cin <= 64 anywhere; the big maps with long K stay with conv_lds_kernel, which is within 20 % of their HBM floor
        const bool pays = a.npix <= 20000 || (a.npix <= 70000 && ks <= 6) || ks <= 2;
        if (ks_ok && pays) {
            const size_t lds = (size_t)16 * mt * ws_stride(a.cin * 2);
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / lds));
            s.args(a, n32, dec_args);
            return use_variant(s, K_WS1, {mt, ks, false, 0}, dim3((unsigned)std::max(1, std::min((n32 + 3) / 4, 256 * per_cu / gy)), gy), dim3(256), lds);
        }
    }
    // weight-stationary persistent kernel for the stride-2 layers whose weights fit (cin <= 64): 8 x 16 output tiles, 17 x 33 patches
    if (a.stride == 2 && a.ksz == 3 && a.cin % 8 == 0 && !a.res) {
        const int cp = (a.cin + 31) & ~31;
        if ((cp == 32 && (mt == 2 || mt == 4)) || (cp == 64 && (mt == 4 || mt == 3))) {
            const size_t lds = (((size_t)16 * mt * ws_stride(9 * cp * 2) + 15) & ~size_t(15)) + (size_t)17 * 33 * (cp * 2 + 16);
            const int tiles_x = (a.Wo + LT_W - 1) / LT_W, tiles_y = (a.Ho + 7) / 8, n_tiles = tiles_x * tiles_y * B;
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / lds));
            s.args(a, tiles_x, tiles_y, n_tiles);
            return use_variant(s, K_WS3, {mt, 1, 8, cp, false, 2}, dim3((unsigned)std::max(1, std::min(n_tiles, 256 * per_cu / gy)), gy), dim3(512), lds);
        }
    }
    // the same for 3x3 stride 1: the whole weight matrix + one all-channel patch in LDS
    const int cinp = a.cin == 80 ? 80 : (a.cin + 31) & ~31;       // channels per pixel in the LDS image
    const bool ws_shape = a.stride == 1 && a.ksz == 3 && a.cin % 8 == 0 && a.cout == 16 * mt &&
                          ((cinp == 32 && mt <= 2) || (cinp == 64 && (mt == 4 || mt == 5 || mt == 3)) || (cinp == 80 && mt == 5));
    if (ws_shape && !generic80) {
        const long tiles16 = (long)((a.Wo + LT_W - 1) / LT_W) * ((a.Ho + 15) / 16) * B;
        auto lds_of = [&](int tr) {
            return (((size_t)16 * mt * ws_stride(9 * cinp * 2) + 15) & ~size_t(15)) + (size_t)(tr + 2) * (LT_W + 2) * ws_stride(cinp * 2);
        };
        const int TR = tiles16 >= 512 && lds_of(16) <= 156 * 1024 ? 16 : 8;          // tile rows
        const size_t lds = lds_of(TR);
        if (lds <= 156 * 1024) {
            const int tiles_x = (a.Wo + LT_W - 1) / LT_W, tiles_y = (a.Ho + TR - 1) / TR, n_tiles = tiles_x * tiles_y * B;
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / lds));
            s.args(a, tiles_x, tiles_y, n_tiles);
            return use_variant(s, K_WS3, {mt, TR / 8, 8, cinp, a.res != nullptr, 1}, dim3((unsigned)std::min(n_tiles, 256 * per_cu)), dim3(512), lds);
        }
    }
    // measured per layer (profiles/r01_yolo_b64_*): the LDS kernel wins for stride-1 3x3 (any cin >= 16, the tail of
    // a partial 32-channel chunk is zero-filled) and for 1x1 with whole chunks
    // (1x1 with a partial last chunk: the kernel zero-fills it like the 3x3 form's; taken for the widths a padded class branch brings,
    // 112 and up -- cin = 48 and 80, scale n's, stay on the kernels they are pinned to bit for bit)
    const bool whole_or_wide = a.cin % LT_CK == 0 || (a.cin % 16 == 0 && a.cin > 96 && !split);
    if (a.stride == 1 && ((a.ksz == 3 && a.cin >= 16 && a.cin % 8 == 0) || (a.ksz == 1 && whole_or_wide))) return lds_tiled();
    // the long-K stride-2 layers (scale n: the two with cin = 128; s: 256 -> 512 / 256; m: 192 -> 384, 384 -> 384): the GEMM form where its
    // tile fits (cin in whole 64-channel steps, cout in 128-channel tiles) ...
    const bool gemm_s2 = a.ksz == 3 && a.stride == 2 && a.cin % CG_SC == 0 && a.cout % 128 == 0 && !a.res && a.kreal == 9 * a.cin;
    if (gemm_s2 && !hk.no_gemm) return gemm128();
    // ... and conv_lds_kernel's stride-2 form for the other 64-channel-tiled ones (m: 96 -> 192, 384 -> 576, 192 -> 192)
    if (a.ksz == 3 && a.stride == 2 && a.cin % 8 == 0 && mt == 4 && !a.res && !gemm_s2) return lds_tiled();
    s.args(a);
    return use_variant(s, K_MFMA, {mt, 2}, dim3((a.npix + 16 * 2 * 4 - 1) / (16 * 2 * 4), gy), dim3(256), 0);
}

// the same for the float32 chain: the LDS-tiled GEMM form for every layer but the stem (cin = 4)
int choose_conv_f32(const ConvArgsF& a, Step& s) {
    s.args(a);
    if (a.cin % 16 == 0) {
        // channel tile: the widest of 128, 80, 64, 48, 32, 16 that divides cout (48: scale m's 48 / 96 / 288; 16: a padded class count)
        int AR = 16;
        for (int t : {32, 48, 64, 80, 128})
            if (a.cout % t == 0) AR = t;
        const int BR = AR == 128 ? 64 : 128, KC = a.cin % 32 == 0 ? 32 : 16;
        return use_variant(s, K_GEMM_F32, {AR, BR, KC}, dim3((a.npix + BR - 1) / BR, a.cout / AR), dim3(256), (size_t)2 * (AR + BR) * (KC * 4 + 32));
    }
    AV_REQUIRE(a.cin == 4 && a.cout % 16 == 0, AV_EINVAL, "av_yolo: no float32 kernel for a convolution %d -> %d", a.cin, a.cout);
    // the stem (K = 27), in 16-channel tiles at every scale; pixels per wave (16 NT): small maps need small tiles to fill the chip
    const int nt = a.npix >= 200000 ? 4 : (a.npix >= 50000 ? 2 : 1);
    return use_variant(s, K_STEM_F32, {1, nt, 4, 2}, dim3((a.npix + 64 * nt - 1) / (64 * nt), a.cout / 16), dim3(256), 0);
}

// the 1x1 convolution cv can fetch its first channels from upsample op's half-resolution source itself
bool reads_upsample(const Yolo& y, const Yolo::Op& op, const Yolo::Op& cv) {
    const ConvArgs& c = cv.ca;
    const Buf& bo = y.bufs[op.out.buf];
    return cv.kind == OP_CONV && c.ksz == 1 && c.stride == 1 && c.cin % LT_CK == 0 && op.C % LT_CK == 0 && c.in == bo.p && c.in_coff == op.out.coff &&
           c.in_cs == bo.C && c.H == 2 * op.H && c.W == 2 * op.W && cv.mt == 4 && c.cout % 64 == 0 && c.cin > op.C && !c.res;
}

// a 32-channel C2f block of np bottleneck pairs as the c2f32 kernels expect it: cv1 = c1, first 3x3 layer b1, cv2 = c2 reading the whole concat buffer
bool c2f32_shapes(const ConvArgs& c1, const ConvArgs& b1, const ConvArgs& c2, int np) {
    return c2.kpad == 32 * (np + 2) && b1.kpad == 288 && c2.in == c1.out && c2.in_coff == c1.out_coff && c2.in_cs == c1.out_cs;
}

// C2f32Args of a 32-channel block whose cv1 is c1, for the bottleneck pair b1 / b2 that reads concat channels [32 np, 32 np + 32)
C2f32Args c2f32_args(const ConvArgs& c1, const ConvArgs& b1, const ConvArgs& b2, int np, int B) {
    C2f32Args fa{};
    fa.H = c1.H, fa.W = c1.W, fa.tiles_x = (c1.W + 15) / 16, fa.tiles_y = (c1.H + 15) / 16, fa.n_tiles = fa.tiles_x * fa.tiles_y * B;
    fa.cat = c1.out, fa.cat_cs = c1.out_cs, fa.cat_coff = c1.out_coff;
    fa.in = c1.out, fa.in_cs = c1.out_cs, fa.in_coff = c1.out_coff + 32 * np;
    fa.w_b1 = b1.wgt, fa.w_b2 = b2.wgt, fa.bs_b1 = b1.bias, fa.bs_b2 = b2.bias, fa.kb = b1.kpad;
    return fa;
}

// Every launch of a forward from the frame to the head's candidates (float32: to its logits), in order.  Which kernel runs a layer
// depends on the layer shapes and the batch (fixed at create), the hooks and keep_logits -- and on the frame pointer's alignment,
// for which the plan holds both forms of the front (Step::when).
// decode_alone: the head has no decode epilogue for this model's shapes -- its last convolutions write float32 logits and the stand-alone
// decode_kernel makes the candidates (always so in the float32 chain).  Epilogues exist for a 64 -> 64 box convolution together with a class
// convolution of 80 -> 80 with nc = 80 (compile-time count) or hc -> 16 mt >= nc with a conv1x1_ws_kernel<mt, hc / 32, false, 3> in kVariants.
int plan_forward(const Yolo& y, Hooks hk, bool keep_logits, std::vector<Step>& plan, bool& decode_alone) {
    const int B = y.B, n = B * y.H * y.W;
    plan.clear();
    decode_alone = true;
    auto add = [&](When when = ALWAYS) -> Step& {
        plan.emplace_back();
        plan.back().when = when;
        return plan.back();
    };
    auto preprocess = [&](auto kernel, int threads, When when, auto* out) {       // (the walker puts the frame pointer in)
        Step& s = add(when);
        s.kernel(kernel, dim3((threads + 255) / 256), dim3(256), 0, nullptr, B, y.inH, y.inW, y.H, y.W, y.nh, y.nw, y.top, y.left, out);
        s.takes_bgr = true;
    };
    if (y.f32) {
        // reference-precision chain: one lane, one launch per layer, float32 logits, stand-alone decode
        preprocess(preprocess_f32_kernel, n, ALWAYS, reinterpret_cast<float*>(y.bufs[0].p));
        for (const Yolo::Op& op : y.ops) {
            const int k = (int)(&op - y.ops.data());
            if (op.kind == OP_CONV_F32) {
                const int rc = choose_conv_f32(op.cf, add());
                if (rc != AV_OK) return rc;
                plan.back().first_op = k, plan.back().n_ops = 1;
                continue;
            }
            AV_REQUIRE(op.kind == OP_MAXPOOL || op.kind == OP_UPSAMPLE, AV_EINVAL, "av_yolo: op kind %d has no float32 form", (int)op.kind);
            const Buf &bi = y.bufs[op.in.buf], &bo = y.bufs[op.out.buf];
            const int threads = op.kind == OP_MAXPOOL ? B * op.H * op.W * op.C : B * 4 * op.H * op.W * (op.C / 4);
            add().kernel(op.kind == OP_MAXPOOL ? maxpool5_f32_kernel : upsample2_f32_kernel, dim3((threads + 255) / 256), dim3(256), 0,
                         reinterpret_cast<const float*>(bi.p), bi.C, op.in.coff, reinterpret_cast<float*>(bo.p), bo.C, op.out.coff, B, op.H, op.W, op.C);
            plan.back().first_op = k, plan.back().n_ops = 1;
        }
        return AV_OK;
    }
    // which decode epilogue the head's last convolutions have (the three levels share their shapes)
    auto cls_epilogue = [&](const Yolo::Op& o) {
        const ConvArgs& a = o.ca;
        if (a.cin == 80 && a.cout == 80 && o.mt == 5 && y.model.nc == NC) return 2;
        const int p[6] = {o.mt, a.cin / 32, 0, 3, 0, 0};
        return a.cin % 32 == 0 && a.cout == 16 * o.mt && find_variant(K_WS1, p) ? 3 : 0;
    };
    int epilogue = 0;
    for (const Yolo::Op& o : y.ops) {
        if (o.dec == 1 && !(o.ca.cin == 64 && o.ca.cout == 64 && o.mt == 4)) break;
        if (o.dec == 2) { epilogue = cls_epilogue(o); break; }
    }
    decode_alone = epilogue == 0;
    // the 2:1 letterbox kernels read dwords: they need a 4-byte aligned frame pointer
    const bool twice = y.inH == 2 * y.nh && y.inW == 2 * y.nw && y.inW % 4 == 0 && y.left % 2 == 0 && y.nw % 2 == 0 && y.W % 2 == 0 && !hk.generic_pre;
    // letterbox + stem + layer 1 in one launch (front_fused_kernel); with keep_logits (test hook) the three launches run, so that
    // the network input and the stem's map exist for inspection
    const bool front = twice && y.left == 0 && y.nw == y.W && y.H % 4 == 0 && y.W % 4 == 0 && y.ops.size() > 2 && y.ops[0].kind == OP_STEM &&
                       y.ops[1].kind == OP_CONV && y.ops[1].ca.cin == 16 && y.ops[1].ca.cout == 32 && y.ops[1].ca.stride == 2 && !keep_logits && !hk.no_fuse;
    if (front) {
        const ConvArgs &c0 = y.ops[0].ca, &c1 = y.ops[1].ca;
        FrontArgs fa;
        fa.bgr = nullptr, fa.fh = y.inH, fa.fw = y.inW, fa.H = y.H, fa.W = y.W, fa.top = y.top, fa.nh = y.nh;
        fa.w_stem = c0.wgt, fa.bs_stem = c0.bias, fa.w_l1 = c1.wgt, fa.bs_l1 = c1.bias, fa.kpad1 = c1.kpad;
        fa.out = c1.out, fa.out_cs = c1.out_cs, fa.out_coff = c1.out_coff, fa.Ho = c1.Ho, fa.Wo = c1.Wo;
        fa.tiles_x = (c1.Wo + 15) / 16, fa.tiles_y = (c1.Ho + 7) / 8, fa.n_tiles = fa.tiles_x * fa.tiles_y * B;
        static_assert(offsetof(FrontArgs, bgr) == 0, "Step::takes_bgr");
        Step& s = add(BGR_ALIGNED);
        s.kernel(front_fused_kernel, dim3((unsigned)std::min(fa.n_tiles, 512)), dim3(FR_NTH), FR_LDS, fa);
        s.takes_bgr = true, s.first_op = 0, s.n_ops = 2;
    } else if (twice) {
        preprocess(preprocess2_kernel, n / 2, BGR_ALIGNED, y.bufs[0].p);
    }
    preprocess(preprocess_kernel, n, twice ? BGR_UNALIGNED : ALWAYS, y.bufs[0].p);
    // (Walking the chain with 2 or 4 sub-batches of the frames on as many streams was measured, to let one group's per-launch
    // latency hide behind another's work: 1.78 -> 1.80 / 1.99 ms at 64 frames -- every launch already occupies the whole chip,
    // so the groups only queue behind each other; dropped)
    for (size_t oi = 0; oi < y.ops.size(); ++oi) {
        const Yolo::Op& op = y.ops[oi];
        const size_t at = oi, first = plan.size();
        auto conv = [&](const Yolo::Op& o, const ConvArgs& a) {
            DecArgs dec{};
            const int epi = !o.dec || !epilogue ? 0 : (o.dec == 1 ? 1 : epilogue);
            if (epi) {
                int aoff = 0;
                for (int i = 0; i < o.dec_level; ++i) aoff += y.lvH[i] * y.lvW[i];
                dec = DecArgs{y.cbox, y.cconf, y.ccls, y.A, aoff, 8 << o.dec_level, keep_logits ? 1 : 0, y.model.nc};
            }
            const int rc = choose_conv(a, o.mt, epi, dec, B, hk, add());
            plan.back().first_op = (int)(&o - y.ops.data()), plan.back().n_ops = 1;
            return rc;
        };
        auto c2f32 = [&](auto kernel, size_t lds, const C2f32Args& fa) {
            add().kernel(kernel, dim3((unsigned)std::min(fa.n_tiles, 256)), dim3(F32_NTH), lds, fa);
            plan.back().n_ops = 3;                         // a bottleneck pair + the 1x1 convolution on one of its sides
        };
        int rc = AV_OK;
        if (op.fuse == 1 && !hk.no_fuse) {                 // cv1, 3x3, 3x3 + shortcut, cv2 in one launch
            const ConvArgs &c1 = op.ca, &b1 = y.ops[oi + 1].ca, &b2 = y.ops[oi + 2].ca, &c2 = y.ops[oi + 3].ca;
            C2f16Args fa;
            fa.in = c1.in, fa.in_cs = c1.in_cs, fa.in_coff = c1.in_coff;
            fa.out = c2.out, fa.out_cs = c2.out_cs, fa.out_coff = c2.out_coff;
            fa.H = c1.H, fa.W = c1.W, fa.tiles_x = (c1.W + 15) / 16, fa.tiles_y = (c1.H + 15) / 16;
            fa.n_tiles = fa.tiles_x * fa.tiles_y * B;
            fa.w_cv1 = c1.wgt, fa.w_b1 = b1.wgt, fa.w_b2 = b2.wgt, fa.w_cv2 = c2.wgt;
            fa.bs_cv1 = c1.bias, fa.bs_b1 = b1.bias, fa.bs_b2 = b2.bias, fa.bs_cv2 = c2.bias;
            fa.kb = b1.kpad, fa.kc = c2.kpad;
            add().kernel(c2f16_fused_kernel, dim3((unsigned)std::min(fa.n_tiles, 512)), dim3(C2F_NTH), C2F_LDS, fa);
            plan.back().first_op = (int)at, plan.back().n_ops = 4;
            oi += 3;
        } else if (op.kind == OP_UPSAMPLE && op.vcat == (int)oi + 1 && !hk.no_fuse && reads_upsample(y, op, y.ops[oi + 1])) {
            // virtual Upsample + Concat: the upsample launch is skipped and its only reader, a 1x1 convolution, fetches the first k1 input
            // channels from the half-resolution source itself (same values: bit-identical output)
            const Yolo::Op& cv = y.ops[oi + 1];
            const ConvArgs& c1 = cv.ca;
            const Buf& bi = y.bufs[op.in.buf];
            ConvArgs v = c1;
            v.in = bi.p, v.in_cs = bi.C, v.in_coff = op.in.coff;                            // channels [0, k1): the upsample's source, half resolution
            v.in2 = c1.in, v.in2_cs = c1.in_cs, v.in2_coff = c1.in_coff + op.C, v.k1 = op.C;   // channels [k1, cin): the concat buffer's own part
            rc = conv(cv, v);
            plan.back().first_op = (int)at, plan.back().n_ops = 2;       // the upsample and its reader
            oi += 1;
            const ConvArgs* c2 = cv.fuse == 3 ? &y.ops[oi + 3].ca : nullptr;
            if (rc == AV_OK && c2 && c2f32_shapes(c1, y.ops[oi + 1].ca, *c2, 1)) {
                // layer 15's block continues with its bottleneck pair + cv2 in one launch (otherwise: with the unfused bottlenecks)
                C2f32Args fa = c2f32_args(c1, y.ops[oi + 1].ca, y.ops[oi + 2].ca, 1, B);
                fa.w_cv2 = c2->wgt, fa.bs_cv2 = c2->bias, fa.kc = c2->kpad;
                fa.out = c2->out, fa.out_cs = c2->out_cs, fa.out_coff = c2->out_coff;
                c2f32(c2f32_tail_kernel<64, false>, f32t_lds(64), fa);
                plan.back().first_op = (int)oi + 1;
                oi += 3;
            }
        } else if (op.fuse == 2 && !hk.no_fuse && op.ca.kpad == 64 && c2f32_shapes(op.ca, y.ops[oi + 1].ca, y.ops[oi + 5].ca, 2)) {
            // layer 4: cv1 + the first bottleneck pair, then the second pair + cv2
            const ConvArgs &c1 = op.ca, &c2 = y.ops[oi + 5].ca;
            C2f32Args fh = c2f32_args(c1, y.ops[oi + 1].ca, y.ops[oi + 2].ca, 1, B);
            fh.in = c1.in, fh.in_cs = c1.in_cs, fh.in_coff = c1.in_coff;
            fh.w_cv1 = c1.wgt, fh.bs_cv1 = c1.bias, fh.k1 = c1.kpad;
            c2f32(c2f32_head_kernel, F32H_LDS, fh);
            plan.back().first_op = (int)at;
            C2f32Args ft = c2f32_args(c1, y.ops[oi + 3].ca, y.ops[oi + 4].ca, 2, B);
            ft.w_cv2 = c2.wgt, ft.bs_cv2 = c2.bias, ft.kc = c2.kpad;
            ft.out = c2.out, ft.out_cs = c2.out_cs, ft.out_coff = c2.out_coff;
            c2f32(c2f32_tail_kernel<96, true>, f32t_lds(96), ft);
            plan.back().first_op = (int)at + 3;
            oi += 5;
        } else if (op.kind == OP_CONV) {
            rc = conv(op, op.ca);
        } else if (op.kind == OP_STEM) {
            if (op.ca.cout == 16) add().kernel(stem_conv_kernel<false>, dim3((op.ca.npix + 255) / 256), dim3(256), 0, op.ca, op.ca.npix);
            else add().kernel(stem_conv_kernel<true>, dim3((op.ca.npix + 255) / 256, op.ca.cout / 16), dim3(256), 0, op.ca, op.ca.npix);
            plan.back().first_op = (int)at, plan.back().n_ops = 1;
        } else {
            AV_REQUIRE(op.kind == OP_POOLS || op.kind == OP_UPSAMPLE, AV_EINVAL, "av_yolo: op kind %d has no half-precision form", (int)op.kind);
            const Buf &bi = y.bufs[op.in.buf], &bo = y.bufs[op.out.buf];
            const int hw = op.H * op.W;
            if (op.kind == OP_POOLS)
                add().kernel(sppf_pools_kernel, dim3(B, op.C / 8), dim3((hw + 63) / 64 * 64), (size_t)hw * 64, bi.p, bi.C, op.in.coff, bo.p, bo.C,
                             op.out.coff, op.H, op.W, op.C);
            else
                add().kernel(upsample2_kernel, dim3((B * 4 * hw * (op.C / 8) + 255) / 256), dim3(256), 0, bi.p, bi.C, op.in.coff, bo.p, bo.C,
                             op.out.coff, B, op.H, op.W, op.C);
            plan.back().first_op = (int)at, plan.back().n_ops = 1;
        }
        if (rc != AV_OK) return rc;
        for (size_t q = first; q < plan.size(); ++q) {
            plan[q].lane = op.lane;
            if (front && at < 2) plan[q].when = BGR_UNALIGNED;       // the stem and layer 1, where front_fused_kernel cannot run
        }
        if ((int)at == y.head_begin) plan[first].head = true;
    }
    return AV_OK;
}

}  // namespace

struct av_yolo { Yolo y; };

extern "C" {

int av_yolo_ctx_free(av_ctx*) { return AV_OK; }

int av_yolo_model_preset(int scale_char, int nc, av_yolo_model* model) {
    AV_REQUIRE(model, AV_EINVAL, "av_yolo_model_preset: null argument");
    // yolov8.yaml: depth, width, max_channels per scale; channels = make_divisible(min(c, max_channels) width, 8), repeats = max(round(n depth), 1)
    double depth, width;
    int max_ch;
    switch (scale_char) {
    case 'n': depth = 0.33, width = 0.25, max_ch = 1024; break;
    case 's': depth = 0.33, width = 0.50, max_ch = 1024; break;
    case 'm': depth = 0.67, width = 0.75, max_ch = 768; break;
    case 'l':
    case 'x':
        av_set_error("av_yolo_model_preset: scale '%c' is not built (n, s and m are)", scale_char);
        return AV_EINVAL;
    default:
        av_set_error("av_yolo_model_preset: unknown scale character %d (n, s and m are built)", scale_char);
        return AV_EINVAL;
    }
    AV_REQUIRE(nc >= 1 && nc <= 256, AV_EINVAL, "av_yolo_model_preset: nc = %d, 1 .. 256 are built", nc);
    av_yolo_model m{};
    const int base[5] = {64, 128, 256, 512, 1024}, reps[4] = {3, 6, 6, 3};
    for (int i = 0; i < 5; ++i) m.ch[i] = (int)std::ceil(std::min(base[i], max_ch) * width / 8.0) * 8;
    for (int i = 0; i < 4; ++i) m.rep[i] = std::max((int)std::nearbyint(reps[i] * depth), 1);
    m.neck_rep = std::max((int)std::nearbyint(3 * depth), 1);
    m.nc = nc;
    *model = m;
    return AV_OK;
}

namespace {
// a model this library builds and tests: what av_yolo_model_preset gives for scale n, s or m with the model's nc, reserved words zero
// (the struct is how the graph builder is told the model, not an invitation to other widths: their kernels are not listed)
bool model_ok(const av_yolo_model& m) {
    if (m.nc < 1 || m.nc > 256) return false;
    for (char scale : {'n', 's', 'm'}) {
        av_yolo_model p;
        if (av_yolo_model_preset(scale, m.nc, &p) == AV_OK && memcmp(&p, &m, sizeof p) == 0) return true;
    }
    return false;
}
}  // namespace

size_t av_yolo_model_param_count(const av_yolo_model* model) {
    if (!model || !model_ok(*model)) return 0;
    const av_yolo_model& m = *model;
    size_t n = 0;
    auto conv = [&](int cin, int cout, int k, bool bn) { n += (size_t)cout * cin * k * k + (bn ? 4 : 1) * (size_t)cout; };
    auto c2f = [&](int cin, int cout, int r) {
        const int c = cout / 2;
        conv(cin, 2 * c, 1, true);
        for (int i = 0; i < 2 * r; ++i) conv(c, c, 3, true);
        conv((2 + r) * c, cout, 1, true);
    };
    const int c1 = m.ch[0], c2 = m.ch[1], c3 = m.ch[2], c4 = m.ch[3], c5 = m.ch[4];
    conv(3, c1, 3, true), conv(c1, c2, 3, true), c2f(c2, c2, m.rep[0]), conv(c2, c3, 3, true), c2f(c3, c3, m.rep[1]);
    conv(c3, c4, 3, true), c2f(c4, c4, m.rep[2]), conv(c4, c5, 3, true), c2f(c5, c5, m.rep[3]);
    conv(c5, c5 / 2, 1, true), conv(2 * c5, c5, 1, true);
    c2f(c5 + c4, c4, m.neck_rep), c2f(c4 + c3, c3, m.neck_rep), conv(c3, c3, 3, true), c2f(c3 + c4, c4, m.neck_rep);
    conv(c4, c4, 3, true), c2f(c4 + c5, c5, m.neck_rep);
    const int hb = std::max(16, std::max(c3 / 4, 4 * REG_MAX)), hc = std::max(c3, std::min(m.nc, 100));
    for (int ch : {c3, c4, c5}) {
        conv(ch, hb, 3, true), conv(hb, hb, 3, true), conv(hb, 4 * REG_MAX, 1, false);
        conv(ch, hc, 3, true), conv(hc, hc, 3, true), conv(hc, m.nc, 1, false);
    }
    return n;
}

size_t av_yolo_param_count(void) {
    // the (n, 80) preset; must equal oracle/yolo_ref.py: param_count() = 3167776
    av_yolo_model m;
    return av_yolo_model_preset('n', NC, &m) == AV_OK ? av_yolo_model_param_count(&m) : 0;
}

int av_yolo_destroy(av_yolo* h) {
    if (!h) return AV_OK;
    for (void* p : h->y.allocs) (void)hipFree(p);
    if (h->y.side) (void)hipStreamDestroy(h->y.side);
    if (h->y.tail) (void)hipStreamDestroy(h->y.tail);
    if (h->y.ev_heads) (void)hipEventDestroy(h->y.ev_heads);
    if (h->y.ev_tail) (void)hipEventDestroy(h->y.ev_tail);
    if (h->y.ev_fork) (void)hipEventDestroy(h->y.ev_fork);
    if (h->y.ev_join) (void)hipEventDestroy(h->y.ev_join);
    delete h;
    return AV_OK;
}

int av_yolo_create(av_ctx* ctx, int batch, int in_h, int in_w, const float* weights, size_t n_weights, av_yolo** out) {
    return av_yolo_create_ex(ctx, batch, in_h, in_w, weights, n_weights, AV_YOLO_FP16, out);
}

int av_yolo_create_ex(av_ctx* ctx, int batch, int in_h, int in_w, const float* weights, size_t n_weights, int precision, av_yolo** out) {
    av_yolo_model m;
    const int rc = av_yolo_model_preset('n', NC, &m);
    return rc != AV_OK ? rc : av_yolo_create_model(ctx, batch, in_h, in_w, &m, weights, n_weights, precision, out);
}

int av_yolo_create_model(av_ctx* ctx, int batch, int in_h, int in_w, const av_yolo_model* model, const float* weights, size_t n_weights,
                         int precision, av_yolo** out) {
    AV_REQUIRE(ctx && weights && out && model, AV_EINVAL, "av_yolo_create: null argument");
    AV_REQUIRE(precision == AV_YOLO_FP16 || precision == AV_YOLO_FP32, AV_EINVAL, "av_yolo_create_ex: unknown precision %d", precision);
    AV_REQUIRE(batch > 0 && in_h >= 32 && in_w >= 32, AV_EINVAL, "av_yolo_create: bad shape");
    AV_REQUIRE(model_ok(*model), AV_EINVAL, "av_yolo_create_model: widths %d %d %d %d %d, repeats %d %d %d %d / %d, nc %d is not a preset of scale n, s or m with 1 .. 256 classes",
               model->ch[0], model->ch[1], model->ch[2], model->ch[3], model->ch[4], model->rep[0], model->rep[1], model->rep[2], model->rep[3],
               model->neck_rep, model->nc);
    AV_REQUIRE(n_weights == av_yolo_model_param_count(model), AV_EINVAL, "av_yolo_create: expected %zu parameters, got %zu",
               av_yolo_model_param_count(model), n_weights);
    AV_HIP(hipSetDevice(ctx->device));
    av_yolo* h = new (std::nothrow) av_yolo();
    AV_REQUIRE(h, AV_ENOMEM, "av_yolo_create: out of host memory");
    Yolo& y = h->y;
    y.model = *model;
    y.ctx = ctx, y.B = batch, y.inH = in_h, y.inW = in_w, y.wsrc = weights, y.wtotal = n_weights;
    y.f32 = precision == AV_YOLO_FP32;
    letterbox(in_h, in_w, y.gain, y.nh, y.nw, y.top, y.left, y.H, y.W);
    const int rc = [&]() -> int {
        const int rg = build_graph(y);
        if (rg != AV_OK) return rg;
        AV_HIP(hipStreamCreateWithFlags(&y.side, hipStreamNonBlocking));
        AV_HIP(hipEventCreateWithFlags(&y.ev_fork, hipEventDisableTiming));
        AV_HIP(hipEventCreateWithFlags(&y.ev_join, hipEventDisableTiming));
        for (const Variant& v : kVariants)
            if (v.lds_limit) AV_HIP(hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, v.lds_limit));
        // the first plan: a shape that no kernel serves fails here, not at the first forward
        y.plan_hooks = read_hooks(), y.plan_keep_logits = y.keep_logits;
        return plan_forward(y, y.plan_hooks, y.plan_keep_logits, y.plan, y.decode_alone);
    }();
    if (rc != AV_OK) {
        av_yolo_destroy(h);
        return rc;
    }
    (void)hipDeviceSynchronize();
    *out = h;
    return AV_OK;
}

int av_yolo_model_of(const av_yolo* h, av_yolo_model* model) {
    AV_REQUIRE(h && model, AV_EINVAL, "av_yolo_model_of: null argument");
    *model = h->y.model;
    return AV_OK;
}

int av_yolo_dims(const av_yolo* h, int* net_h, int* net_w, int* n_anchors) {
    AV_REQUIRE(h && net_h && net_w && n_anchors, AV_EINVAL, "av_yolo_dims: null argument");
    *net_h = h->y.H, *net_w = h->y.W, *n_anchors = h->y.A;
    return AV_OK;
}

// test hook: NHWC half slice of an intermediate tensor (ids follow the yolov8.yaml layer numbers; 0 = input)
int av_yolo_tensor(const av_yolo* h, int id, void** ptr, int* H, int* W, int* C, int* cstride, int* coff) {
    AV_REQUIRE(h && ptr && H && W && C && cstride && coff, AV_EINVAL, "av_yolo_tensor: null argument");
    if (id >= 100 && id < 106) {            // head outputs (float32): 100+2i box, 101+2i cls
        const int i = (id - 100) / 2;
        *ptr = (id & 1) ? (void*)h->y.head_cls[i] : (void*)h->y.head_box[i];
        *H = h->y.lvH[i], *W = h->y.lvW[i], *C = (id & 1) ? h->y.model.nc : 4 * REG_MAX, *cstride = (id & 1) ? h->y.ncp : *C, *coff = 0;      // (channels [nc, cstride): 0.0f)
        return AV_OK;
    }
    if (id >= 110 && id < 113) {            // candidates written by the head's decode epilogues: box [A][4], confidence [A], class [A] (int32)
        *ptr = id == 110 ? (void*)h->y.cbox : (id == 111 ? (void*)h->y.cconf : (void*)h->y.ccls);
        *H = 1, *W = h->y.A, *C = id == 110 ? 4 : 1, *cstride = *C, *coff = 0;
        return AV_OK;
    }
    if (id >= 120 && id < 123) {            // the same from decode_kernel on the kept logits (av_yolo_keep_logits)
        AV_REQUIRE(h->y.dbg_cbox, AV_EINVAL, "av_yolo_tensor: candidates of the stand-alone decode exist only after av_yolo_keep_logits(h, 1)");
        *ptr = id == 120 ? (void*)h->y.dbg_cbox : (id == 121 ? (void*)h->y.dbg_cconf : (void*)h->y.dbg_ccls);
        *H = 1, *W = h->y.A, *C = id == 120 ? 4 : 1, *cstride = *C, *coff = 0;
        return AV_OK;
    }
    for (const auto& kv : h->y.named)
        if (kv.first == id) {
            const Buf& b = h->y.bufs[kv.second.buf];
            *ptr = b.p, *H = b.H, *W = b.W, *C = kv.second.c, *cstride = b.C, *coff = kv.second.coff;
            return AV_OK;
        }
    av_set_error("av_yolo_tensor: unknown tensor id %d", id);
    return AV_EINVAL;
}

// test hook: the ops as build_graph made them (reads host memory only)
static_assert(sizeof(av_yolo_slice) == 32 && sizeof(av_yolo_op_info) == 184 && offsetof(av_yolo_op_info, wgt) == 168, "what _native.py binds");
int av_yolo_op_count(const av_yolo* h, int* n_ops) {
    AV_REQUIRE(h && n_ops, AV_EINVAL, "av_yolo_op_count: null argument");
    *n_ops = (int)h->y.ops.size();
    return AV_OK;
}

int av_yolo_op(const av_yolo* h, int k, av_yolo_op_info* info) {
    AV_REQUIRE(h && info, AV_EINVAL, "av_yolo_op: null argument");
    const Yolo& y = h->y;
    AV_REQUIRE(k >= 0 && k < (int)y.ops.size(), AV_EINVAL, "av_yolo_op: op %d of %d", k, (int)y.ops.size());
    const Yolo::Op& op = y.ops[k];
    const int f32 = y.f32 ? 1 : 0;
    av_yolo_op_info o{};
    auto of_slice = [&](Slice s, int H, int W) {
        const Buf& b = y.bufs[s.buf];
        return av_yolo_slice{b.p, H, W, b.C, s.coff, s.c, f32};
    };
    // the members ConvArgs and ConvArgsF share
    auto of_conv = [&](const auto& a) {
        o.kind = AV_YOLO_OP_CONV, o.ksz = a.ksz, o.stride = a.stride, o.act = a.act, o.cin = a.cin, o.cout = a.cout;
        o.in = av_yolo_slice{a.in, a.H, a.W, a.in_cs, a.in_coff, a.cin, f32};
        o.cout = op.cout_real;                               // (a.cout counts the zero filters of a padded class branch too)
        o.out = av_yolo_slice{a.out, a.Ho, a.Wo, a.out_cs, a.out_coff, o.cout, f32};
        if (a.res) o.res = av_yolo_slice{a.res, a.Ho, a.Wo, a.res_cs, a.res_coff, o.cout, f32};
        o.wgt = a.wgt, o.bias = a.bias;
    };
    switch (op.kind) {
    case OP_CONV_F32:
        of_conv(op.cf);
        o.kpad = o.kreal = op.cf.ksz * op.cf.ksz * op.cf.cin, o.wgt_f32 = 1;
        break;
    case OP_CONV:
    case OP_STEM:
        of_conv(op.ca);
        o.kpad = op.ca.kpad, o.kreal = op.ca.kreal;
        if (op.ca.out32) o.out.ptr = op.ca.out32, o.out.f32 = 1;
        if (op.kind == OP_STEM) o.kind = AV_YOLO_OP_STEM, o.in_frame = 1, o.in.H += 2, o.in.W += 2;
        if (k > 0 && y.ops[k - 1].kind == OP_UPSAMPLE && y.ops[k - 1].vcat == k && reads_upsample(y, y.ops[k - 1], op))
            o.in2 = of_slice(y.ops[k - 1].in, y.ops[k - 1].H, y.ops[k - 1].W);
        break;
    case OP_POOLS:
    case OP_MAXPOOL:
    case OP_UPSAMPLE: {
        const int up = op.kind == OP_UPSAMPLE ? 2 : 1;
        o.kind = op.kind == OP_POOLS ? AV_YOLO_OP_POOLS : (op.kind == OP_MAXPOOL ? AV_YOLO_OP_MAXPOOL : AV_YOLO_OP_UPSAMPLE);
        o.ksz = op.kind == OP_UPSAMPLE ? 0 : 5, o.stride = 1, o.cin = op.in.c, o.cout = op.out.c;
        o.in = of_slice(op.in, op.H, op.W), o.out = of_slice(op.out, up * op.H, up * op.W);
        break;
    }
    }
    *info = o;
    return AV_OK;
}

static_assert(sizeof(av_yolo_step_info) == 72 && sizeof(av_yolo_model) == 64, "what _native.py binds");
static_assert(AV_YOLO_K_MFMA == K_MFMA && AV_YOLO_K_GEMM128 == K_GEMM128 && AV_YOLO_K_LDS == K_LDS && AV_YOLO_K_WS3 == K_WS3 && AV_YOLO_K_WS1 == K_WS1 &&
              AV_YOLO_K_GEMM_F32 == K_GEMM_F32 && AV_YOLO_K_STEM_F32 == K_STEM_F32 && AV_YOLO_K_FIXED == K_FIXED, "family ids of avhot.h");
static_assert(AV_YOLO_WHEN_ALWAYS == ALWAYS && AV_YOLO_WHEN_BGR_ALIGNED == BGR_ALIGNED && AV_YOLO_WHEN_BGR_UNALIGNED == BGR_UNALIGNED, "avhot.h");
int av_yolo_plan_count(const av_yolo* h, int* n_steps) {
    AV_REQUIRE(h && n_steps, AV_EINVAL, "av_yolo_plan_count: null argument");
    *n_steps = (int)h->y.plan.size();
    return AV_OK;
}

int av_yolo_plan_step(const av_yolo* h, int k, av_yolo_step_info* info) {
    AV_REQUIRE(h && info, AV_EINVAL, "av_yolo_plan_step: null argument");
    const std::vector<Step>& plan = h->y.plan;
    AV_REQUIRE(k >= 0 && k < (int)plan.size(), AV_EINVAL, "av_yolo_plan_step: step %d of %d", k, (int)plan.size());
    const Step& s = plan[k];
    av_yolo_step_info o{};
    o.family = s.fam, o.first_op = s.first_op, o.n_ops = s.n_ops, o.when = (int)s.when;
    o.grid[0] = (int)s.grid.x, o.grid[1] = (int)s.grid.y, o.grid[2] = (int)s.grid.z;
    o.block[0] = (int)s.block.x, o.block[1] = (int)s.block.y, o.block[2] = (int)s.block.z;
    o.lds_bytes = (int)s.lds, o.lane = s.lane;
    std::copy(s.var, s.var + 6, o.variant);
    *info = o;
    return AV_OK;
}

// The tail of a forward on `st`: threshold + sort, then greedy NMS + scale_boxes, of the candidates cbox / cconf / ccls ([B][A] in the
// handle's geometry) through the handle's scratch (sbox / sidx / scount).  av_yolo_forward passes the head's candidates, av_yolo_tail
// the caller's.
static int launch_tail(Yolo& y, hipStream_t st, const float* cbox, const float* cconf, const int* ccls, float conf_thres, float iou_thres,
                       int max_det, int32_t* det_n, float* det_box, float* det_conf, int32_t* det_cls) {
    const int B = y.B;
    {
        const int rounds = (y.A + 1023) / 1024;
        if (rounds <= 7) hipLaunchKernelGGL(nms_sort_kernel<8>, dim3(B), dim3(1024), rs_lds(rounds, 8), st, y.A, rounds, conf_thres, cbox, cconf, ccls, y.sbox, y.sidx, y.scount);
        else hipLaunchKernelGGL(nms_sort_kernel<7>, dim3(B), dim3(1024), rs_lds(rounds, 7), st, y.A, rounds, conf_thres, cbox, cconf, ccls, y.sbox, y.sidx, y.scount);
    }
    AV_LAUNCH_CHECK();
    // gain/pad of ultralytics scale_boxes
    const float gain = std::fmin((float)y.H / y.inH, (float)y.W / y.inW);
    const float padx = (float)std::lround((y.W - y.inW * gain) / 2 - 0.1), pady = (float)std::lround((y.H - y.inH * gain) / 2 - 0.1);
    const size_t nms_lds = (size_t)max_det * 24;
    hipLaunchKernelGGL(nms_greedy_kernel, dim3(B), dim3(64 * NMS_WAVES), nms_lds, st, y.A, max_det, iou_thres, y.sbox, y.scount, y.sidx,
                       cbox, cconf, ccls, gain, padx, pady, (float)y.inW, (float)y.inH, det_n, det_box, det_conf, det_cls);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int av_yolo_forward(av_yolo* h, av_stream_t stream, const uint8_t* bgr, float conf_thres, float iou_thres, int max_det,
                    int32_t* det_n, float* det_box, float* det_conf, int32_t* det_cls) {
    AV_REQUIRE(h && bgr && det_n && det_box && det_conf && det_cls, AV_EINVAL, "av_yolo_forward: null argument");
    AV_REQUIRE(max_det > 0 && max_det <= 2500 && conf_thres > 0.f, AV_EINVAL,
               "av_yolo_forward: max_det must be in [1,2500] (kept boxes live in LDS) and conf_thres > 0");
    Yolo& y = h->y;
    AV_REQUIRE(!(y.f32 && y.defer_tail), AV_ESTATE, "av_yolo_forward: the float32 mode has no deferred tail");
    const hipStream_t st_main = as_stream(stream);
    const int B = y.B;
    const Hooks hk = read_hooks();
    if (y.plan.empty() || !(hk == y.plan_hooks) || y.keep_logits != y.plan_keep_logits) {
        y.plan_hooks = hk, y.plan_keep_logits = y.keep_logits;
        const int rc = plan_forward(y, hk, y.keep_logits, y.plan, y.decode_alone);
        if (rc != AV_OK) {
            y.plan.clear();
            return rc;
        }
    }
    const When skip = (reinterpret_cast<uintptr_t>(bgr) & 3) == 0 ? BGR_UNALIGNED : BGR_ALIGNED;
    bool forked = false;
    for (Step& s : y.plan) {
        if (s.when == skip) continue;
        if (s.head) {
            if (y.tail_pending)                            // the previous forward's sort + NMS must be done with the candidates the head rewrites
                AV_HIP(hipStreamWaitEvent(st_main, y.ev_tail, 0));
            AV_HIP(hipEventRecord(y.ev_fork, st_main));    // backbone + neck done on the caller's stream: open the side lane
            AV_HIP(hipStreamWaitEvent(y.side, y.ev_fork, 0));
            forked = true;
        }
        if (s.takes_bgr) memcpy(s.params, &bgr, sizeof bgr);
        void* argv[12];
        for (int i = 0; i < s.nargs; ++i) argv[i] = s.params + s.off[i];
        AV_HIP(hipLaunchKernel(s.fn, s.grid, s.block, argv, s.lds, s.lane ? y.side : st_main));
    }
    if (forked) {                                          // the decode reads both branches
        AV_HIP(hipEventRecord(y.ev_join, y.side));
        AV_HIP(hipStreamWaitEvent(st_main, y.ev_join, 0));
    }
    hipStream_t st = st_main;
    if (y.defer_tail) {                                    // the rest goes to the tail stream, behind the head
        AV_HIP(hipEventRecord(y.ev_heads, st_main));
        AV_HIP(hipStreamWaitEvent(y.tail, y.ev_heads, 0));
        st = y.tail;
    }
    Level lv[3];
    int aoff = 0;
    const int strides[3] = {8, 16, 32};
    for (int i = 0; i < 3; ++i) {
        lv[i] = Level{y.head_box[i], y.head_cls[i], y.lvH[i], y.lvW[i], strides[i], aoff};
        aoff += y.lvH[i] * y.lvW[i];
    }
    // The candidates (cbox / cconf / ccls) were written by the head's last convolutions.  With keep_logits the stand-alone
    // decode runs as well, from the float32 logits into buffers of its own: the test hook that shows the two are equal.
    // the 80-class model keeps its compile-time count; any other takes nc and the padded stride at run time
    auto decode = [&](float* cbox, float* cconf, int* ccls) {
        const auto kernel = y.model.nc == NC ? decode_kernel<NC> : decode_kernel<0>;
        hipLaunchKernelGGL(kernel, dim3((B * y.A + 127) / 128), dim3(128), 0, st, lv[0], lv[1], lv[2], y.A, B, cbox, cconf, ccls, y.model.nc, y.ncp);
    };
    if (y.f32 || y.decode_alone) {                         // no decode epilogue (the float32 chain; head shapes without one): the stand-alone decode IS the decode
        decode(y.cbox, y.cconf, y.ccls);
        AV_LAUNCH_CHECK();
    }
    if (!y.f32 && y.keep_logits) {
        decode(y.dbg_cbox, y.dbg_cconf, y.dbg_ccls);
        AV_LAUNCH_CHECK();
    }
    {
        const int rc = launch_tail(y, st, y.cbox, y.cconf, y.ccls, conf_thres, iou_thres, max_det, det_n, det_box, det_conf, det_cls);
        if (rc != AV_OK) return rc;
    }
    if (y.defer_tail) {
        AV_HIP(hipEventRecord(y.ev_tail, st));
        y.tail_pending = true;
    }
    return AV_OK;
}

// test hook: the forward's tail on the caller's candidates
int av_yolo_tail(av_yolo* h, av_stream_t stream, const float* cand_box, const float* cand_conf, const int32_t* cand_cls, float conf_thres,
                 float iou_thres, int max_det, int32_t* det_n, float* det_box, float* det_conf, int32_t* det_cls) {
    AV_REQUIRE(h && cand_box && cand_conf && cand_cls && det_n && det_box && det_conf && det_cls, AV_EINVAL, "av_yolo_tail: null argument");
    AV_REQUIRE(max_det > 0 && max_det <= 2500 && conf_thres > 0.f, AV_EINVAL,
               "av_yolo_tail: max_det must be in [1,2500] (kept boxes live in LDS) and conf_thres > 0");
    Yolo& y = h->y;
    AV_REQUIRE(!y.tail_pending, AV_ESTATE, "av_yolo_tail: a deferred tail of this handle is pending (it uses the same scratch): av_yolo_join_tail first");
    return launch_tail(y, as_stream(stream), cand_box, cand_conf, cand_cls, conf_thres, iou_thres, max_det, det_n, det_box, det_conf, det_cls);
}

int av_yolo_keep_logits(av_yolo* h, int enable) {
    AV_REQUIRE(h, AV_EINVAL, "av_yolo_keep_logits: null handle");
    Yolo& y = h->y;
    if (enable && !y.dbg_cbox) {
        const size_t n = (size_t)y.B * y.A;
        if (!dev_alloc(y, (void**)&y.dbg_cbox, n * 16) || !dev_alloc(y, (void**)&y.dbg_cconf, n * 4) || !dev_alloc(y, (void**)&y.dbg_ccls, n * 4)) {
            av_set_error("av_yolo_keep_logits: device allocation failed");
            return AV_ENOMEM;
        }
    }
    y.keep_logits = enable != 0;
    return AV_OK;
}

int av_yolo_defer_tail(av_yolo* h, int enable) {
    AV_REQUIRE(h, AV_EINVAL, "av_yolo_defer_tail: null handle");
    Yolo& y = h->y;
    if (enable && !y.tail) {
        AV_HIP(hipStreamCreateWithFlags(&y.tail, hipStreamNonBlocking));
        AV_HIP(hipEventCreateWithFlags(&y.ev_heads, hipEventDisableTiming));
        AV_HIP(hipEventCreateWithFlags(&y.ev_tail, hipEventDisableTiming));
    }
    y.defer_tail = enable != 0;
    return AV_OK;
}

int av_yolo_join_tail(av_yolo* h, av_stream_t stream) {
    AV_REQUIRE(h, AV_EINVAL, "av_yolo_join_tail: null handle");
    if (h->y.tail_pending) {
        AV_HIP(hipStreamWaitEvent(as_stream(stream), h->y.ev_tail, 0));
        h->y.tail_pending = false;
    }
    return AV_OK;
}

}  // extern "C"
