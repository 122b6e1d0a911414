// Baseline JPEG decode on the device (include/avhot.h: av_jpeg_parse / av_jpeg_decode).
//   clear     zero the coefficients a frame uses, status = what the parse flagged
//   entropy   one lane per (frame, restart segment); the frame's Huffman tables in LDS; sparse int16 stores into the zeroed area
//   idct      one thread per 8 x 8 block: dequantise, jidctint "islow", u8 samples into per-component planes (MCU-padded)
//   convert   four pixels per thread: fancy chroma upsampling, YCbCr -> BGR, the output written once
// No workgroup waits for another one; every loop is bounded by the frame geometry or a segment's byte range (jpeg_dev.h).
#include "common.h"
#include "jpeg_dev.h"

namespace {

using jpeg::Geom;

static_assert(sizeof(av_jpeg_desc) == AV_JPEG_DESC_BYTES, "av_jpeg_desc layout");
static_assert(sizeof(av_jpeg_seg) == 8, "av_jpeg_seg layout");

// workspace: coefficients i16 [n][cap][64], then samples u8 [n][cap][64]; cap = jpeg::cap_blocks(h, w)
// total: entries of the batch's segment table; max_per_frame: lanes per frame of the entropy launch (max_segs).  A frame with more
// segments than that is not decoded at all (AV_JPEG_EDESC), rather than left with rows of gray that no status bit tells of
struct SegLimits {
    int total, max_per_frame;
};
__device__ __forceinline__ bool frame_ok(const av_jpeg_desc& d, int h, int w, SegLimits lim, Geom& g) {
    return jpeg::geom_from(d, h, w, g) && d.seg_base >= 0 && d.seg_base <= lim.total && d.n_segments <= lim.total - d.seg_base &&
           d.n_segments <= lim.max_per_frame;
}

__global__ __launch_bounds__(256) void jpeg_clear_kernel(const av_jpeg_desc* __restrict__ desc, SegLimits lim, int h, int w, int cap,
                                                         int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    const int f = blockIdx.y;
    Geom g;
    const bool ok = frame_ok(desc[f], h, w, lim, g);
    if (blockIdx.x == 0 && threadIdx.x == 0) status[f] = ok ? (desc[f].flags & AV_JPEG_ESEGS) : AV_JPEG_EDESC;
    if (!ok) return;
    uint4* dst = reinterpret_cast<uint4*>(coef + (size_t)f * cap * 64);
    const int n = g.n_blocks * 8;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const av_jpeg_desc* __restrict__ desc, const av_jpeg_seg* __restrict__ segs,
                                                          SegLimits lim, const uint32_t* __restrict__ words, uint32_t byte_limit, int h, int w,
                                                          int cap, int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    __shared__ jpeg::Tables T;
    const int f = blockIdx.y;
    const av_jpeg_desc& d = desc[f];
    Geom g;
    const bool ok = frame_ok(d, h, w, lim, g);
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (!ok || (int)blockIdx.x * 64 >= d.n_segments) return;           // the same in every lane of the workgroup
    if (threadIdx.x < 4) jpeg::build_table(d, T, threadIdx.x);
    else if (threadIdx.x == 4) jpeg::build_zigzag(T);
    __syncthreads();
    if (i >= d.n_segments) return;
    const av_jpeg_seg s = segs[d.seg_base + i];
    const uint64_t b0 = (uint64_t)d.byte_base + s.begin, b1 = (uint64_t)d.byte_base + s.end;
    const uint32_t end = (uint32_t)(b1 < byte_limit ? b1 : byte_limit);
    const uint32_t begin = (uint32_t)(b0 < end ? b0 : end);
    const int ri = d.restart_interval;
    const int e = jpeg::decode_segment(d, g, T, words, begin, end, ri > 0 ? i * ri : 0, ri > 0 ? ri : g.n_mcus, coef + (size_t)f * cap * 64);
    if (e) atomicOr(&status[f], e);
}

// ---- jidctint "islow", one dimension, 32-bit wrapping arithmetic ---------------------------------------------------------------
__device__ __forceinline__ int wmul(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
__device__ __forceinline__ int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int wsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int wshl13(int a) { return (int)((unsigned)a << 13); }

template <int SHIFT>
__device__ __forceinline__ void idct8(const int (&in)[8], int (&out)[8]) {
    int z1 = wmul(wadd(in[2], in[6]), 4433);
    int tmp2 = wsub(z1, wmul(in[6], 15137)), tmp3 = wadd(z1, wmul(in[2], 6270));
    int tmp0 = wshl13(wadd(in[0], in[4])), tmp1 = wshl13(wsub(in[0], in[4]));
    const int tmp10 = wadd(tmp0, tmp3), tmp13 = wsub(tmp0, tmp3), tmp11 = wadd(tmp1, tmp2), tmp12 = wsub(tmp1, tmp2);
    tmp0 = in[7], tmp1 = in[5], tmp2 = in[3], tmp3 = in[1];
    z1 = wadd(tmp0, tmp3);
    int z2 = wadd(tmp1, tmp2), z3 = wadd(tmp0, tmp2), z4 = wadd(tmp1, tmp3);
    const int z5 = wmul(wadd(z3, z4), 9633);
    tmp0 = wmul(tmp0, 2446), tmp1 = wmul(tmp1, 16819), tmp2 = wmul(tmp2, 25172), tmp3 = wmul(tmp3, 12299);
    z1 = wmul(z1, -7373), z2 = wmul(z2, -20995), z3 = wadd(wmul(z3, -16069), z5), z4 = wadd(wmul(z4, -3196), z5);
    tmp0 = wadd(tmp0, wadd(z1, z3)), tmp1 = wadd(tmp1, wadd(z2, z4)), tmp2 = wadd(tmp2, wadd(z2, z3)), tmp3 = wadd(tmp3, wadd(z1, z4));
    constexpr int R = 1 << (SHIFT - 1);
    out[0] = wadd(wadd(tmp10, tmp3), R) >> SHIFT, out[7] = wadd(wsub(tmp10, tmp3), R) >> SHIFT;
    out[1] = wadd(wadd(tmp11, tmp2), R) >> SHIFT, out[6] = wadd(wsub(tmp11, tmp2), R) >> SHIFT;
    out[2] = wadd(wadd(tmp12, tmp1), R) >> SHIFT, out[5] = wadd(wsub(tmp12, tmp1), R) >> SHIFT;
    out[3] = wadd(wadd(tmp13, tmp0), R) >> SHIFT, out[4] = wadd(wsub(tmp13, tmp0), R) >> SHIFT;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const av_jpeg_desc* __restrict__ desc, SegLimits lim, int h, int w, int cap,
                                                        const int16_t* __restrict__ coef, uint8_t* __restrict__ samples) {
    __shared__ uint8_t q[4][64];
    const int f = blockIdx.y;
    const av_jpeg_desc& d = desc[f];
    Geom g;
    if (!frame_ok(d, h, w, lim, g) || (int)blockIdx.x * 256 >= g.n_blocks) return;
    if (threadIdx.x < 64) reinterpret_cast<uint32_t*>(&q[0][0])[threadIdx.x] = reinterpret_cast<const uint32_t*>(&d.qt[0][0])[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= g.n_blocks) return;
    const int c = b >= g.off[2] && g.ncomp == 3 ? 2 : (b >= g.off[1] && g.ncomp == 3 ? 1 : 0);
    const int rb = b - g.off[c], by = rb / g.bw[c], bx = rb - by * g.bw[c];
    const uint8_t* qc = q[d.tq[c] & 3];
    const uint4* src = reinterpret_cast<const uint4*>(coef + ((size_t)f * cap + b) * 64);
    int ws[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const uint4 v = src[r];
        const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ws[r][2 * k] = (int)(int16_t)(u[k] & 0xFFFF) * (int)qc[r * 8 + 2 * k];
            ws[r][2 * k + 1] = (int)(int16_t)(u[k] >> 16) * (int)qc[r * 8 + 2 * k + 1];
        }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {
        int in[8], out[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = ws[r][col];
        idct8<11>(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r][col] = out[r];
    }
    const int pitch = g.bw[c] * 8;
    uint8_t* plane = samples + ((size_t)f * cap + g.off[c]) * 64 + ((size_t)by * 8) * pitch + bx * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int out[8];
        idct8<18>(ws[r], out);
        uint2 o;
        o.x = clamp255(out[0] + 128) | (clamp255(out[1] + 128) << 8) | (clamp255(out[2] + 128) << 16) | (clamp255(out[3] + 128) << 24);
        o.y = clamp255(out[4] + 128) | (clamp255(out[5] + 128) << 8) | (clamp255(out[6] + 128) << 16) | (clamp255(out[7] + 128) << 24);
        *reinterpret_cast<uint2*>(plane + (size_t)r * pitch) = o;
    }
}

// t[k] = the vertically filtered chroma sample of column i0 - 1 + k (columns clamped to the real extent), times 4 for 4:2:0
__device__ __forceinline__ void chroma_taps(const uint8_t* __restrict__ near, const uint8_t* __restrict__ far, int i0, int cw, bool v2, int (&t)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = min(max(i0 - 1 + k, 0), cw - 1);
        t[k] = v2 ? 3 * (int)near[i] + (int)far[i] : (int)near[i];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void jpeg_convert_kernel(const av_jpeg_desc* __restrict__ desc, SegLimits lim, int h, int w, int cap,
                                                           const uint8_t* __restrict__ samples, uint8_t* __restrict__ bgr) {
    const int f = blockIdx.y, w4 = (w + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= h * w4) return;
    const int y = idx / w4, x0 = (idx - y * w4) * 4;
    Geom g;
    const bool ok = frame_ok(desc[f], h, w, lim, g);
    int Y[4], cb[4], cr[4];
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = 128, cb[k] = cr[k] = 0;
    } else {
        const uint8_t* base = samples + (size_t)f * cap * 64;
        const int p0 = g.bw[0] * 8;
        const uint32_t yy = *reinterpret_cast<const uint32_t*>(base + (size_t)y * p0 + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = (int)((yy >> (8 * k)) & 255), cb[k] = cr[k] = 0;
        if (g.ncomp == 3) {
            const int p1 = g.bw[1] * 8;
            const uint8_t* pb = base + (size_t)g.off[1] * 64;
            const uint8_t* pr = base + (size_t)g.off[2] * 64;
            if (g.hs == 1) {
                const uint32_t ub = *reinterpret_cast<const uint32_t*>(pb + (size_t)y * p1 + x0);
                const uint32_t ur = *reinterpret_cast<const uint32_t*>(pr + (size_t)y * p1 + x0);
#pragma unroll
                for (int k = 0; k < 4; ++k) cb[k] = (int)((ub >> (8 * k)) & 255) - 128, cr[k] = (int)((ur >> (8 * k)) & 255) - 128;
            } else {
                const bool v2 = g.vs == 2;
                const int cy = v2 ? y >> 1 : y;
                const int fy = v2 ? min(max((y & 1) ? cy + 1 : cy - 1, 0), g.ch - 1) : cy;
                const int i0 = x0 >> 1;
                int tb[4], tr[4];
                chroma_taps(pb + (size_t)cy * p1, pb + (size_t)fy * p1, i0, g.cw, v2, tb);
                chroma_taps(pr + (size_t)cy * p1, pr + (size_t)fy * p1, i0, g.cw, v2, tr);
                // the filters see the clamped neighbours only where a real neighbour is missing
                const int r0 = v2 ? 8 : 1, r1 = v2 ? 7 : 2, sh = v2 ? 4 : 2;
                cb[0] = ((3 * tb[1] + tb[0] + r0) >> sh) - 128, cb[1] = ((3 * tb[1] + tb[2] + r1) >> sh) - 128;
                cb[2] = ((3 * tb[2] + tb[1] + r0) >> sh) - 128, cb[3] = ((3 * tb[2] + tb[3] + r1) >> sh) - 128;
                cr[0] = ((3 * tr[1] + tr[0] + r0) >> sh) - 128, cr[1] = ((3 * tr[1] + tr[2] + r1) >> sh) - 128;
                cr[2] = ((3 * tr[2] + tr[1] + r0) >> sh) - 128, cr[3] = ((3 * tr[2] + tr[3] + r1) >> sh) - 128;
            }
        }
    }
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[3 * k] = (uint8_t)clamp255(Y[k] + ((116130 * cb[k] + 32768) >> 16));
        px[3 * k + 1] = (uint8_t)clamp255(Y[k] + ((-22554 * cb[k] - 46802 * cr[k] + 32768) >> 16));
        px[3 * k + 2] = (uint8_t)clamp255(Y[k] + ((91881 * cr[k] + 32768) >> 16));
    }
    uint8_t* o = bgr + ((size_t)f * h * w + (size_t)y * w + x0) * 3;
    if (VEC) {                                   // w % 4 == 0 and a 4-byte aligned output: every thread owns 12 aligned bytes
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k) o4[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        const int n = min(4, w - x0) * 3;
        for (int k = 0; k < n; ++k) o[k] = px[k];
    }
}

}  // namespace

extern "C" {

int av_jpeg_parse(const uint8_t* data, size_t len, int h, int w, av_jpeg_desc* desc, av_jpeg_seg* segs, int seg_cap, int* n_segs) {
    AV_REQUIRE(data && desc && segs && n_segs, AV_EINVAL, "av_jpeg_parse: null argument");
    AV_REQUIRE(h > 0 && w > 0 && h <= 65535 && w <= 65535 && seg_cap > 0, AV_EINVAL, "av_jpeg_parse: bad size %dx%d or seg_cap %d", w, h, seg_cap);
    const char* why = "";
    const int rc = jpeg::parse(data, len, h, w, desc, segs, seg_cap, n_segs, &why);
    if (rc != AV_OK) av_set_error("av_jpeg_parse: %s", why);
    return rc;
}

size_t av_jpeg_workspace_bytes(int n_frames, int h, int w) {
    if (n_frames <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535) return 0;
    return (size_t)n_frames * jpeg::cap_blocks(h, w) * (128 + 64);
}

int av_jpeg_decode(av_ctx* ctx, av_stream_t stream, int n_frames, int h, int w, const av_jpeg_desc* desc, const av_jpeg_seg* segs,
                   int n_segs_total, int max_segs, const uint8_t* bytes, size_t n_bytes, void* workspace, uint8_t* bgr, int32_t* status) {
    AV_REQUIRE(ctx && desc && segs && bytes && workspace && bgr && status, AV_EINVAL, "av_jpeg_decode: null argument");
    AV_REQUIRE(n_frames > 0 && n_frames <= 65535 && h > 0 && w > 0 && h <= 65535 && w <= 65535, AV_EINVAL, "av_jpeg_decode: bad batch %d x %dx%d",
               n_frames, w, h);
    AV_REQUIRE(n_segs_total > 0 && max_segs > 0 && max_segs <= n_segs_total, AV_EINVAL, "av_jpeg_decode: bad segment counts");
    AV_REQUIRE(n_bytes >= 8 && n_bytes <= 0xFFFFFFF0u, AV_EINVAL, "av_jpeg_decode: n_bytes must hold 8 bytes of padding and stay below 4 GiB");
    AV_REQUIRE(((uintptr_t)bytes & 3) == 0 && ((uintptr_t)workspace & 15) == 0, AV_EINVAL, "av_jpeg_decode: bytes / workspace misaligned");
    AV_REQUIRE((size_t)h * w < ((size_t)1 << 31) / 4, AV_EINVAL, "av_jpeg_decode: frame too large");
    const int cap = jpeg::cap_blocks(h, w);
    int16_t* coef = static_cast<int16_t*>(workspace);
    uint8_t* samples = reinterpret_cast<uint8_t*>(coef + (size_t)n_frames * cap * 64);
    hipStream_t s = as_stream(stream);
    const unsigned nf = (unsigned)n_frames;
    const SegLimits lim{n_segs_total, max_segs};
    hipLaunchKernelGGL(jpeg_clear_kernel, dim3((unsigned)((cap * 8 + 1023) / 1024), nf), dim3(256), 0, s, desc, lim, h, w, cap, coef, status);
    AV_LAUNCH_CHECK();
    // a reader may touch the whole dword that holds its segment's last byte: keep those inside n_bytes
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((max_segs + 63) / 64), nf), dim3(64), 0, s, desc, segs, lim,
                       reinterpret_cast<const uint32_t*>(bytes), (uint32_t)(n_bytes - 4), h, w, cap, coef, status);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((cap + 255) / 256), nf), dim3(256), 0, s, desc, lim, h, w, cap, coef, samples);
    AV_LAUNCH_CHECK();
    const dim3 cgrid((unsigned)((h * ((w + 3) / 4) + 255) / 256), nf);
    if (w % 4 == 0 && ((uintptr_t)bgr & 3) == 0)
        hipLaunchKernelGGL(jpeg_convert_kernel<true>, cgrid, dim3(256), 0, s, desc, lim, h, w, cap, samples, bgr);
    else
        hipLaunchKernelGGL(jpeg_convert_kernel<false>, cgrid, dim3(256), 0, s, desc, lim, h, w, cap, samples, bgr);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"
