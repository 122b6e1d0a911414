// Baseline JPEG encode on the device (include/avhot.h: av_jpeg_encode_header / av_jpeg_encode).
//   front    one workgroup per strip of 64 x (8 or 16) pixels: BGR read once, colour conversion, edge replication and chroma
//            downsampling in LDS, jfdctint "islow" with eight lanes per block, quantisation; int16 coefficients in zigzag order,
//            blocks in scan order, dummy blocks resolved
//   size     one lane per block: its bit count (the DC predecessor is read from the coefficient buffer)
//   scan     one wave per restart interval: exclusive prefix sum of the bit counts, the interval's unstuffed byte length
//   prefix   one workgroup per frame: where each interval's unstuffed bytes start
//   zero     the used part of the unstuffed streams
//   pack     one lane per block: its codes at its bit offset (dwords shared with a neighbour by atomic OR), 1-bits behind an interval
//   count    one wave per interval: FF bytes -> stuffed length
//   prefix   again, over the stuffed lengths and the restart markers; len and status
//   gather   one wave per interval: stuffed bytes, RST marker, header copy and EOI to their final places, never beyond the slot
// No workgroup waits for another one.  Every index into the caller's buffers comes from the geometry of (h, w, subsampling,
// restart_mcus), which av_jpeg_encode checks; offsets read back from the workspace are clamped to the stream capacity.
#include "common.h"
#include "jpeg_enc_dev.h"

namespace {

using jpege::Geom;

struct Izz {
    uint8_t v[64];
};
constexpr Izz make_izz() {
    Izz t{};
    const uint8_t zz[64] = {JPEG_ZIGZAG};
    for (int i = 0; i < 64; ++i) t.v[zz[i]] = (uint8_t)i;
    return t;
}
__constant__ jpege::Tables c_tables = jpege::make_tables();
__constant__ Izz c_izz = make_izz();                      // natural index -> zigzag position

// workspace of a batch: coef i16 [n][n_blocks][64] | bits u32 [n][n_blocks] | iv u32 [n][4][ivs] | tot u32 [n][4] | stream [n][cap]
enum { IV_UBYTES = 0, IV_USTART = 1, IV_SBYTES = 2, IV_SSTART = 3 };
struct Ws {
    int16_t* coef;
    uint32_t* bits;
    uint32_t* iv;
    uint32_t* tot;
    uint8_t* stream;
    uint32_t cap;             // bytes of one frame's unstuffed stream area
    int ivs;                  // entries of one interval array
    size_t bytes;
};
Ws layout(void* base, int n, const Geom& g) {
    Ws s;
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    uint8_t* p = static_cast<uint8_t*>(base);
    size_t o = 0;
    s.ivs = (g.n_mcus + 3) & ~3;
    s.cap = (uint32_t)jpege::stream_cap(g.n_blocks, g.n_mcus);
    s.coef = reinterpret_cast<int16_t*>(p + o), o += (size_t)n * g.n_blocks * 128;
    s.bits = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n * g.n_blocks * 4);
    s.iv = reinterpret_cast<uint32_t*>(p + o), o += (size_t)n * 4 * s.ivs * 4;
    s.tot = reinterpret_cast<uint32_t*>(p + o), o += (size_t)n * 16;
    s.stream = p + o, o += (size_t)n * s.cap;
    s.bytes = o;
    return s;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane_id() >= o) v += u;
    }
    return v;
}

// ---- jfdctint "islow", one dimension: rows first (outputs scaled up by 4), then columns -------------------------------------------
template <bool ROWS>
__device__ __forceinline__ void fdct8(const int (&d)[8], int (&o)[8]) {
    constexpr int SH = ROWS ? 11 : 15, R = 1 << (SH - 1);
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (ROWS) o[0] = (tmp10 + tmp11) * 4, o[4] = (tmp10 - tmp11) * 4;
    else o[0] = (tmp10 + tmp11 + 2) >> 2, o[4] = (tmp10 - tmp11 + 2) >> 2;
    int z1 = (tmp12 + tmp13) * 4433;
    o[2] = (z1 + tmp13 * 6270 + R) >> SH, o[6] = (z1 - tmp12 * 15137 + R) >> SH;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    o[7] = (t4 + z1 + z3 + R) >> SH, o[5] = (t5 + z2 + z4 + R) >> SH, o[3] = (t6 + z2 + z3 + R) >> SH, o[1] = (t7 + z1 + z4 + R) >> SH;
}

constexpr int TW = 64;        // pixels per strip row
constexpr int TBLK = 24;      // blocks per strip at most: 4 MCUs of 6 (4:2:0), 4 of 4 (4:2:2), 8 of 3 (4:4:4)

// luma block j of MCU (mx, my) holds no real pixel?
__device__ __forceinline__ bool is_dummy(const Geom& g, int mx, int my, int j) {
    return j < g.nl && (mx * g.hs + j % g.hs >= g.nbx || my * g.vs + j / g.hs >= g.nby);
}

__global__ __launch_bounds__(256) void jpege_front_kernel(Geom g, int h, int w, const uint8_t* __restrict__ bgr, int vec,
                                                          const uint8_t* __restrict__ qt, int16_t* __restrict__ coef) {
    __shared__ uint32_t sP[3][16][TW / 4];        // Y, Cb, Cr at full resolution, four samples per dword
    __shared__ uint8_t sC[2][8][TW];              // the chroma planes as the DCT reads them
    __shared__ int sW[TBLK][8][9];
    __shared__ __attribute__((aligned(16))) int16_t sZ[TBLK][64];
    __shared__ uint32_t sQ[2][64], sR[2][64];     // 8 q, and ceil(2^32 / 8 q)
    const int t = threadIdx.x, f = blockIdx.z, my = blockIdx.y;
    const int mpt = TW / (8 * g.hs), mx0 = blockIdx.x * mpt, th = 8 * g.vs, x0 = mx0 * 8 * g.hs;
    if (t < 128) {
        const uint32_t q = qt[t], q8 = 8 * (q ? q : 1);
        sQ[t >> 6][t & 63] = q8, sR[t >> 6][t & 63] = (uint32_t)((((uint64_t)1 << 32) + q8 - 1) / q8);
    }
    if ((t >> 4) < th) {
        const int ty = t >> 4, gy = min(my * th + ty, h - 1), gx0 = x0 + (t & 15) * 4;
        const uint8_t* row = bgr + ((size_t)f * h + gy) * w * 3;
        uint8_t px[12];
        if (vec && gx0 + 3 < w) {
            const uint32_t* r4 = reinterpret_cast<const uint32_t*>(row + (size_t)gx0 * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t v = r4[k];
                px[4 * k] = v & 255, px[4 * k + 1] = (v >> 8) & 255, px[4 * k + 2] = (v >> 16) & 255, px[4 * k + 3] = v >> 24;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint8_t* p = row + (size_t)min(gx0 + k, w - 1) * 3;
                px[3 * k] = p[0], px[3 * k + 1] = p[1], px[3 * k + 2] = p[2];
            }
        }
        uint32_t y4 = 0, cb4 = 0, cr4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = px[3 * k], gg = px[3 * k + 1], r = px[3 * k + 2];
            y4 |= (uint32_t)((19595 * r + 38470 * gg + 7471 * b + 32768) >> 16) << (8 * k);
            cb4 |= (uint32_t)((-11058 * r - 21710 * gg + 32768 * b + (128 << 16) + 32767) >> 16) << (8 * k);
            cr4 |= (uint32_t)((32768 * r - 27439 * gg - 5329 * b + (128 << 16) + 32767) >> 16) << (8 * k);
        }
        sP[0][ty][t & 15] = y4, sP[1][ty][t & 15] = cb4, sP[2][ty][t & 15] = cr4;
    }
    __syncthreads();
    {   // chroma: downsample the edge-replicated full-resolution rows; rows below the real chroma extent repeat its last row
        const uint8_t(*full)[16][TW] = reinterpret_cast<const uint8_t(*)[16][TW]>(&sP[0][0][0]);
        const int cwt = TW / g.hs;
        for (int i = t; i < 2 * 8 * cwt; i += 256) {
            const int c = i / (8 * cwt), r = (i / cwt) & 7, x = i % cwt;
            int v;
            if (g.hs == 1) {
                v = full[1 + c][r][x];
            } else if (g.vs == 1) {
                v = (full[1 + c][r][2 * x] + full[1 + c][r][2 * x + 1] + (x & 1)) >> 1;
            } else {
                const int rl = min(r, g.ch - 1 - my * 8);
                v = (full[1 + c][2 * rl][2 * x] + full[1 + c][2 * rl][2 * x + 1] + full[1 + c][2 * rl + 1][2 * x] + full[1 + c][2 * rl + 1][2 * x + 1] + 1 +
                     (x & 1)) >> 2;
            }
            sC[c][r][x] = (uint8_t)v;
        }
    }
    __syncthreads();
    const int nblk = min(mpt, g.mcus_x - mx0) * g.bpm;
    const int blk = t >> 3, m = blk / g.bpm, j = blk - m * g.bpm;
    bool dummy = false;
    if (blk < nblk) {       // rows: lane (block, r)
        int js = j;
        while (is_dummy(g, mx0 + m, my, js)) --js, dummy = true;      // a dummy block takes the DC of the block coded before it
        const int r = t & 7;
        const uint8_t* src;
        if (js < g.nl) src = reinterpret_cast<const uint8_t*>(&sP[0][0][0]) + ((js / g.hs) * 8 + r) * TW + (m * g.hs + js % g.hs) * 8;
        else src = &sC[js - g.nl][r][m * 8];
        int d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)src[k] - 128;
        fdct8<true>(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) sW[blk][r][k] = o[k];
    }
    __syncthreads();
    if (blk < nblk) {       // columns: lane (block, c), then quantisation
        const int c = t & 7, tq = j >= g.nl;
        int d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = sW[blk][k][c];
        fdct8<false>(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nat = k * 8 + c;
            const uint32_t a = (uint32_t)abs(o[k]) + (sQ[tq][nat] >> 1);
            const int q = (int)__umulhi(a, sR[tq][nat]);
            sZ[blk][c_izz.v[nat]] = (int16_t)(dummy && nat ? 0 : (o[k] < 0 ? -q : q));
        }
    }
    __syncthreads();
    if (t < nblk * 8) {
        uint4* dst = reinterpret_cast<uint4*>(coef + ((size_t)f * g.n_blocks + (size_t)(my * g.mcus_x + mx0) * g.bpm) * 64);
        dst[t] = reinterpret_cast<const uint4*>(&sZ[0][0])[t];
    }
}

__device__ __forceinline__ void tables_to_lds(jpege::Tables& T) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&c_tables);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&T);
    for (int i = threadIdx.x; i < (int)(sizeof(jpege::Tables) / 4); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

__global__ __launch_bounds__(256) void jpege_size_kernel(Geom g, const int16_t* __restrict__ coef, uint32_t* __restrict__ bits) {
    __shared__ jpege::Tables T;
    tables_to_lds(T);
    const int f = blockIdx.y, blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= g.n_blocks) return;
    const int16_t* fc = coef + (size_t)f * g.n_blocks * 64;
    const int pb = jpege::pred_block(g, blk);
    jpege::CountSink s;
    jpege::code_block(T, fc + (size_t)blk * 64, pb < 0 ? 0 : (int)fc[(size_t)pb * 64], blk % g.bpm >= g.nl, s);
    bits[(size_t)f * g.n_blocks + blk] = s.bits;
}

__global__ __launch_bounds__(64) void jpege_scan_kernel(Geom g, uint32_t* __restrict__ bits, uint32_t* __restrict__ iv, int ivs) {
    const int f = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    const int b0 = i * g.ri * g.bpm, b1 = min((i + 1) * g.ri, g.n_mcus) * g.bpm;
    uint32_t* fb = bits + (size_t)f * g.n_blocks;
    uint32_t run = 0;
    for (int base = b0; base < b1; base += 64) {
        const int idx = base + lane;
        const uint32_t v = idx < b1 ? fb[idx] : 0, inc = wave_incl_scan(v);
        if (idx < b1) fb[idx] = run + inc - v;
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) iv[((size_t)f * 4 + IV_UBYTES) * ivs + i] = (run + 7) >> 3;
}

// out[i] = sum of in[k] (+ add for every k but the last) over k < i; the total goes to tot[f][slot].  With len: the frame's length
// and its status word.
__global__ __launch_bounds__(256) void jpege_prefix_kernel(int n_int, uint32_t* __restrict__ iv, int ivs, int k_in, int k_out, uint32_t add,
                                                           uint32_t* __restrict__ tot, int slot, int header_len, int out_cap,
                                                           int32_t* __restrict__ len, int32_t* __restrict__ status) {
    __shared__ uint32_t wsum[4];
    const int f = blockIdx.x, t = threadIdx.x;
    const uint32_t* in = iv + ((size_t)f * 4 + k_in) * ivs;
    uint32_t* out = iv + ((size_t)f * 4 + k_out) * ivs;
    uint32_t run = 0;
    for (int base = 0; base < n_int; base += 256) {
        const int i = base + t;
        const uint32_t v = i < n_int ? in[i] + (i < n_int - 1 ? add : 0) : 0, inc = wave_incl_scan(v);
        if ((t & 63) == 63) wsum[t >> 6] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) before += k < (t >> 6) ? wsum[k] : 0, all += wsum[k];
        if (i < n_int) out[i] = run + before + inc - v;
        run += all;
        __syncthreads();
    }
    if (t == 0) {
        tot[f * 4 + slot] = run;
        if (len) {
            const int64_t L = (int64_t)header_len + run + 2;
            len[f] = (int32_t)(L < 0x7FFFFFFF ? L : 0x7FFFFFFF);
            status[f] = L > out_cap ? AV_JPEG_EFULL : 0;
        }
    }
}

__global__ __launch_bounds__(256) void jpege_zero_kernel(const uint32_t* __restrict__ tot, uint8_t* __restrict__ stream, uint32_t cap) {
    const int f = blockIdx.y;
    const uint32_t used = min(tot[f * 4 + 0], cap), n16 = (used + 15) / 16;
    uint4* s4 = reinterpret_cast<uint4*>(stream + (size_t)f * cap);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n16; i += gridDim.x * 256) s4[i] = make_uint4(0, 0, 0, 0);
}

struct AtomicStore {
    __device__ void merge(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
    __device__ void own(uint32_t* p, uint32_t v) const { *p = v; }
};

__global__ __launch_bounds__(256) void jpege_pack_kernel(Geom g, const int16_t* __restrict__ coef, const uint32_t* __restrict__ bits,
                                                         const uint32_t* __restrict__ iv, int ivs, uint8_t* __restrict__ stream, uint32_t cap) {
    __shared__ jpege::Tables T;
    tables_to_lds(T);
    const int f = blockIdx.y, blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= g.n_blocks) return;
    const int16_t* fc = coef + (size_t)f * g.n_blocks * 64;
    const int pb = jpege::pred_block(g, blk), i = (blk / g.bpm) / g.ri;
    const uint64_t at = (uint64_t)iv[((size_t)f * 4 + IV_USTART) * ivs + i] * 8 + bits[(size_t)f * g.n_blocks + blk];
    jpege::WordSink<AtomicStore> s(AtomicStore(), reinterpret_cast<uint32_t*>(stream + (size_t)f * cap), at, cap / 4);
    jpege::code_block(T, fc + (size_t)blk * 64, pb < 0 ? 0 : (int)fc[(size_t)pb * 64], blk % g.bpm >= g.nl, s);
    s.finish(blk + 1 == min((i + 1) * g.ri, g.n_mcus) * g.bpm);
}

// the unstuffed bytes of interval i of frame f, clamped to the frame's stream area
__device__ __forceinline__ const uint8_t* interval_bytes(const uint32_t* iv, int ivs, const uint8_t* stream, uint32_t cap, int f, int i, uint32_t& n) {
    const uint32_t s0 = min(iv[((size_t)f * 4 + IV_USTART) * ivs + i], cap);
    n = min(iv[((size_t)f * 4 + IV_UBYTES) * ivs + i], cap - s0);
    return stream + (size_t)f * cap + s0;
}

__global__ __launch_bounds__(64) void jpege_count_kernel(uint32_t* __restrict__ iv, int ivs, const uint8_t* __restrict__ stream, uint32_t cap) {
    const int f = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    uint32_t n;
    const uint8_t* src = interval_bytes(iv, ivs, stream, cap, f, i, n);
    uint32_t ff = 0;
    for (uint32_t off = lane * 4; off < n; off += 256) ff += jpege::count_ff(src + off, min(4u, n - off));
    ff = __shfl(wave_incl_scan(ff), 63, 64);
    if (lane == 0) iv[((size_t)f * 4 + IV_SBYTES) * ivs + i] = n + ff;
}

__global__ __launch_bounds__(64) void jpege_gather_kernel(int n_int, const uint32_t* __restrict__ iv, int ivs, const uint32_t* __restrict__ tot,
                                                          const uint8_t* __restrict__ stream, uint32_t cap, const uint8_t* __restrict__ header,
                                                          int header_len, uint8_t* __restrict__ out, int out_cap) {
    const int f = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
    uint32_t n;
    const uint8_t* src = interval_bytes(iv, ivs, stream, cap, f, i, n);
    uint8_t* dst = out + (size_t)f * out_cap;
    const int64_t limit = out_cap, pos0 = (int64_t)header_len + iv[((size_t)f * 4 + IV_SSTART) * ivs + i];
    uint32_t run = 0;
    for (uint32_t base = 0; base < n; base += 256) {
        const uint32_t off = base + lane * 4, m = off < n ? min(4u, n - off) : 0;
        const uint32_t c = jpege::count_ff(src + off, m), inc = wave_incl_scan(c);
        jpege::stuff_bytes(src + off, m, dst, pos0 + off + run + inc - c, limit);
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0 && i < n_int - 1) {
        const int64_t p = pos0 + n + run;
        if (p < limit) dst[p] = 0xFF;
        if (p + 1 < limit) dst[p + 1] = (uint8_t)(0xD0 + (i & 7));
    }
    if (i == 0)
        for (int k = lane; k < header_len && k < out_cap; k += 64) dst[k] = header[k];
    if (lane == 0 && i == n_int - 1) {
        const int64_t p = (int64_t)header_len + tot[f * 4 + 1];
        if (p < limit) dst[p] = 0xFF;
        if (p + 1 < limit) dst[p + 1] = 0xD9;
    }
}

}  // namespace

extern "C" {

int av_jpeg_encode_header(int h, int w, int quality, int subsampling, int restart_mcus, uint8_t* out, int cap, uint8_t qt[2][64]) {
    AV_REQUIRE(out && qt, AV_EINVAL, "av_jpeg_encode_header: null argument");
    Geom g;
    AV_REQUIRE(quality >= 1 && quality <= 100 && jpege::geom(h, w, subsampling, restart_mcus, g), AV_EINVAL,
               "av_jpeg_encode_header: bad size %dx%d, quality %d, subsampling %d or restart_mcus %d", w, h, quality, subsampling, restart_mcus);
    uint8_t q[2][64];
    const int n = jpege::write_header(h, w, quality, subsampling, restart_mcus, out, cap, q);
    AV_REQUIRE(n > 0, AV_EINVAL, "av_jpeg_encode_header: the header does not fit in %d bytes", cap);
    memcpy(qt, q, sizeof q);
    return n;
}

size_t av_jpeg_encode_workspace_bytes(int n_frames, int h, int w, int subsampling) {
    Geom g;
    if (n_frames <= 0 || n_frames > 65535 || !jpege::geom(h, w, subsampling, 0, g)) return 0;
    return layout(nullptr, n_frames, g).bytes;
}

int av_jpeg_encode(av_ctx* ctx, av_stream_t stream, int n_frames, int h, int w, const uint8_t* bgr, const uint8_t* qt, int subsampling,
                   int restart_mcus, const uint8_t* header, int header_len, void* workspace, uint8_t* out, int out_cap, int32_t* len,
                   int32_t* status) {
    AV_REQUIRE(ctx && bgr && qt && header && workspace && out && len && status, AV_EINVAL, "av_jpeg_encode: null argument");
    Geom g;
    AV_REQUIRE(n_frames > 0 && n_frames <= 65535 && jpege::geom(h, w, subsampling, restart_mcus, g), AV_EINVAL,
               "av_jpeg_encode: bad batch %d x %dx%d, subsampling %d or restart_mcus %d", n_frames, w, h, subsampling, restart_mcus);
    AV_REQUIRE(header_len >= 0 && header_len <= jpege::HEADER_MAX && out_cap >= 0, AV_EINVAL, "av_jpeg_encode: bad header_len %d or out_cap %d",
               header_len, out_cap);
    AV_REQUIRE(((uintptr_t)workspace & 15) == 0, AV_EINVAL, "av_jpeg_encode: workspace misaligned");
    const Ws s = layout(workspace, n_frames, g);
    hipStream_t st = as_stream(stream);
    const unsigned nf = (unsigned)n_frames, nb = (unsigned)((g.n_blocks + 255) / 256), ni = (unsigned)g.n_int;
    const int mpt = TW / (8 * g.hs), vec = w % 4 == 0 && ((uintptr_t)bgr & 3) == 0;
    hipLaunchKernelGGL(jpege_front_kernel, dim3((unsigned)((g.mcus_x + mpt - 1) / mpt), (unsigned)g.mcus_y, nf), dim3(256), 0, st, g, h, w, bgr, vec,
                       qt, s.coef);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpege_size_kernel, dim3(nb, nf), dim3(256), 0, st, g, s.coef, s.bits);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpege_scan_kernel, dim3(ni, nf), dim3(64), 0, st, g, s.bits, s.iv, s.ivs);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpege_prefix_kernel, dim3(nf), dim3(256), 0, st, g.n_int, s.iv, s.ivs, (int)IV_UBYTES, (int)IV_USTART, 0u, s.tot, 0, 0, 0,
                       (int32_t*)nullptr, (int32_t*)nullptr);
    AV_LAUNCH_CHECK();
    const unsigned nz = (unsigned)((s.cap / 4096 + 1) < 64 ? (s.cap / 4096 + 1) : 64);
    hipLaunchKernelGGL(jpege_zero_kernel, dim3(nz, nf), dim3(256), 0, st, s.tot, s.stream, s.cap);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpege_pack_kernel, dim3(nb, nf), dim3(256), 0, st, g, s.coef, s.bits, s.iv, s.ivs, s.stream, s.cap);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpege_count_kernel, dim3(ni, nf), dim3(64), 0, st, s.iv, s.ivs, s.stream, s.cap);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpege_prefix_kernel, dim3(nf), dim3(256), 0, st, g.n_int, s.iv, s.ivs, (int)IV_SBYTES, (int)IV_SSTART, 2u, s.tot, 1, header_len,
                       out_cap, len, status);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(jpege_gather_kernel, dim3(ni, nf), dim3(64), 0, st, g.n_int, s.iv, s.ivs, s.tot, s.stream, s.cap, header, header_len, out,
                       out_cap);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

}  // extern "C"
