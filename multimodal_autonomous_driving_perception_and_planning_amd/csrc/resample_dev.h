// What the kernels that make a picture by sampling another one share: av_ground_warp (ground.hip), av_remap (lens.hip),
// av_rig_surround (surround.hip) and the ground odometry's patch stage (egoflow.hip).  The tile: a thread makes four adjacent pixels
// of one output row, a 256-thread workgroup 64 columns x 16 rows (neighbouring output pixels read neighbouring source pixels: a
// tile's taps share cache lines in both directions); grid.z is the caller's.  The store: 12 bytes at once, a row's tail byte by byte.
// The sample: rasterdev::resize_channel's bilinear rule at a position in 1/65536 pixel, in two forms that return the same bytes
// (__host__ __device__: tests/resample_check.cpp holds them against each other on the host).
#pragma once
#include "common.h"
#include "raster_dev.h"

namespace resample {

constexpr int TILE_W = 64, TILE_H = 16, PX = 4;     // pixels per tile row, rows per tile, pixels per thread

// the thread's row, first column and number of pixels (1 .. PX) of a dh x dw picture; false for a thread outside it.  (Inside, the
// mask changes nothing: it shows the compiler that c0 >= 0, which saves the nearest surround kernel a wave of occupancy.)
__device__ __forceinline__ bool tile_thread(int dh, int dw, int& r, int& c0, int& npx) {
    r = blockIdx.y * TILE_H + (int)(threadIdx.x / (TILE_W / PX));
    const long long c0l = (long long)blockIdx.x * TILE_W + (int)(threadIdx.x % (TILE_W / PX)) * PX;
    c0 = (int)(c0l & 0x7fffffff);
    npx = min(PX, dw - c0);
    return r < dh && c0l < dw;
}

__device__ __forceinline__ void store_px1(uint8_t* __restrict__ o, unsigned p) {
    o[0] = (uint8_t)p, o[1] = (uint8_t)(p >> 8), o[2] = (uint8_t)(p >> 16);
}
// the first npx of four adjacent pixels (b | g << 8 | r << 16 each): one 12-byte store at any alignment, or the row's tail byte by byte
__device__ __forceinline__ void store_px4(uint8_t* __restrict__ o, const unsigned (&px)[PX], int npx) {
    if (npx == PX) {
        const unsigned words[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
        __builtin_memcpy(o, words, 12);
    } else {
#pragma unroll
        for (int j = 0; j < PX - 1; ++j)
            if (j < npx) store_px1(o + j * 3, px[j]);
    }
}

// The two horizontally adjacent taps of one source row as b | g << 8 | r << 16 each.  They are six contiguous bytes, fetched as a
// 4-byte and a 2-byte load at whatever alignment they have (two loads per row in place of five byte and short gathers): pixels
// xa = min(x0, sw - 2) and xa + 1, so that at the frame's right edge, where x1 == x0 == sw - 1, nothing past the row is read.
// Needs sw >= 2; bytes [3 xa, 3 xa + 6) lie inside the row because xa + 1 <= sw - 1.
struct RowTaps { unsigned p0, p1; };
__host__ __device__ __forceinline__ RowTaps row_taps(const uint8_t* __restrict__ row, int x0, int sw) {
    const int xa = min(x0, sw - 2);
    unsigned lo;
    unsigned short hi;
    __builtin_memcpy(&lo, row + (size_t)xa * 3, 4);
    __builtin_memcpy(&hi, row + (size_t)xa * 3 + 4, 2);
    RowTaps t;
    t.p1 = (lo >> 24) | ((unsigned)hi << 8);
    t.p0 = x0 == xa ? (lo & 0xffffffu) : t.p1;
    return t;
}

// rasterdev::resize_channel's rule on one channel of the four taps, in unsigned arithmetic: the horizontal blends are below 2^24,
// the vertical one is a 32 x 32 -> 64 bit multiply-add; the same integers as the rule's 64-bit products, term by term
__host__ __device__ __forceinline__ unsigned blend(unsigned p00, unsigned p01, unsigned p10, unsigned p11, unsigned wx, unsigned wy) {
    const unsigned top = p00 * (65536u - wx) + p01 * wx, bot = p10 * (65536u - wx) + p11 * wx;
    return (unsigned)(((unsigned long long)top * (65536u - wy) + (unsigned long long)bot * wy + (1ull << 31)) >> 32);
}

// the picture src [sh][sw][3] at (tu, tv) / 65536, 0 <= tu <= (sw - 1) << 16 and 0 <= tv <= (sh - 1) << 16 (the caller's check), as
// b | g << 8 | r << 16.  WIDE: row_taps and blend, needs sw >= 2; otherwise tap by tap through resize_channel itself.  T: int32_t
// (a table entry) or long long (warp_position's).
template <bool WIDE, typename T>
__host__ __device__ __forceinline__ unsigned bilinear_bgr(const uint8_t* __restrict__ src, int sh, int sw, T tu, T tv) {
    rasterdev::ResizeTap t;
    t.x0 = (int)(tu >> 16), t.wx = (int)(tu & 65535), t.x1 = min(t.x0 + 1, sw - 1);     // 0 <= x0 <= sw - 1
    t.y0 = (int)(tv >> 16), t.wy = (int)(tv & 65535), t.y1 = min(t.y0 + 1, sh - 1);     // 0 <= y0 <= sh - 1
    if constexpr (WIDE) {
        const RowTaps a = row_taps(src + (size_t)t.y0 * sw * 3, t.x0, sw), b = row_taps(src + (size_t)t.y1 * sw * 3, t.x0, sw);
        unsigned px = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            px |= blend((a.p0 >> (8 * k)) & 255u, (a.p1 >> (8 * k)) & 255u, (b.p0 >> (8 * k)) & 255u, (b.p1 >> (8 * k)) & 255u,
                        (unsigned)t.wx, (unsigned)t.wy) << (8 * k);
        return px;
    } else {
        return (unsigned)rasterdev::resize_channel(src, sw, t, 0) | ((unsigned)rasterdev::resize_channel(src, sw, t, 1) << 8) |
               ((unsigned)rasterdev::resize_channel(src, sw, t, 2) << 16);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
inline unsigned pack_bgr(const uint8_t fill[3]) { return (unsigned)fill[0] | ((unsigned)fill[1] << 8) | ((unsigned)fill[2] << 16); }
// the grid of tiles for n_z pictures of dh x dw (all >= 1), or the refusal in the words of entry `who`, whose n_z counts `what`
inline int tile_grid(int dw, int dh, int n_z, const char* who, const char* what, dim3* grid) {
    const long long tiles_y = ((long long)dh + TILE_H - 1) / TILE_H;
    AV_REQUIRE(n_z <= 65535 && tiles_y <= 65535, AV_EINVAL, "%s: more than 65535 %s or tile rows", who, what);
    *grid = dim3((unsigned)(((long long)dw + TILE_W - 1) / TILE_W), (unsigned)tiles_y, (unsigned)n_z);
    return AV_OK;
}
// do [a, a + na) and [b, b + nb) share a byte?  (128 bits: neither a byte count nor an end address wraps)
inline bool overlap(const void* a, unsigned __int128 na, const void* b, unsigned __int128 nb) {
    const unsigned __int128 pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace resample
