// The lens model's device and host side (include/avhot.h: av_lens_cfg): OpenCV's five-coefficient Brown-Conrady distortion, its
// Jacobian, and the undistortion of a raw pixel by six Newton iterations, shared by the map builders (lens.hip) and the lens form
// of av_track_obstacles_ground (obstacles.hip).  float64, every operation rounded on its own, in the order the header states.
#pragma once
#include "common.h"

namespace lensdev {

struct Distorted {
    double xd, yd;      // the distorted normalised point
    double a, b, d;     // its Jacobian [[a, b], [b, d]] with respect to (x, y)
};

// c: the five coefficients k1, k2, p1, p2, k3 (av_lens_cfg's order; a wave-uniform table entry is read through scalar loads)
__host__ __device__ __forceinline__ void distort(const double* __restrict__ c, double x, double y, double* xd, double* yd) {
    const double k1 = c[0], k2 = c[1], p1 = c[2], p2 = c[3], k3 = c[4];
    const double r2 = x * x + y * y;
    const double rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3));
    *xd = x * rad + (2 * p1 * x * y + p2 * (r2 + 2 * x * x));
    *yd = y * rad + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y);
}

__host__ __device__ __forceinline__ Distorted distort_jac(const double* __restrict__ c, double x, double y) {
    const double k1 = c[0], k2 = c[1], p1 = c[2], p2 = c[3], k3 = c[4];
    const double r2 = x * x + y * y;
    const double rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3));
    Distorted o;
    o.xd = x * rad + (2 * p1 * x * y + p2 * (r2 + 2 * x * x));
    o.yd = y * rad + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y);
    const double drad = k1 + r2 * (2 * k2 + r2 * (3 * k3));
    o.a = rad + 2 * x * x * drad + (2 * p1 * y + 6 * p2 * x);
    o.b = 2 * x * y * drad + (2 * p1 * x + 2 * p2 * y);
    o.d = rad + 2 * y * y * drad + (6 * p1 * y + 2 * p2 * x);
    return o;
}

constexpr int NEWTON_ITERATIONS = 6;
constexpr double RESIDUAL_MAX = 1e-20;      // on ex^2 + ey^2, normalised units

struct Undistorted {
    double x, y;            // the undistorted normalised point
    double u, v;            // the rectified pixel (nfx*x + ncx, nfy*y + ncy)
    double a, b, d, det;    // the model's Jacobian at (x, y) and its determinant
    bool valid;             // det > 0 at every iterate and at the result, and the residual small  (a NaN fails)
};

__host__ __device__ __forceinline__ Undistorted undistort(const av_lens_cfg* __restrict__ L, double ru, double rv) {
    const double* c = &L->k1;
    const double xd = (ru - L->cx) / L->fx, yd = (rv - L->cy) / L->fy;
    Undistorted o;
    o.x = xd, o.y = yd;
    bool ok = true;
    for (int it = 0; it < NEWTON_ITERATIONS; ++it) {
        const Distorted m = distort_jac(c, o.x, o.y);
        const double ex = m.xd - xd, ey = m.yd - yd;
        const double det = m.a * m.d - m.b * m.b;
        ok = ok && det > 0.0;
        o.x = o.x - (m.d * ex - m.b * ey) / det;
        o.y = o.y - (m.a * ey - m.b * ex) / det;
    }
    const Distorted m = distort_jac(c, o.x, o.y);
    const double ex = m.xd - xd, ey = m.yd - yd;
    o.a = m.a, o.b = m.b, o.d = m.d;
    o.det = m.a * m.d - m.b * m.b;
    o.valid = ok && o.det > 0.0 && ex * ex + ey * ey <= RESIDUAL_MAX;
    o.u = L->nfx * o.x + L->ncx, o.v = L->nfy * o.y + L->ncy;
    return o;
}

// the Jacobian raw pixel -> rectified pixel at an undistorted point
struct LensJac {
    double juu, juv, jvu, jvv;
};
__host__ __device__ __forceinline__ LensJac jacobian(const av_lens_cfg* __restrict__ L, const Undistorted& p) {
    LensJac j;
    j.juu = (p.d / p.det) * (L->nfx / L->fx), j.juv = (-p.b / p.det) * (L->nfx / L->fy);
    j.jvu = (-p.b / p.det) * (L->nfy / L->fx), j.jvv = (p.a / p.det) * (L->nfy / L->fy);
    return j;
}

// a raw-frame position in 1/65536 pixels as a map entry: (-1, -1) outside the frame (a NaN too)
__host__ __device__ __forceinline__ void map_entry(double u, double v, int w, int h, int32_t* tu, int32_t* tv) {
    const double fu = floor(u * 65536.0 + 0.5), fv = floor(v * 65536.0 + 0.5);
    // (inside these bounds both are exact integers below 2^31: w, h <= 32768)
    const bool in = fu >= 0.0 && fu <= (double)(w - 1) * 65536.0 && fv >= 0.0 && fv <= (double)(h - 1) * 65536.0;
    *tu = in ? (int32_t)fu : -1, *tv = in ? (int32_t)fv : -1;
}

}  // namespace lensdev
