// The pair test that av_rig_fuse (rig.hip) and av_rig_track (rigtrack.hip) share: the squared distance on the road and the gate,
// in the operation order include/avhot.h states for both.
#pragma once
#include "common.h"

// (X, Y, R): the cluster or slot; (x, y, r): the candidate.  True when the pair is admissible (a NaN d2 never is; an infinite one
// is turned away by the caller's `d2 < best`, whose best starts at +inf).
__device__ __forceinline__ bool rig_pair(double X, double Y, double R, double x, double y, double r, double gate_min, double gate_scale,
                                         double& d2) {
    const double dx = X - x, dy = Y - y;
    d2 = dx * dx + dy * dy;
    const double gate = fmax(gate_min, gate_scale * fmax(R, r));
    return d2 <= gate * gate;
}
