// Gradient clipping by global norm: the device code every launch that decides a clip coefficient shares (the step tail with
// clipping in train_tail.hip, the host-driven step's resolve launch in grad_clip.hip), so S, norm and coef are stated once and the
// two step paths are bit-equal.  Definition: include/mindpose_hip.h, "gradient clipping by global norm".
#pragma once
#include "common.h"

namespace mp {

constexpr int kNormThreads = 256;
constexpr int kNormSpan = 4 * kNormThreads;  // quads one workgroup reads per trip: four 16-byte loads per lane
constexpr int kNormBlocksCap = 256 * 8;  // the finite check's cap: every workgroup of a full grid is resident at once (8 per CU)

// Sum over the 64 lanes in a fixed pattern; lane 0 holds it.  (A lane whose source is past the wave reads itself: those sums
// never reach lane 0.)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// S of a launch of ONE wave: lane l adds partials l, l + 64, ... in index order, then the lanes are added.  Lane 0 holds it.
__device__ __forceinline__ double clip_sum_partials(const double* __restrict__ partials, int n_partials) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += kWave) s += partials[i];
    return wave_sum_f64(s);
}

struct ClipDecision {
    double norm, coef;
    bool clipped;
};

__device__ __forceinline__ ClipDecision clip_decide(double sum_sq, double base, double clip_norm) {
    ClipDecision d;
    d.norm = sqrt(sum_sq) * base;
    d.clipped = isfinite(d.norm) && d.norm > clip_norm;
    d.coef = d.clipped ? clip_norm / d.norm : 1.0;
    return d;
}

// a step that was not skipped
__device__ __forceinline__ void clip_record(mp_grad_clip_state* __restrict__ cs, const ClipDecision& d) {
    cs->last_norm = d.norm;
    cs->norm_sum += d.norm;
    if (d.norm > cs->norm_max) cs->norm_max = d.norm;
    cs->measured_steps += 1;
    if (d.clipped) cs->clipped_steps += 1;
}

}  // namespace mp
