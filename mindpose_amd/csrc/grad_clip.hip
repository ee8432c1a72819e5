// Gradient clipping by global norm (include/mindpose_hip.h, "gradient clipping by global norm"): the overflow check and the sum of
// squares of the gradient arena as ONE read of it, and the single-workgroup launch that turns the partial sums into norm and clip
// coefficient for a host-driven step.  The device-resident step decides the same in its tail launch (train_tail.hip) through the
// same device functions (grad_clip.h).  Nothing here scales a gradient: the coefficient is a factor of the gradient scale the update
// kernels apply while reading the arena.
//
// The reference trains without clipping; the definition is mindspore.ops.clip_by_global_norm's (clip_norm / norm when norm >
// clip_norm, no epsilon), the `clip_grad` / `clip_value` keys are those of the sibling mindcv recipes.
#include "grad_clip.h"

namespace mp {
namespace {

__device__ __forceinline__ double add_sq(double acc, float x) {
    const double d = (double)x;
    return acc + d * d;  // the product is exact: fused or not, one rounding
}

__device__ __forceinline__ double quad_sq(double acc, const float4& v) { return add_sq(add_sq(add_sq(add_sq(acc, v.x), v.y), v.z), v.w); }

// One fp64 accumulator per thread, its quads added in index order whatever the batching of the loads; grid = f(count) (the launcher).
// The accumulator is also the overflow check: the square of a finite fp32 value is below 2^256 and 2^64 of them cannot reach fp64's
// 2^1024, so the sum of finite values is finite; inf gives inf, NaN gives NaN, and neither ever returns to a finite sum.  A thread
// saw a non-finite value iff its sum is non-finite - no per-value exponent test (three VALU operations per value beside the two
// fp64 ones) is needed.
__global__ __launch_bounds__(kNormThreads) void finite_norm_kernel(const float4* __restrict__ g4, const float* __restrict__ g, size_t n4,
                                                                   size_t n, int* __restrict__ flag, double* __restrict__ partials) {
    __shared__ double wave_sums[kNormThreads / kWave];
    double acc = 0.0;
    // A trip of a workgroup is one contiguous run of kNormSpan quads (16 KB): a lane's four 16-byte loads in flight lie 4 KB apart, and
    // all workgroups together sweep one contiguous window of the arena per trip (loads a whole grid stride apart - 8 MiB, a power of
    // two - would meet in the same memory channels).
    const size_t stride = (size_t)gridDim.x * kNormSpan;
    size_t base = (size_t)blockIdx.x * kNormSpan;
    for (; base + kNormSpan <= n4; base += stride) {
        const float4* q = g4 + base + threadIdx.x;
        const float4 v0 = q[0], v1 = q[kNormThreads], v2 = q[2 * kNormThreads], v3 = q[3 * kNormThreads];
        acc = quad_sq(quad_sq(quad_sq(quad_sq(acc, v0), v1), v2), v3);
    }
    for (size_t i = base + threadIdx.x; i < n4 && i < base + kNormSpan; i += kNormThreads) acc = quad_sq(acc, g4[i]);  // a last, partial run
    if (blockIdx.x == 0) {  // the ragged end: at most three values, after the thread's quads
        for (size_t j = n4 * 4 + threadIdx.x; j < n; j += kNormThreads) acc = add_sq(acc, g[j]);
    }
    const bool bad = ((unsigned)__double2hiint(acc) & 0x7ff00000u) == 0x7ff00000u;
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_sums[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sums[0];
#pragma unroll
        for (int w = 1; w < kNormThreads / kWave; ++w) s += wave_sums[w];
        partials[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kWave) void grad_clip_resolve_kernel(const int* __restrict__ overflow_flag, const double* __restrict__ partials,
                                                                  int n_partials, double mean_scale, double loss_scale,
                                                                  double static_loss_scale, double clip_norm,
                                                                  mp_grad_clip_state* __restrict__ cs, mp_grad_clip_resolved* __restrict__ out) {
    const double sum_sq = clip_sum_partials(partials, n_partials);
    if (threadIdx.x != 0) return;
    const int flag = overflow_flag != nullptr ? *overflow_flag : 0;
    ClipDecision d = clip_decide(sum_sq, mean_scale / loss_scale / static_loss_scale, clip_norm);
    if (flag != 0) {
        d.coef = 1.0;  // the step is skipped: nothing is used or recorded
    } else {
        clip_record(cs, d);
    }
    out->flag = flag;
    out->pad = 0;
    out->norm = d.norm;
    out->coef = d.coef;
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

int mp_grad_norm_partials(size_t count) {
    if (count == 0) return 0;
    size_t blocks = (count / 4 + kNormSpan - 1) / kNormSpan;
    if (blocks > (size_t)kNormBlocksCap) blocks = kNormBlocksCap;
    if (blocks == 0) blocks = 1;
    return (int)blocks;
}

int mp_grad_finite_norm(const float* grad, size_t count, int* flag, double* partials, mp_stream_t stream) {
    if (!grad || !flag || !partials) return MP_ERR_NULL;
    if (count == 0) return MP_OK;
    if ((reinterpret_cast<uintptr_t>(grad) & 15) != 0 || (reinterpret_cast<uintptr_t>(partials) & 7) != 0) return MP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(finite_norm_kernel, dim3((unsigned)mp_grad_norm_partials(count)), dim3(kNormThreads), 0, as_stream(stream),
                       reinterpret_cast<const float4*>(grad), grad, count / 4, count, flag, partials);
    return check_launch();
}

int mp_grad_clip_resolve(const int* overflow_flag, const double* partials, int n_partials, double mean_scale, double loss_scale,
                         double static_loss_scale, double clip_norm, mp_grad_clip_state* clip_state, mp_grad_clip_resolved* resolved,
                         mp_stream_t stream) {
    if (!clip_state || !resolved || (!partials && n_partials != 0)) return MP_ERR_NULL;
    if (n_partials < 0 || n_partials > kNormBlocksCap || !(clip_norm > 0.0)) return MP_ERR_SHAPE;
    hipLaunchKernelGGL(grad_clip_resolve_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), overflow_flag, partials, n_partials, mean_scale,
                       loss_scale, static_loss_scale, clip_norm, clip_state, resolved);
    return check_launch();
}

}  // extern "C"
