// The step end: everything that runs after the backward pass has filled the flat fp32 gradient arena - the overflow check, the sum
// of squares for the global gradient norm, the loss-scale / skip / clip / learning-rate decision, and the parameter update.
//   checks     mp_grad_finite_check (flag only) and mp_grad_finite_norm (flag + partial sums of squares), each ONE read of the arena
//   decision   mp_train_tail_advance[_clip]: the dynamic-loss-scale state machine, the skip decision, the learning-rate lookup and the
//              clip coefficient as ONE single-workgroup launch that fills a step-arguments block in device memory - the host queues
//              step t+1 without reading anything of step t back; mp_grad_clip_resolve: norm and coefficient for a host-driven step
//   update     one streaming kernel over the arena per optimizer rule (optim_update.h), its step-dependent arguments either by value
//              from the host (mp_adamw_step, mp_adamw_step_scaled, mp_optimizer_step) or from the step-arguments block
//              (mp_adamw_step_resident, mp_optimizer_step_resident)
// Nothing here scales a gradient in memory: 1 / loss scale, 1 / world and the clip coefficient are factors of the gradient scale the
// update kernels apply while reading the arena.
//
// Reference: tools/train.py:170-181 (DynamicLossScaleManager under amp O2: overflow check, skip + halve) and the loop that
// mindspore.Model.train(..., dataset_sink_mode=True) runs on the device (tools/train.py:233); optim/optim_factory.py:9-14, 69-72 (the
// optimizers).  The host-driven form of the same arithmetic is utils/loss_scale.py + utils/adamw.py; every quantity here is that
// integer / double arithmetic restated.  The reference trains without clipping; the definition is
// mindspore.ops.clip_by_global_norm's (clip_norm / norm when norm > clip_norm, no epsilon), the `clip_grad` / `clip_value` keys are
// those of the sibling mindcv recipes (include/mindpose_hip.h, "gradient clipping by global norm").
#include "common.h"
#include "optim_update.h"

namespace mp {
namespace {

// ---- overflow check: one read of the arena, flag |= any(!isfinite) ----------------------------------------------------------
__global__ __launch_bounds__(256) void finite_check_kernel(const float4* __restrict__ g4, const float* __restrict__ g, size_t n4,
                                                           size_t n, int* __restrict__ flag) {
    // a value is non-finite iff its exponent field is all ones
    unsigned bad = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = g4[i];
        const unsigned e = 0x7f800000u;
        bad |= (unsigned)((__float_as_uint(v.x) & e) == e) | (unsigned)((__float_as_uint(v.y) & e) == e) |
               (unsigned)((__float_as_uint(v.z) & e) == e) | (unsigned)((__float_as_uint(v.w) & e) == e);
    }
    if (blockIdx.x == 0) {
        for (size_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) bad |= (unsigned)((__float_as_uint(g[i]) & 0x7f800000u) == 0x7f800000u);
    }
    if (__ballot(bad != 0) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// ---- the same read with the sum of squares riding on it (gradient clipping by global norm) -----------------------------------
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

// ---- the clip decision: the device code both launches that decide a coefficient share (the step tail with clipping, the host-driven
// step's resolve launch), so S, norm and coef are stated once and the two step paths are bit-equal -------------------------------

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

// ---- the device-resident step tail --------------------------------------------------------------------------------------------
// One wave: fills *args from the state before the update, then advances the state.  CLIP: the 64 lanes sum the partials of
// mp_grad_finite_norm, lane 0 decides the coefficient and records the norm of a step that is not skipped; without it no partial is
// read, the coefficient is exactly 1.0 (the gradient scale is then the base itself, bit for bit) and nothing is recorded - the
// instantiation carries none of that code.  The coefficient multiplies the gradient scale last.
template <bool CLIP>
__global__ __launch_bounds__(kWave) void train_tail_advance_kernel(const int* __restrict__ overflow_flag, mp_train_tail_state* __restrict__ st,
                                                                   double factor, long long window, double mean_scale,
                                                                   double static_loss_scale, const float* __restrict__ lr_table,
                                                                   long long lr_len, const float* __restrict__ aux_table, long long aux_len,
                                                                   mp_step_args* __restrict__ args, float* __restrict__ loss_scale_out,
                                                                   const double* __restrict__ partials, int n_partials, double clip_norm,
                                                                   mp_grad_clip_state* __restrict__ cs) {
    const double sum_sq = CLIP ? clip_sum_partials(partials, n_partials) : 0.0;
    if (threadIdx.x != 0) return;
    const bool scaling = overflow_flag != nullptr;
    const bool overflow = scaling && *overflow_flag != 0;
    double loss_scale = st->loss_scale;
    const double base = mean_scale / loss_scale / static_loss_scale;
    ClipDecision d = {0.0, 1.0, false};
    if (CLIP) d = clip_decide(sum_sq, base, clip_norm);
    const long long cur = st->cur_iter, applied = st->applied_steps;
    // what the update launches of THIS step read
    const long long li = applied < lr_len - 1 ? applied : lr_len - 1;
    args->skip = overflow ? 1 : 0;
    args->grad_scale = (float)(base * d.coef);
    args->lr = lr_table[li];
    float aux0 = 0.f, aux1 = 0.f;
    if (aux_table != nullptr) {
        const long long ai = applied < aux_len - 1 ? applied : aux_len - 1;
        aux0 = aux_table[2 * ai];
        aux1 = aux_table[2 * ai + 1];
    }
    args->aux0 = aux0;
    args->aux1 = aux1;
    args->first_step = applied == 0 ? 1.f : 0.f;
    // DynamicLossScaleManager.update_loss_scale
    if (overflow) {
        const double halved = loss_scale / factor;
        loss_scale = halved > 1.0 ? halved : 1.0;
        st->last_overflow_iter = cur;
        st->skipped_steps += 1;
    } else {
        if (scaling && (cur - st->last_overflow_iter) % window == 0) loss_scale *= factor;
        st->applied_steps = applied + 1;
    }
    st->loss_scale = loss_scale;
    st->cur_iter = cur + 1;
    if (loss_scale_out != nullptr) *loss_scale_out = (float)loss_scale;  // the next replay multiplies the loss by it
    if (CLIP && !overflow) clip_record(cs, d);
}

// ---- the update: one streaming loop, parameterised on the rule and on where the step-dependent arguments come from ---------------
// An argument source supplies lr, the gradient scale, whether the step is skipped (uniform over the grid) and - for the rules whose
// hyper-parameters depend on the step - what replaces h3 / h4 of the launch.
struct HostStepArgs {  // by value, from the host
    float lr_, grad_scale_;
    const int* skip_;  // device flag of the overflow check, or NULL = never skip
    __device__ __forceinline__ float lr() const { return lr_; }
    __device__ __forceinline__ float grad_scale() const { return grad_scale_; }
    __device__ __forceinline__ bool skip() const { return skip_ != nullptr && *skip_ != 0; }
    template <int KIND>
    __device__ __forceinline__ void step_hyper(float&, float&) const {}
};

struct ResidentStepArgs {  // the block mp_train_tail_advance filled
    const mp_step_args* __restrict__ a;
    __device__ __forceinline__ float lr() const { return a->lr; }
    __device__ __forceinline__ float grad_scale() const { return a->grad_scale; }
    __device__ __forceinline__ bool skip() const { return a->skip != 0; }
    // Adam's beta^t (h3, h4) and SGD's first_step (h3) come from the block, the rest from the launch
    template <int KIND>
    __device__ __forceinline__ void step_hyper(float& h3, float& h4) const {
        if (KIND == 1) {
            h3 = a->aux0;
            h4 = a->aux1;
        } else if (KIND == 2) {
            h3 = a->first_step;
        }
    }
};

// KIND 0: mindspore.nn.AdamWeightDecay (adamw_update; h0 ... h2 = beta1, beta2, eps); kinds 1 ... 4: optimizer_update
template <int KIND, class Args>
__global__ __launch_bounds__(256) void step_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                          float* __restrict__ s2, size_t n, float wd, float h0, float h1, float h2,
                                                          float h3, float h4, Args args) {
    if (args.skip()) return;  // overflow step: parameters and state untouched
    const float lr = args.lr(), grad_scale = args.grad_scale();
    args.template step_hyper<KIND>(h3, h4);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (KIND == 0)
            adamw_update(p, s1, s2, i, g[i] * grad_scale, lr, h0, h1, h2, wd);
        else
            optimizer_update<KIND>(p, s1, s2, i, g[i], lr, grad_scale, wd, h0, h1, h2, h3, h4);
    }
}

unsigned update_grid(size_t count) {
    size_t blocks = (count + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    return (unsigned)blocks;
}

template <int KIND, class Args>
void launch_update_kind(float* param, const float* grad, float* state1, float* state2, size_t count, float wd, const float* h,
                        const Args& args, hipStream_t s) {
    hipLaunchKernelGGL((step_update_kernel<KIND, Args>), dim3(update_grid(count)), dim3(256), 0, s, param, grad, state1, state2, count, wd,
                       h[0], h[1], h[2], h[3], h[4], args);
}

// kind 0 ... 4, checked by the caller; count == 0 launches nothing
template <class Args>
int launch_update(int kind, float* param, const float* grad, float* state1, float* state2, size_t count, float wd, const float* h,
                  const Args& args, mp_stream_t stream) {
    if (count == 0) return MP_OK;
    hipStream_t s = as_stream(stream);
    switch (kind) {
        case 0: launch_update_kind<0>(param, grad, state1, state2, count, wd, h, args, s); break;
        case 1: launch_update_kind<1>(param, grad, state1, state2, count, wd, h, args, s); break;
        case 2: launch_update_kind<2>(param, grad, state1, state2, count, wd, h, args, s); break;
        case 3: launch_update_kind<3>(param, grad, state1, state2, count, wd, h, args, s); break;
        default: launch_update_kind<4>(param, grad, state1, state2, count, wd, h, args, s); break;
    }
    return check_launch();
}

int check_optimizer_args(int kind, const float* param, const float* grad, const float* state1, const float* state2, const float* hyper) {
    if (!param || !grad || !hyper) return MP_ERR_NULL;
    if (kind < 1 || kind > 4) return MP_ERR_UNSUPPORTED;
    if (!state1 && !(kind == 2 && hyper[0] == 0.f)) return MP_ERR_NULL;
    if (kind == 1 && !state2) return MP_ERR_NULL;
    return MP_OK;
}

// Both entries of the step tail: `clip` says whether the caller brought a clip state (then it and the partials are checked too).
int launch_tail(const int* overflow_flag, mp_train_tail_state* state, double scale_factor, int64_t scale_window, double mean_scale,
                double static_loss_scale, const float* lr_table, int64_t lr_len, const float* aux_table, int64_t aux_len,
                mp_step_args* step_args, float* loss_scale_out, bool clip, const double* partials, int n_partials, double clip_norm,
                mp_grad_clip_state* clip_state, mp_stream_t stream) {
    if (!state || !lr_table || !step_args || (clip && (!clip_state || (!partials && n_partials != 0)))) return MP_ERR_NULL;
    if (lr_len < 1 || (aux_table && aux_len < 1)) return MP_ERR_SHAPE;
    if (overflow_flag && scale_window < 1) return MP_ERR_SHAPE;
    if (clip && (n_partials < 0 || n_partials > kNormBlocksCap || !(clip_norm > 0.0))) return MP_ERR_SHAPE;
    hipLaunchKernelGGL(clip ? train_tail_advance_kernel<true> : train_tail_advance_kernel<false>, dim3(1), dim3(kWave), 0,
                       as_stream(stream), overflow_flag, state, scale_factor, (long long)scale_window, mean_scale, static_loss_scale, lr_table, (long long)lr_len, aux_table, (long long)aux_len,
                       step_args, loss_scale_out, partials, n_partials, clip_norm, clip_state);
    return check_launch();
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

int mp_grad_finite_check(const float* grad, size_t count, int* flag, mp_stream_t stream) {
    if (!grad || !flag) return MP_ERR_NULL;
    if (count == 0) return MP_OK;
    if ((reinterpret_cast<uintptr_t>(grad) & 15) != 0) return MP_ERR_UNSUPPORTED;  // arena slices are 16-byte aligned by the caller
    const size_t n4 = count / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(finite_check_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const float4*>(grad), grad, n4, count, flag);
    return check_launch();
}

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

int mp_train_tail_advance(const int* overflow_flag, mp_train_tail_state* state, double scale_factor, int64_t scale_window,
                          double mean_scale, double static_loss_scale, const float* lr_table, int64_t lr_len, const float* aux_table,
                          int64_t aux_len, mp_step_args* step_args, float* loss_scale_out, mp_stream_t stream) {
    return launch_tail(overflow_flag, state, scale_factor, scale_window, mean_scale, static_loss_scale, lr_table, lr_len, aux_table, aux_len,
                       step_args, loss_scale_out, false, nullptr, 0, 1.0, nullptr, stream);
}

int mp_train_tail_advance_clip(const int* overflow_flag, mp_train_tail_state* state, double scale_factor, int64_t scale_window,
                               double mean_scale, double static_loss_scale, const float* lr_table, int64_t lr_len, const float* aux_table,
                               int64_t aux_len, mp_step_args* step_args, float* loss_scale_out, const double* partials, int n_partials,
                               double clip_norm, mp_grad_clip_state* clip_state, mp_stream_t stream) {
    return launch_tail(overflow_flag, state, scale_factor, scale_window, mean_scale, static_loss_scale, lr_table, lr_len, aux_table, aux_len,
                       step_args, loss_scale_out, true, partials, n_partials, clip_norm, clip_state, stream);
}

// AdamWeightDecay with the gradient scale folded in (1 / (loss_scale * world)) and a device-side skip flag
int mp_adamw_step_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t count, float lr, float beta1,
                         float beta2, float eps, float weight_decay, float grad_scale, const int* skip_flag, mp_stream_t stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) return MP_ERR_NULL;
    const float h[5] = {beta1, beta2, eps, 0.f, 0.f};
    return launch_update(0, param, grad, exp_avg, exp_avg_sq, count, weight_decay, h, HostStepArgs{lr, grad_scale, skip_flag}, stream);
}

// the scaled form with scale 1 (g * 1.0f is g, bit for bit) and no skip flag
int mp_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t count, float lr, float beta1,
                  float beta2, float eps, float weight_decay, mp_stream_t stream) {
    return mp_adamw_step_scaled(param, grad, exp_avg, exp_avg_sq, count, lr, beta1, beta2, eps, weight_decay, 1.0f, nullptr, stream);
}

int mp_adamw_step_resident(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t count, float beta1, float beta2,
                           float eps, float weight_decay, const mp_step_args* step_args, mp_stream_t stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_args) return MP_ERR_NULL;
    const float h[5] = {beta1, beta2, eps, 0.f, 0.f};
    return launch_update(0, param, grad, exp_avg, exp_avg_sq, count, weight_decay, h, ResidentStepArgs{step_args}, stream);
}

int mp_optimizer_step(int kind, float* param, const float* grad, float* state1, float* state2, size_t count, float lr,
                      float grad_scale, float weight_decay, const float hyper[5], mp_stream_t stream) {
    if (int rc = check_optimizer_args(kind, param, grad, state1, state2, hyper)) return rc;
    return launch_update(kind, param, grad, state1, state2, count, weight_decay, hyper, HostStepArgs{lr, grad_scale, nullptr}, stream);
}

int mp_optimizer_step_resident(int kind, float* param, const float* grad, float* state1, float* state2, size_t count,
                               float weight_decay, const float hyper[5], const mp_step_args* step_args, mp_stream_t stream) {
    if (!step_args) return MP_ERR_NULL;
    if (int rc = check_optimizer_args(kind, param, grad, state1, state2, hyper)) return rc;
    return launch_update(kind, param, grad, state1, state2, count, weight_decay, hyper, ResidentStepArgs{step_args}, stream);
}

}  // extern "C"
