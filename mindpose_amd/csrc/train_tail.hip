// Device-resident step tail: the dynamic-loss-scale state machine, the skip decision and the learning-rate lookup of a training
// step as ONE single-workgroup launch (mp_train_tail_advance), and the arena optimizers' update launches reading what it decided
// from a step-arguments block in device memory (mp_adamw_step_resident / mp_optimizer_step_resident) - the host queues step t+1
// without reading anything of step t back.
//
// Reference: tools/train.py:170-181 (DynamicLossScaleManager under amp O2) and the loop that
// mindspore.Model.train(..., dataset_sink_mode=True) runs on the device (tools/train.py:233).  The host-driven form of the same
// arithmetic is utils/loss_scale.py + utils/adamw.py; every quantity here is that integer / double arithmetic restated, or the
// same fp32 update body (optim_update.h).
#include "common.h"
#include "grad_clip.h"
#include "optim_update.h"

namespace mp {
namespace {

// The step tail of ONE thread: fills *args from the state before the update, then advances the state.  clip_coef multiplies the
// gradient scale last (1.0 without clipping: the product is then the scale itself, bit for bit).  Returns whether the step is skipped.
__device__ __forceinline__ bool tail_advance(const int* __restrict__ overflow_flag, mp_train_tail_state* __restrict__ st, double factor,
                                             long long window, double grad_scale_base, double clip_coef,
                                             const float* __restrict__ lr_table, long long lr_len, const float* __restrict__ aux_table,
                                             long long aux_len, mp_step_args* __restrict__ args, float* __restrict__ loss_scale_out) {
    const bool scaling = overflow_flag != nullptr;
    const bool overflow = scaling && *overflow_flag != 0;
    double loss_scale = st->loss_scale;  // (grad_scale_base was made from it by the caller)
    const long long cur = st->cur_iter, applied = st->applied_steps;
    // what the update launches of THIS step read
    const long long li = applied < lr_len - 1 ? applied : lr_len - 1;
    args->skip = overflow ? 1 : 0;
    args->grad_scale = (float)(grad_scale_base * clip_coef);
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
    return overflow;
}

__global__ __launch_bounds__(64) void train_tail_advance_kernel(const int* __restrict__ overflow_flag, mp_train_tail_state* __restrict__ st,
                                                                double factor, long long window, double mean_scale,
                                                                double static_loss_scale, const float* __restrict__ lr_table,
                                                                long long lr_len, const float* __restrict__ aux_table, long long aux_len,
                                                                mp_step_args* __restrict__ args, float* __restrict__ loss_scale_out) {
    if (threadIdx.x != 0) return;
    tail_advance(overflow_flag, st, factor, window, mean_scale / st->loss_scale / static_loss_scale, 1.0, lr_table, lr_len, aux_table,
                 aux_len, args, loss_scale_out);
}

// The same with gradient clipping by global norm (grad_clip.h): the 64 lanes sum the partials of mp_grad_finite_norm, lane 0 decides
// the coefficient and records the norm of a step that is not skipped.
__global__ __launch_bounds__(64) void train_tail_advance_clip_kernel(const int* __restrict__ overflow_flag,
                                                                     mp_train_tail_state* __restrict__ st, double factor, long long window,
                                                                     double mean_scale, double static_loss_scale,
                                                                     const float* __restrict__ lr_table, long long lr_len,
                                                                     const float* __restrict__ aux_table, long long aux_len,
                                                                     mp_step_args* __restrict__ args, float* __restrict__ loss_scale_out,
                                                                     const double* __restrict__ partials, int n_partials, double clip_norm,
                                                                     mp_grad_clip_state* __restrict__ cs) {
    const double sum_sq = clip_sum_partials(partials, n_partials);
    if (threadIdx.x != 0) return;
    const double base = mean_scale / st->loss_scale / static_loss_scale;
    const ClipDecision d = clip_decide(sum_sq, base, clip_norm);
    const bool skipped = tail_advance(overflow_flag, st, factor, window, base, d.coef, lr_table, lr_len, aux_table, aux_len, args,
                                      loss_scale_out);
    if (!skipped) clip_record(cs, d);
}

__global__ __launch_bounds__(256) void adamw_resident_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, size_t n, float b1, float b2, float eps, float wd,
                                                             const mp_step_args* __restrict__ args) {
    if (args->skip != 0) return;  // overflow step: parameters and moments untouched (uniform over the grid)
    const float lr = args->lr, grad_scale = args->grad_scale;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        adamw_update(p, m, v, i, g[i] * grad_scale, lr, b1, b2, eps, wd);
}

// kinds 1 ... 4 of optimizer_update; Adam's beta^t (h3, h4) and SGD's first_step (h3) come from the block, the rest from the launch
template <int KIND>
__global__ __launch_bounds__(256) void optimizer_resident_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                                 float* __restrict__ s2, size_t n, float wd, float h0, float h1, float h2,
                                                                 float h3, float h4, const mp_step_args* __restrict__ args) {
    if (args->skip != 0) return;
    const float lr = args->lr, grad_scale = args->grad_scale;
    if (KIND == 1) {
        h3 = args->aux0;
        h4 = args->aux1;
    } else if (KIND == 2) {
        h3 = args->first_step;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        optimizer_update<KIND>(p, s1, s2, i, g[i], lr, grad_scale, wd, h0, h1, h2, h3, h4);
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

int mp_train_tail_advance(const int* overflow_flag, mp_train_tail_state* state, double scale_factor, int64_t scale_window,
                          double mean_scale, double static_loss_scale, const float* lr_table, int64_t lr_len, const float* aux_table,
                          int64_t aux_len, mp_step_args* step_args, float* loss_scale_out, mp_stream_t stream) {
    if (!state || !lr_table || !step_args) return MP_ERR_NULL;
    if (lr_len < 1 || (aux_table && aux_len < 1)) return MP_ERR_SHAPE;
    if (overflow_flag && scale_window < 1) return MP_ERR_SHAPE;
    hipLaunchKernelGGL(train_tail_advance_kernel, dim3(1), dim3(64), 0, as_stream(stream), overflow_flag, state, scale_factor,
                       (long long)scale_window, mean_scale, static_loss_scale, lr_table, (long long)lr_len, aux_table, (long long)aux_len,
                       step_args, loss_scale_out);
    return check_launch();
}

int mp_train_tail_advance_clip(const int* overflow_flag, mp_train_tail_state* state, double scale_factor, int64_t scale_window,
                               double mean_scale, double static_loss_scale, const float* lr_table, int64_t lr_len, const float* aux_table,
                               int64_t aux_len, mp_step_args* step_args, float* loss_scale_out, const double* partials, int n_partials,
                               double clip_norm, mp_grad_clip_state* clip_state, mp_stream_t stream) {
    if (!state || !lr_table || !step_args || !clip_state || (!partials && n_partials != 0)) return MP_ERR_NULL;
    if (lr_len < 1 || (aux_table && aux_len < 1)) return MP_ERR_SHAPE;
    if (overflow_flag && scale_window < 1) return MP_ERR_SHAPE;
    if (n_partials < 0 || n_partials > kNormBlocksCap || !(clip_norm > 0.0)) return MP_ERR_SHAPE;
    hipLaunchKernelGGL(train_tail_advance_clip_kernel, dim3(1), dim3(64), 0, as_stream(stream), overflow_flag, state, scale_factor,
                       (long long)scale_window, mean_scale, static_loss_scale, lr_table, (long long)lr_len, aux_table, (long long)aux_len,
                       step_args, loss_scale_out, partials, n_partials, clip_norm, clip_state);
    return check_launch();
}

int mp_adamw_step_resident(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t count, float beta1, float beta2,
                           float eps, float weight_decay, const mp_step_args* step_args, mp_stream_t stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_args) return MP_ERR_NULL;
    if (count == 0) return MP_OK;
    size_t blocks = (count + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(adamw_resident_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), param, grad, exp_avg, exp_avg_sq,
                       count, beta1, beta2, eps, weight_decay, step_args);
    return check_launch();
}

int mp_optimizer_step_resident(int kind, float* param, const float* grad, float* state1, float* state2, size_t count,
                               float weight_decay, const float hyper[5], const mp_step_args* step_args, mp_stream_t stream) {
    if (!param || !grad || !hyper || !step_args) return MP_ERR_NULL;
    if (kind < 1 || kind > 4) return MP_ERR_UNSUPPORTED;
    if (!state1 && !(kind == 2 && hyper[0] == 0.f)) return MP_ERR_NULL;
    if (kind == 1 && !state2) return MP_ERR_NULL;
    if (count == 0) return MP_OK;
    size_t blocks = (count + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = as_stream(stream);
    const float h0 = hyper[0], h1 = hyper[1], h2 = hyper[2], h3 = hyper[3], h4 = hyper[4];
    switch (kind) {
        case 1: hipLaunchKernelGGL(optimizer_resident_kernel<1>, grid, block, 0, s, param, grad, state1, state2, count, weight_decay, h0, h1, h2, h3, h4, step_args); break;
        case 2: hipLaunchKernelGGL(optimizer_resident_kernel<2>, grid, block, 0, s, param, grad, state1, state2, count, weight_decay, h0, h1, h2, h3, h4, step_args); break;
        case 3: hipLaunchKernelGGL(optimizer_resident_kernel<3>, grid, block, 0, s, param, grad, state1, state2, count, weight_decay, h0, h1, h2, h3, h4, step_args); break;
        default: hipLaunchKernelGGL(optimizer_resident_kernel<4>, grid, block, 0, s, param, grad, state1, state2, count, weight_decay, h0, h1, h2, h3, h4, step_args); break;
    }
    return check_launch();
}

}  // extern "C"
