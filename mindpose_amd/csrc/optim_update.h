// The per-element update rules of the arena optimizers, each stated once: step_update_kernel of step_end.hip runs these bodies, with
// lr / gradient scale / skip from the host or from the device's step-arguments block.
#pragma once
#include "common.h"

namespace mp {

// mindspore.nn.AdamWeightDecay: Adam WITHOUT bias correction, decoupled weight decay, eps added to sqrt(v)
// (mindpose/optim/optim_factory.py:69-72 selects it for "adamw").  gi = the gradient as the update sees it.
__device__ __forceinline__ void adamw_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, size_t i, float gi,
                                             float lr, float b1, float b2, float eps, float wd) {
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float upd = mi / (sqrtf(vi) + eps);
    upd += wd * p[i];
    p[i] = p[i] - lr * upd;
}

// The other optimizers the reference registers (mindpose/optim/optim_factory.py:9-14), same flat-arena form.  Update rules as
// documented for mindspore.nn.{Adam, SGD, Momentum, Adagrad} [MS-knowledge: no reference test pins them]; the gradient is
// first divided by the static loss scale and given the L2 term (g = g * grad_scale + wd * p), as those optimizers do.
//   kind 1 Adam:     m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
//        (h: b1, b2, eps, b1^t, b2^t)
//   kind 2 SGD:      buf = g on the first step, else mom buf + (1-damp) g; d = nesterov ? g + mom buf : buf (d = g when
//        mom == 0); p -= lr d      (h: mom, damp, nesterov, first_step)
//   kind 3 Momentum: acc = mom acc + g; p -= lr (nesterov ? g + mom acc : acc)      (h: mom, nesterov)
//   kind 4 Adagrad:  acc += g^2; p -= lr g / sqrt(acc)      (accumulator initialised by the caller, 0.1 in MindSpore)
// graw = the arena's gradient value.
template <int KIND>
__device__ __forceinline__ void optimizer_update(float* __restrict__ p, float* __restrict__ s1, float* __restrict__ s2, size_t i,
                                                 float graw, float lr, float grad_scale, float wd, float h0, float h1, float h2,
                                                 float h3, float h4) {
    const float w = p[i];
    const float gi = graw * grad_scale + wd * w;
    if (KIND == 1) {
        const float mi = h0 * s1[i] + (1.f - h0) * gi;
        const float vi = h1 * s2[i] + (1.f - h1) * gi * gi;
        s1[i] = mi;
        s2[i] = vi;
        const float lr_t = lr * sqrtf(1.f - h4) / (1.f - h3);
        p[i] = w - lr_t * mi / (sqrtf(vi) + h2);
    } else if (KIND == 2) {
        float d = gi;
        if (h0 != 0.f) {
            const float buf = h3 != 0.f ? gi : h0 * s1[i] + (1.f - h1) * gi;
            s1[i] = buf;
            d = h2 != 0.f ? gi + h0 * buf : buf;
        }
        p[i] = w - lr * d;
    } else if (KIND == 3) {
        const float acc = h0 * s1[i] + gi;
        s1[i] = acc;
        p[i] = w - lr * (h1 != 0.f ? gi + h0 * acc : acc);
    } else {
        const float acc = s1[i] + gi * gi;
        s1[i] = acc;
        p[i] = w - lr * gi / sqrtf(acc);
    }
}

}  // namespace mp
