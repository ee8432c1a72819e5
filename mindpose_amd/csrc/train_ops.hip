// Training-side HBM-bound kernels (gfx950): BatchNorm2d in training mode (batch statistics, forward and
// backward) and the backward of the exchange-unit sum (the optimizer updates are in step_end.hip).  All reductions are
// two-stage with a fixed partition and a fixed combine order, so results are bit-reproducible run to run.
#include "common.h"

#include <math.h>
#include <stdlib.h>

#include <mutex>
#include <unordered_map>

namespace mp {

constexpr int kBnSplit = 32;  // per-channel partial reductions (fixed: determinism)
constexpr int kBn16MaxSplit = 256;

__device__ __forceinline__ double block_sum_256(double v, double* sm) {
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// ---- the pieces every BatchNorm form shares: each formula, and each per-channel publication, is written here once -------------------
// one lane of one element
__device__ __forceinline__ float bn_xhat(float z, float mu, float is) { return (z - mu) * is; }
// dz = gamma*invstd * (g - dbeta/M - xhat*dgamma/M):  k = gamma * invstd, mb = dbeta / M, mg = dgamma / M
__device__ __forceinline__ float bn_dz(float k, float g, float mb, float xh, float mg) { return k * (g - mb - xh * mg); }

// Batch statistics of a channel from its fp64 sums, the fp64 divide / sqrt flavour (the fp32 kernels and the reducing fp16 forms; the
// apply-only forms have their own, bn16_fwd_coeffs, which rounds differently - the tests that compare forms allow for exactly that).
// mindspore.nn.BatchNorm2d(momentum=0.9): moving = 0.9 * moving + 0.1 * batch; the moving variance takes the UNBIASED batch
// variance (cuDNN / PyTorch convention) [MS-knowledge, unverifiable here - affects only the moving statistics, never the
// training-mode output or any gradient].
struct BnStats {
    double mean, var, count;
    float invstd;
    __device__ __forceinline__ float var_unbiased() const { return (float)(count > 1.0 ? var * count / (count - 1.0) : var); }
};
__device__ __forceinline__ BnStats bn_stats(double s0, double s1, double count, float eps) {
    BnStats o;
    o.count = count;
    o.mean = s0 / count;
    o.var = s1 / count - o.mean * o.mean;
    if (o.var < 0.0) o.var = 0.0;
    o.invstd = (float)(1.0 / sqrt(o.var + (double)eps));
    return o;
}

// what a direction leaves per channel.  The apply-only argument records carry these; the reducing kernels build them from their own
// __restrict__ parameters (as struct members the pointers lose it, and bn16_coop_kernel<false> an occupancy step with it).
// The *_acc pair is both or neither (bn_grad_out).
struct BnStatOut { float *save_mean, *save_invstd, *moving_mean, *moving_var; float momentum; };
struct BnGradOut { float *dgamma, *dbeta, *dgamma_acc, *dbeta_acc; };
// per-channel inputs (mean / invstd: backward only; beta in the backward: only where the ReLU mask is re-derived from z)
struct BnChannels { const float *gamma, *beta, *mean, *invstd; };

// saved statistics + moving averages of channel ch; the moving variance takes the unbiased variance ALREADY rounded to fp32
__device__ __forceinline__ void bn_fwd_publish(int ch, float mean, float invstd, float var_unbiased, const BnStatOut& o) {
    o.save_mean[ch] = mean;
    o.save_invstd[ch] = invstd;
    if (o.moving_mean) {
        o.moving_mean[ch] = o.momentum * o.moving_mean[ch] + (1.f - o.momentum) * mean;
        o.moving_var[ch] = o.momentum * o.moving_var[ch] + (1.f - o.momentum) * var_unbiased;
    }
}
// dbeta / dgamma of channel ch, + straight into the caller's gradient buffers (no separate add launch)
__device__ __forceinline__ void bn_bwd_publish(int ch, float db, float dg, const BnGradOut& o) {
    o.dbeta[ch] = db;
    o.dgamma[ch] = dg;
    if (o.dgamma_acc) {
        o.dbeta_acc[ch] += db;
        o.dgamma_acc[ch] += dg;
    }
}

// stage 1: grid (C, kBnSplit); block (c, s) reduces images n = s, s + kBnSplit, ... of channel c.
// out: part[(c * kBnSplit + s) * 2 + {0,1}] = (sum a, sum a*b) in fp64, where
//   forward  a = z,            b = z            -> sum z, sum z^2
//   backward a = g (masked dy), b = xhat         -> sum g, sum g*xhat
template <bool BWD>
__global__ __launch_bounds__(256) void bn_reduce_kernel(const float* __restrict__ a_in, const float* __restrict__ z,
                                                        const float* __restrict__ y, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, double* __restrict__ part,
                                                        int n, int c, int hw, int relu) {
    const int ch = blockIdx.x, sp = blockIdx.y;
    double s0 = 0.0, s1 = 0.0;
    const float mu = BWD ? mean[ch] : 0.f, is = BWD ? invstd[ch] : 0.f;
    // Both widths stay spelled out, here and in the two apply kernels: which product the compiler contracts into an fma (today: lane
    // x of the backward float4 body, no other) depends on the shape of the source; a shared per-element body moved that choice and
    // with it the last bit of the partial sums, so of the saved statistics of every fp32 BatchNorm.
    for (int img = sp; img < n; img += kBnSplit) {
        const size_t base = ((size_t)img * c + ch) * hw;
        float f0 = 0.f, f1 = 0.f;  // fp32 per-thread partial over <= hw/256 elements, then fp64
        if ((hw & 3) == 0) {  // planes are 16-byte multiples: float4 loads (same element-to-thread order whatever the width:
                              // thread t takes elements 4q .. 4q+3 for q = t, t + 256, ...)
            for (int q = threadIdx.x; q < (hw >> 2); q += 256) {
                const float4 zv = reinterpret_cast<const float4*>(z + base)[q];
                if (BWD) {
                    float4 g = reinterpret_cast<const float4*>(a_in + base)[q];
                    if (relu) {
                        const float4 yv = reinterpret_cast<const float4*>(y + base)[q];
                        if (!(yv.x > 0.f)) g.x = 0.f;
                        if (!(yv.y > 0.f)) g.y = 0.f;
                        if (!(yv.z > 0.f)) g.z = 0.f;
                        if (!(yv.w > 0.f)) g.w = 0.f;
                    }
                    f0 += g.x; f1 += g.x * ((zv.x - mu) * is);
                    f0 += g.y; f1 += g.y * ((zv.y - mu) * is);
                    f0 += g.z; f1 += g.z * ((zv.z - mu) * is);
                    f0 += g.w; f1 += g.w * ((zv.w - mu) * is);
                } else {
                    f0 += zv.x; f1 += zv.x * zv.x;
                    f0 += zv.y; f1 += zv.y * zv.y;
                    f0 += zv.z; f1 += zv.z * zv.z;
                    f0 += zv.w; f1 += zv.w * zv.w;
                }
            }
        } else {
            for (int i = threadIdx.x; i < hw; i += 256) {
                if (BWD) {
                    float g = a_in[base + i];
                    if (relu && !(y[base + i] > 0.f)) g = 0.f;
                    const float xh = (z[base + i] - mu) * is;
                    f0 += g;
                    f1 += g * xh;
                } else {
                    const float v = z[base + i];
                    f0 += v;
                    f1 += v * v;
                }
            }
        }
        s0 += (double)f0;
        s1 += (double)f1;
    }
    __shared__ double sm[256];
    s0 = block_sum_256(s0, sm);
    s1 = block_sum_256(s1, sm);
    if (threadIdx.x == 0) {
        part[((size_t)ch * kBnSplit + sp) * 2 + 0] = s0;
        part[((size_t)ch * kBnSplit + sp) * 2 + 1] = s1;
    }
}

// stage 2 is folded into the apply kernels below: per channel mean / biased variance -> scale/shift, saved stats, moving-average
// update (bn_stats, bn_fwd_publish), or dgamma / dbeta (bn_bwd_publish).
// totals of one channel from its kBnSplit partials: the first wave of the block, lane l = split l, fixed-order shuffle tree
__device__ __forceinline__ void bn_channel_sums(const double* __restrict__ part, int ch, double& s0, double& s1) {
    s0 = 0.0;
    s1 = 0.0;
    if (threadIdx.x < kBnSplit) {
        const double2 v = *reinterpret_cast<const double2*>(part + ((size_t)ch * kBnSplit + threadIdx.x) * 2);
        s0 = v.x;
        s1 = v.y;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        s0 += __shfl_down(s0, off, 64);
        s1 += __shfl_down(s1, off, 64);
    }
}

// y = act(z * scale[c] + shift[c] (+ res)) - block per (n, c) plane.  Stage 2 is folded in: every block reduces its channel's 32
// partials itself (same values, same order in every block); the block of image 0 also writes the saved statistics and the moving
// averages - one launch less per BatchNorm and direction.
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, const double* __restrict__ part,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                       float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                       const float* __restrict__ res, float* __restrict__ y, int c, int hw, int relu,
                                                       double count, float eps, float momentum) {
    const BnStatOut out = {save_mean, save_invstd, moving_mean, moving_var, momentum};
    const size_t plane = blockIdx.x;
    const int ch = (int)(plane % c);
    __shared__ float s_sc, s_sh;
    if (threadIdx.x < 64) {
        double s0, s1;
        bn_channel_sums(part, ch, s0, s1);
        if (threadIdx.x == 0) {
            const BnStats st = bn_stats(s0, s1, count, eps);
            const float a = gamma[ch] * st.invstd;
            s_sc = a;
            s_sh = beta[ch] - (float)st.mean * a;
            if (plane < (size_t)c) bn_fwd_publish(ch, (float)st.mean, st.invstd, st.var_unbiased(), out);  // image 0
        }
    }
    __syncthreads();
    const float sc = s_sc, sh = s_sh;
    const size_t base = plane * hw;
    if ((hw & 3) == 0) {
        for (int q = threadIdx.x; q < (hw >> 2); q += 256) {
            float4 v = reinterpret_cast<const float4*>(z + base)[q];
            v.x = v.x * sc + sh; v.y = v.y * sc + sh; v.z = v.z * sc + sh; v.w = v.w * sc + sh;
            if (res) { const float4 r = reinterpret_cast<const float4*>(res + base)[q]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
            if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            reinterpret_cast<float4*>(y + base)[q] = v;
        }
    } else {
        for (int i = threadIdx.x; i < hw; i += 256) {
            float v = z[base + i] * sc + sh;
            if (res) v += res[base + i];
            if (relu) v = fmaxf(v, 0.f);
            y[base + i] = v;
        }
    }
}

// dz = bn_dz, dres = g  (g = dy masked by the ReLU of the forward output); stage 2 folded in like the forward (the block of image 0
// writes dgamma / dbeta and adds them into the caller's gradient buffers)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                           const float* __restrict__ y, const double* __restrict__ part,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, float* __restrict__ dgamma_acc,
                                                           float* __restrict__ dbeta_acc, float* __restrict__ dz,
                                                           float* __restrict__ dres, int c, int hw, int relu, float inv_count) {
    const BnGradOut out = {dgamma, dbeta, dgamma_acc, dbeta_acc};
    const size_t plane = blockIdx.x;
    const int ch = (int)(plane % c);
    __shared__ float s_mb, s_mg;
    if (threadIdx.x < 64) {
        double s0, s1;
        bn_channel_sums(part, ch, s0, s1);
        if (threadIdx.x == 0) {
            const float db = (float)s0, dg = (float)s1;
            s_mb = db * inv_count;
            s_mg = dg * inv_count;
            if (plane < (size_t)c) bn_bwd_publish(ch, db, dg, out);  // image 0
        }
    }
    __syncthreads();
    const float mu = mean[ch], is = invstd[ch];
    const float k = gamma[ch] * is, mb = s_mb, mg = s_mg;
    const size_t base = plane * hw;
    if ((hw & 3) == 0) {
        for (int q = threadIdx.x; q < (hw >> 2); q += 256) {
            float4 g = reinterpret_cast<const float4*>(dy + base)[q];
            const float4 zv = reinterpret_cast<const float4*>(z + base)[q];
            if (relu) {
                const float4 yv = reinterpret_cast<const float4*>(y + base)[q];
                if (!(yv.x > 0.f)) g.x = 0.f;
                if (!(yv.y > 0.f)) g.y = 0.f;
                if (!(yv.z > 0.f)) g.z = 0.f;
                if (!(yv.w > 0.f)) g.w = 0.f;
            }
            float4 d;
            d.x = k * (g.x - mb - ((zv.x - mu) * is) * mg);
            d.y = k * (g.y - mb - ((zv.y - mu) * is) * mg);
            d.z = k * (g.z - mb - ((zv.z - mu) * is) * mg);
            d.w = k * (g.w - mb - ((zv.w - mu) * is) * mg);
            reinterpret_cast<float4*>(dz + base)[q] = d;
            if (dres) reinterpret_cast<float4*>(dres + base)[q] = g;
        }
    } else {
        for (int i = threadIdx.x; i < hw; i += 256) {
            float g = dy[base + i];
            if (relu && !(y[base + i] > 0.f)) g = 0.f;
            const float xh = (z[base + i] - mu) * is;
            dz[base + i] = k * (g - mb - xh * mg);
            if (dres) dres[base + i] = g;
        }
    }
}

// backward of out = act(base + sum_k up_{s_k}(t_k)):  g = dy * (out > 0);  dt_k = s_k x s_k block sums of g
__global__ __launch_bounds__(256) void fuse_sum_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ out,
                                                           float* __restrict__ dt, int planes, int h, int w, int sh, int relu) {
    // one thread per element of the LOW-resolution grid of this term (sh = log2 scale); sh == 0 covers dbase-like terms
    const int lh = h >> sh, lw = w >> sh, s = 1 << sh;
    const size_t total = (size_t)planes * lh * lw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lx = (int)(i % lw);
        const size_t r = i / lw;
        const int ly = (int)(r % lh);
        const size_t plane = r / lh;
        const size_t o = (plane * h + (size_t)ly * s) * w + (size_t)lx * s;
        float acc = 0.f;
        for (int a = 0; a < s; ++a)
            for (int b = 0; b < s; ++b) {
                float g = dy[o + (size_t)a * w + b];
                if (relu && !(out[o + (size_t)a * w + b] > 0.f)) g = 0.f;
                acc += g;
            }
        if (dt) dt[i] = acc;
    }
}

// ---- fp16 (amp O2) training: the same BatchNorm passes over channel-blocked fp16 activations [N][C8][HW][8] ------------
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// The forward output is y = half(max(fma(z, sc, sh), 0)) with sc = gamma * invstd, sh = fma(-mean, sc, beta): these two helpers are
// the ONLY place that arithmetic is written, because the backward pass of a ReLU layer WITHOUT a residual input re-derives the
// ReLU mask (y > 0) from z with them instead of reading y (relu mode 2: two tensor reads less per backward BatchNorm).
// 16-bit lanes of channel block blk that hold real channels (c8 layout: channel 8 blk + j in half j)
__device__ __forceinline__ u32x4_t bn16_channel_mask(int blk, int c) {
    u32x4_t m;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        m[w] = (blk * 8 + 2 * w < c ? 0x0000FFFFu : 0u) | (blk * 8 + 2 * w + 1 < c ? 0xFFFF0000u : 0u);
    return m;
}
__device__ __forceinline__ float bn16_shift(float beta, float mean, float sc) { return __builtin_fmaf(-mean, sc, beta); }
__device__ __forceinline__ float bn16_affine(float z, float sc, float sh) { return __builtin_fmaf(z, sc, sh); }
__device__ __forceinline__ bool bn16_relu_open(float z, float sc, float sh) { return (float)(_Float16)bn16_affine(z, sc, sh) > 0.f; }

// fixed-order block reduction of 16 doubles per thread (wave shuffles, then the four waves through LDS)
__device__ __forceinline__ void block_sum16_256(double (&v)[16], double (*sm)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        double x = v[j];
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
        v[j] = x;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) sm[wave][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < 16) v[0] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
    __syncthreads();
}

// The flat (image, pixel) element range [e0, e1) that chunk `chunk` of `chunks` owns in channel block blk of an [N][C8][HW] tensor of
// 16-byte elements: 32-bit index arithmetic, image = multiply-high division by hw (64-bit divisions per element cost more than the
// element's memory traffic).  len = ceil: trailing chunks may be empty (e0 >= e1).
struct Bn16Span {
    unsigned e0, e1, magic_hw;
    int hw;
    bool exact;  // the multiply-high division is exact on [0, n * hw)
    size_t blk_off, img_extra;
    __device__ __forceinline__ Bn16Span(int n, int hw_, int c8, int blk, unsigned chunk, unsigned chunks) : hw(hw_) {
        const unsigned per_blk = (unsigned)n * (unsigned)hw;
        const unsigned len = (per_blk + chunks - 1) / chunks;
        e0 = chunk * len;
        e1 = e0 + len < per_blk ? e0 + len : per_blk;
        magic_hw = hw > 1 ? (unsigned)(0x100000000ULL / (unsigned)hw) + 1u : 0u;
        exact = (unsigned long long)per_blk * (unsigned)hw < 0x100000000ULL;
        blk_off = (size_t)blk * hw;
        img_extra = (size_t)(c8 - 1) * hw;
    }
    __device__ __forceinline__ size_t index_of(unsigned e) const {
        const unsigned img = hw <= 1 ? e : (exact ? __umulhi(e, magic_hw) : e / (unsigned)hw);
        return (size_t)e + (size_t)img * img_extra + blk_off;
    }
};

// ---- the fp16 element formulas, over the 8 channels (lanes) of one 16-byte element -----------------------------------------------
// per-lane constants of a backward pass: xhat = (z - mu) * is; msc / msh = forward scale / shift for the re-derived ReLU mask (relu 2)
struct Bn16GradLanes { float mu[8], is[8], msc[8], msh[8]; };
struct Bn16DzLanes { float k[8], mb[8], mg[8]; };  // bn_dz's per-channel factors
template <bool BWD>
__device__ __forceinline__ Bn16GradLanes bn16_grad_lanes(int blk, int c, int relu, const BnChannels& p) {
    Bn16GradLanes L;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ch = blk * 8 + j;
        L.mu[j] = (BWD && ch < c) ? p.mean[ch] : 0.f;
        L.is[j] = (BWD && ch < c) ? p.invstd[ch] : 0.f;
        L.msc[j] = (BWD && relu == 2 && ch < c) ? p.gamma[ch] * L.is[j] : 0.f;
        L.msh[j] = (BWD && relu == 2 && ch < c) ? bn16_shift(p.beta[ch], L.mu[j], L.msc[j]) : 0.f;
    }
    return L;
}

// one element of a pass: z; in the backward also the incoming gradient, and y where the mask is read from it (relu 1).
// (No __restrict__ on bn16_load's pointers: the kernels' own parameters carry it.  With a second, nested scope here the compiler
// emitted other code for the backward kernels - bn16_coop_kernel<true> 3110 instead of 3473 instructions, fewer and later waits.)
struct Bn16Elem { h16x8 z, g, y; };
template <bool BWD>
__device__ __forceinline__ Bn16Elem bn16_load(const u32x4_t* z, const u32x4_t* dy, const u32x4_t* y, size_t i, int relu) {
    Bn16Elem e;
    e.z = __builtin_bit_cast(h16x8, z[i]);
    e.g = e.z;
    e.y = e.z;
    if (BWD) {
        e.g = __builtin_bit_cast(h16x8, dy[i]);
        if (relu == 1) e.y = __builtin_bit_cast(h16x8, y[i]);
    }
    return e;
}
// the masked gradient of lane j: relu 0 dy itself, 1 masked by the stored y, 2 by the mask re-derived from z
__device__ __forceinline__ float bn16_masked(const Bn16Elem& e, int j, int relu, const Bn16GradLanes& L) {
    float g = (float)e.g[j];
    if (relu == 1 && !((float)e.y[j] > 0.f)) g = 0.f;
    if (relu == 2 && !bn16_relu_open((float)e.z[j], L.msc[j], L.msh[j])) g = 0.f;
    return g;
}
// pass 1: f[2j] += a, f[2j + 1] += a * b with (a, b) = (z, z) forward, (masked g, xhat) backward
template <bool BWD>
__device__ __forceinline__ void bn16_accumulate(float (&f)[16], const Bn16Elem& e, int relu, const Bn16GradLanes& L) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (BWD) {
            const float g = bn16_masked(e, j, relu, L);
            const float xh = bn_xhat((float)e.z[j], L.mu[j], L.is[j]);
            f[2 * j] += g;
            f[2 * j + 1] += g * xh;
        } else {
            const float v = (float)e.z[j];
            f[2 * j] += v;
            f[2 * j + 1] += v * v;
        }
    }
}
// the fp64 tail of pass 1: the block's 16 totals; thread t < 16 returns total t = (channel t >> 1, sum t & 1)
__device__ __forceinline__ double bn16_accumulated(const float (&f)[16]) {
    double acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = (double)f[j];
    __shared__ double sm[4][16];
    block_sum16_256(acc, sm);
    return acc[0];
}
// pass 2 forward: y = act(z * sc + sh (+ res)); padding channels leave as zeros
__device__ __forceinline__ u32x4_t bn16_fwd_elem(h16x8 zv, h16x8 rv, bool has_res, int relu, int blk, int c, const float (&sc)[8],
                                                 const float (&sh)[8]) {
    h16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = 0.f;
        if (blk * 8 + j < c) {
            v = bn16_affine((float)zv[j], sc[j], sh[j]);
            if (has_res) v += (float)rv[j];
            if (relu) v = fmaxf(v, 0.f);
        }
        o[j] = (_Float16)v;
    }
    return __builtin_bit_cast(u32x4_t, o);
}
// pass 2 backward: dz = bn_dz, dres = the masked gradient; padding channels leave as zeros
__device__ __forceinline__ void bn16_bwd_elem(const Bn16Elem& e, int relu, int blk, int c, const Bn16GradLanes& L, const Bn16DzLanes& D,
                                              u32x4_t& dz, u32x4_t& dres) {
    h16x8 oz, og;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float g = 0.f, d = 0.f;
        if (blk * 8 + j < c) {
            g = bn16_masked(e, j, relu, L);
            d = bn_dz(D.k[j], g, D.mb[j], bn_xhat((float)e.z[j], L.mu[j], L.is[j]), D.mg[j]);
        }
        oz[j] = (_Float16)d;
        og[j] = (_Float16)g;
    }
    dz = __builtin_bit_cast(u32x4_t, oz);
    dres = __builtin_bit_cast(u32x4_t, og);
}

// grid (C8, kBnSplit): block (blk, sp) reduces images sp, sp + kBnSplit, ... of the 8 channels of block blk; partials in the
// fp32 kernels' layout part[(ch * kBnSplit + sp) * 2 + {0,1}] so that the finalize kernels are shared
template <bool BWD>
__global__ __launch_bounds__(256) void bn16_reduce_kernel(const u32x4_t* __restrict__ a_in, const u32x4_t* __restrict__ z,
                                                          const u32x4_t* __restrict__ y, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, double* __restrict__ part, int n,
                                                          int c, int c8, int hw, int relu, int gi, int gp) {
    // split sp = (image group sp % gi, pixel chunk sp / gi): enough blocks to fill the chip even for 4 channel blocks
    const int blk = blockIdx.x, sp = blockIdx.y, nsplit = gi * gp;
    const int ig = sp % gi, pc = sp / gi;
    const int chunk = (hw + gp - 1) / gp, p0 = pc * chunk, p1 = min(p0 + chunk, hw);
    const BnChannels chan = {gamma, beta, mean, invstd};
    const Bn16GradLanes L = bn16_grad_lanes<BWD>(blk, c, relu, chan);
    // The block's elements are {images ig, ig + gi, ...} x {pixels p0 .. p1}: walked as ONE flat index space (the small maps give a
    // block only 1-2 elements per thread and image; an image loop around a pixel loop kept a single load in flight per thread and
    // made these passes latency-bound), 32-bit index arithmetic with a multiply-high division by the chunk length.
    float f[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = 0.f;
    const unsigned len = (unsigned)(p1 > p0 ? p1 - p0 : 0);
    const unsigned nimg = ig < n ? (unsigned)((n - ig + gi - 1) / gi) : 0u;
    const unsigned cnt = len * nimg;
    const unsigned magic = len > 1 ? (unsigned)(0x100000000ULL / len) + 1u : 0u;
    const bool exact = (unsigned long long)cnt * len < 0x100000000ULL;  // multiply-high division exact on [0, cnt)
    const size_t img_stride = (size_t)c8 * hw;
#pragma unroll 4
    for (unsigned e = threadIdx.x; e < cnt; e += 256) {
        const unsigned a = len <= 1 ? e : (exact ? __umulhi(e, magic) : e / len);
        const size_t i = ((size_t)(ig + a * gi)) * img_stride + (size_t)blk * hw + p0 + (e - a * len);
        bn16_accumulate<BWD>(f, bn16_load<BWD>(z, a_in, y, i, relu), relu, L);
    }
    const double total = bn16_accumulated(f);
    if (threadIdx.x < 16) {
        const int ch = blk * 8 + (threadIdx.x >> 1);
        if (ch < c) part[((size_t)ch * nsplit + sp) * 2 + (threadIdx.x & 1)] = total;
    }
}

// Stage 2 folded into the consumers: a block of the apply kernels serves ONE 8-channel block (grid = (C8, chunks of the
// image x pixel range)) and first reduces that block's partial sums itself - thread t: channel t >> 5, splits t & 31, + 32, ...
// then a 32-lane shuffle tree; every block computes the same values in the same order (deterministic) - which removes the
// ~5 us stage-2 launch between the two passes of every BatchNorm in both directions (6 % of the amp-O2 step).  Chunk 0 of a
// channel block also writes the per-channel results (saved statistics / moving averages, or dgamma / dbeta).
__device__ __forceinline__ void bn16_channel_sums(const double* __restrict__ part, int ch, int c, int nsplit, double& s0, double& s1) {
    s0 = 0.0;
    s1 = 0.0;
    if (ch < c) {
        // fixed trip count (kBn16MaxSplit / 32): all loads issue before the first add - the same sums in the same order as a
        // `sp < nsplit` loop, without its chain of dependent L2 round trips at the head of every consumer block
        double v0[kBn16MaxSplit / 32], v1[kBn16MaxSplit / 32];
#pragma unroll
        for (int k = 0; k < kBn16MaxSplit / 32; ++k) {
            const int sp = (threadIdx.x & 31) + 32 * k;
            const bool ok = sp < nsplit;
            const double2 v = ok ? *reinterpret_cast<const double2*>(part + ((size_t)ch * nsplit + sp) * 2) : make_double2(0.0, 0.0);
            v0[k] = v.x;
            v1[k] = v.y;
        }
#pragma unroll
        for (int k = 0; k < kBn16MaxSplit / 32; ++k) {
            if ((threadIdx.x & 31) + 32 * k < nsplit) {
                s0 += v0[k];
                s1 += v1[k];
            }
        }
    }
    for (int off = 16; off >= 1; off >>= 1) {  // xor tree inside each 32-lane half: every lane ends with the total
        s0 += __shfl_xor(s0, off, 64);
        s1 += __shfl_xor(s1, off, 64);
    }
}

// y = act(z * scale[c] + shift[c] (+ res)) over c8 elements; padding channels stay zero
__global__ __launch_bounds__(256) void bn16_apply_kernel(const u32x4_t* __restrict__ z, const double* __restrict__ part,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                         float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                         const u32x4_t* __restrict__ res, u32x4_t* __restrict__ y, int n, int c,
                                                         int c8, int hw, int nsplit, double count, float eps, float momentum,
                                                         int relu) {
    const BnStatOut out = {save_mean, save_invstd, moving_mean, moving_var, momentum};
    const int blk = blockIdx.x;
    __shared__ float s_scale[8], s_shift[8];
    {
        const int j = threadIdx.x >> 5, ch = blk * 8 + j;
        double s0, s1;
        bn16_channel_sums(part, ch, c, nsplit, s0, s1);
        if ((threadIdx.x & 31) == 0) {
            float sc = 0.f, sh = 0.f;
            if (ch < c) {
                const BnStats st = bn_stats(s0, s1, count, eps);
                sc = gamma[ch] * st.invstd;
                sh = bn16_shift(beta[ch], (float)st.mean, sc);
                if (blockIdx.y == 0) bn_fwd_publish(ch, (float)st.mean, st.invstd, st.var_unbiased(), out);
            }
            s_scale[j] = sc;
            s_shift[j] = sh;
        }
    }
    __syncthreads();
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = s_scale[j]; sh[j] = s_shift[j]; }
    const Bn16Span span(n, hw, c8, blk, blockIdx.y, gridDim.y);
#pragma unroll 4
    for (unsigned e = span.e0 + threadIdx.x; e < span.e1; e += 256) {
        const size_t i = span.index_of(e);
        const h16x8 zv = __builtin_bit_cast(h16x8, z[i]);
        h16x8 rv = zv;
        if (res) rv = __builtin_bit_cast(h16x8, res[i]);
        y[i] = bn16_fwd_elem(zv, rv, res != nullptr, relu, blk, c, sc, sh);
    }
}

__global__ __launch_bounds__(256) void bn16_bwd_apply_kernel(const u32x4_t* __restrict__ dy, const u32x4_t* __restrict__ z,
                                                             const u32x4_t* __restrict__ y, const double* __restrict__ part,
                                                             const float* __restrict__ gamma, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta, float* __restrict__ dgamma_acc,
                                                             float* __restrict__ dbeta_acc, u32x4_t* __restrict__ dz,
                                                             u32x4_t* __restrict__ dres, int n, int c, int c8, int hw, int nsplit,
                                                             int relu, float inv_count, const float* __restrict__ beta) {
    const BnGradOut out = {dgamma, dbeta, dgamma_acc, dbeta_acc};
    const int blk = blockIdx.x;
    __shared__ float s_k[8], s_mu[8], s_is[8], s_mb[8], s_mg[8], s_sh[8];
    {
        const int j = threadIdx.x >> 5, ch = blk * 8 + j;
        double s0, s1;
        bn16_channel_sums(part, ch, c, nsplit, s0, s1);
        if ((threadIdx.x & 31) == 0) {
            float k = 0.f, mu = 0.f, is = 0.f, mb = 0.f, mg = 0.f;
            if (ch < c) {
                const float db = (float)s0, dg = (float)s1;
                mu = mean[ch];
                is = invstd[ch];
                k = gamma[ch] * is;
                mb = db * inv_count;
                mg = dg * inv_count;
                if (blockIdx.y == 0) bn_bwd_publish(ch, db, dg, out);
            }
            s_k[j] = k; s_mu[j] = mu; s_is[j] = is; s_mb[j] = mb; s_mg[j] = mg;
            s_sh[j] = (relu == 2 && ch < c) ? bn16_shift(beta[ch], mu, k) : 0.f;  // k = gamma * invstd = the forward scale
        }
    }
    __syncthreads();
    Bn16GradLanes L;
    Bn16DzLanes D;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        D.k[j] = L.msc[j] = s_k[j]; L.mu[j] = s_mu[j]; L.is[j] = s_is[j]; D.mb[j] = s_mb[j]; D.mg[j] = s_mg[j]; L.msh[j] = s_sh[j];
    }
    const Bn16Span span(n, hw, c8, blk, blockIdx.y, gridDim.y);
#pragma unroll 4
    for (unsigned e = span.e0 + threadIdx.x; e < span.e1; e += 256) {
        const size_t i = span.index_of(e);
        u32x4_t oz, og;
        bn16_bwd_elem(bn16_load<true>(z, dy, y, i, relu), relu, blk, c, L, D, oz, og);
        dz[i] = oz;
        if (dres) dres[i] = og;
    }
}

// ---- statistics from the conv epilogue (round 3): the apply passes alone -----------------------------------------------------------
// The conv launch that produced z (forward) or the pre-masked gradient g (backward) left per-workgroup fp32 partial sums
// pre[blk][n_parts][8 channels][2] (conv_f16_dev.h); the reduction launches above do not run at all.  A block of the apply
// kernels folds the n_parts x 64 bytes of ITS channel block itself (contiguous: coalesced 16-byte loads, fp64 sums in a fixed
// order, every block the same values), kMaxFoldParts slots at most - above that bn16_fold_kernel reduces them to one slot first.
constexpr int kMaxFoldParts = 512;
constexpr int kFoldSplit = 8;  // slot ranges of the fold launch (more than kMaxFoldParts slots)

// the tail of a slot fold: thread (q = t & 3, r = t >> 2) holds the fp64 sums a[4] of float4 q over its slot rows r, r + 64, ...;
// xor tree over the 16 slot rows of the wave (q fixed), then the four waves through LDS.  Thread t < 16 returns total t of
// {sum0, sumsq0, sum1, ...}; one barrier inside.
__device__ __forceinline__ double bn16_fold_tail(double (&a)[4], double (*sm)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        for (int off = 4; off <= 32; off <<= 1) a[i] += __shfl_xor(a[i], off, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sm[wave][lane * 4 + i] = a[i];
    }
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x < 16) total = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
    return total;
}

// totals of the 8 channels of block blk -> tot[16] = {sum0, sumsq0, sum1, ...} (fp64, LDS); ends with a barrier
__device__ __forceinline__ void bn16_fold_parts(const float* __restrict__ pre, int blk, int n_parts, double* tot, double (*sm)[16]) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(pre + (size_t)blk * n_parts * 16);
    const int q = threadIdx.x & 3, r = threadIdx.x >> 2;  // float4 q of slot r, r + 64, ...
    float4 v[kMaxFoldParts / 64];
#pragma unroll
    for (int k = 0; k < kMaxFoldParts / 64; ++k) {
        const int slot = r + 64 * k;
        v[k] = slot < n_parts ? src[(size_t)slot * 4 + q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kMaxFoldParts / 64; ++k) {
        a[0] += (double)v[k].x; a[1] += (double)v[k].y; a[2] += (double)v[k].z; a[3] += (double)v[k].w;
    }
    const double total = bn16_fold_tail(a, sm);
    if (threadIdx.x < 16) tot[threadIdx.x] = total;
    __syncthreads();
}

// n_parts > kMaxFoldParts: grid (C8, kFoldSplit), block (blk, f) folds slot range f of its channel block (fixed order) into slot f of
// `out` ([C8][kFoldSplit][16]); the consumers then fold kFoldSplit slots
__global__ __launch_bounds__(256) void bn16_fold_kernel(const float* __restrict__ pre, float* __restrict__ out, int n_parts) {
    const int blk = blockIdx.x, f = blockIdx.y;
    const int per = (n_parts + kFoldSplit - 1) / kFoldSplit, s0 = f * per, s1 = min(s0 + per, n_parts);
    const float4* __restrict__ src = reinterpret_cast<const float4*>(pre + (size_t)blk * n_parts * 16);
    const int q = threadIdx.x & 3, r = threadIdx.x >> 2;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int slot = s0 + r; slot < s1; slot += 64) {
        const float4 v = src[(size_t)slot * 4 + q];
        a[0] += (double)v.x; a[1] += (double)v.y; a[2] += (double)v.z; a[3] += (double)v.w;
    }
    __shared__ double sm[4][16];
    const double total = bn16_fold_tail(a, sm);
    // fp32 slots: a range total (|sum| < 2^24 x its mean term) keeps 24 bits - the precision the conv's slots themselves have
    if (threadIdx.x < 16) out[((size_t)blk * kFoldSplit + f) * 16 + threadIdx.x] = (float)total;
}

// One typed argument record per direction of the apply-only passes: by value to the one-layer kernels, as a table of kBnJobs to the
// grouped ones.  The host fills it in ONE place (bn16_fwd_fill / bn16_bwd_fill), which is also where an entry's arguments are checked.
struct Bn16FwdArgs {
    const u32x4_t *z, *res;
    u32x4_t* y;
    const float* pre;  // partial slots [c8][n_parts][8][2] (folded to kFoldSplit slots when there were more than a block folds)
    BnChannels chan;
    BnStatOut out;
    double inv_count, unbias;
    float eps;
    int n_parts, n, c, c8, hw, relu;
    unsigned chunks, first;  // chunks per channel block; first block of the job in a grouped grid (0xFFFFFFFF: no such job)
};
struct Bn16BwdArgs {
    const u32x4_t *g, *z, *y;  // y: the reducing forms' mask (relu 1); the apply-only passes take g pre-masked
    u32x4_t *dz, *dres;
    const float* pre;
    BnChannels chan;
    BnGradOut out;
    float inv_count;
    int n_parts, n, c, c8, hw, relu;
    unsigned chunks, first;
};

// channel j of block blk: batch mean / variance from the folded sums -> the forward scale / shift (0 / 0 on a padding channel).
// gamma_v / beta_v were requested at the top of the kernel (their latency runs under the fold's); the saved statistics and the
// moving averages are published AFTER the caller has released scale / shift to the other threads - the read-modify-write of the
// moving averages is a memory round trip nobody should wait for
struct Bn16Coeffs { float sc, sh, mean, invstd, var_unbiased; };
__device__ __forceinline__ Bn16Coeffs bn16_fwd_coeffs(int j, int blk, int c, const double* s_tot, float gamma_v, float beta_v, double inv_count,
                                                      double unbias, float eps) {
    Bn16Coeffs o = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (blk * 8 + j < c) {
        const double mean = s_tot[2 * j] * inv_count;
        double var = s_tot[2 * j + 1] * inv_count - mean * mean;
        if (var < 0.0) var = 0.0;
        // 1 / sqrt(var + eps): fp32 estimate + one Newton step in fp64 (relative error ~1e-14, no fp64 divide / sqrt sequence)
        const double x = var + (double)eps;
        double r = (double)rsqrtf((float)x);
        r = r * (1.5 - 0.5 * x * r * r);
        o.invstd = (float)r;
        o.mean = (float)mean;
        o.var_unbiased = (float)(var * unbias);
        o.sc = gamma_v * o.invstd;
        o.sh = bn16_shift(beta_v, o.mean, o.sc);
    }
    return o;
}

// The prologue of the apply pass as a launch of its own, grid (C8): the statistics of a mode-1 conv launch -> the folded scale /
// shift its CONSUMER applies on its own operand (conv_f16_wreg.hip, PRE) - same fold, same arithmetic, same saved statistics
__global__ __launch_bounds__(256) void bn16_finalize_kernel(const Bn16FwdArgs a, float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ double s_tot[16];
    __shared__ double s_sm[4][16];
    const int blk = blockIdx.x, ch = blk * 8 + (int)threadIdx.x;
    const bool coef = threadIdx.x < 8 && ch < a.c;
    const float gamma_v = coef ? a.chan.gamma[ch] : 0.f, beta_v = coef ? a.chan.beta[ch] : 0.f;
    bn16_fold_parts(a.pre, blk, a.n_parts, s_tot, s_sm);
    if (threadIdx.x < 8) {
        const Bn16Coeffs o = bn16_fwd_coeffs(threadIdx.x, blk, a.c, s_tot, gamma_v, beta_v, a.inv_count, a.unbias, a.eps);
        scale[ch] = o.sc;
        shift[ch] = o.sh;
        if (coef) bn_fwd_publish(ch, o.mean, o.invstd, o.var_unbiased, a.out);
    }
}

// The streaming loop of the apply-only passes over [span.e0, span.e1), two source tensors a and b (b only if has_b: zeros otherwise).
// Batches of kBnBatch elements per thread: all loads of a batch are issued back to back, and the NEXT batch is requested before
// this one is transformed (a loop of load / wait / transform / store per element keeps one load per tensor in flight and ran
// the large maps at ~2 TB/s).  The first batch goes out BEFORE prologue() - the statistics prologue (partial slots -> totals ->
// scale / shift: three dependent round trips) then runs under its latency - on the small maps that batch is all a thread has.
// apply(a element, b element, index) transforms and stores one element.
constexpr int kBnBatch = 4;
template <class Prologue, class Apply>
__device__ __forceinline__ void bn16_stream(const Bn16Span& span, const u32x4_t* __restrict__ a, const u32x4_t* __restrict__ b, bool has_b,
                                            Prologue prologue, Apply apply) {
    const u32x4_t zero4 = (u32x4_t){0u, 0u, 0u, 0u};
    u32x4_t ca[kBnBatch], cb[kBnBatch];
    size_t ci[kBnBatch];
    auto request = [&](unsigned base, u32x4_t (&qa)[kBnBatch], u32x4_t (&qb)[kBnBatch], size_t (&qi)[kBnBatch]) {
#pragma unroll
        for (int k = 0; k < kBnBatch; ++k) {
            const unsigned e = base + threadIdx.x + 256u * k;
            const bool ok = e < span.e1;
            qi[k] = span.index_of(ok ? e : span.e0);
            qa[k] = ok ? a[qi[k]] : zero4;
            qb[k] = (ok && has_b) ? b[qi[k]] : zero4;
        }
    };
    request(span.e0, ca, cb, ci);
    prologue();
    for (unsigned base = span.e0; base < span.e1; base += 256u * kBnBatch) {
        u32x4_t na[kBnBatch], nb[kBnBatch];
        size_t ni[kBnBatch];
        const bool more = base + 256u * kBnBatch < span.e1;  // uniform
        if (more) request(base + 256u * kBnBatch, na, nb, ni);
#pragma unroll
        for (int k = 0; k < kBnBatch; ++k)
            if (base + threadIdx.x + 256u * k < span.e1) apply(ca[k], cb[k], ci[k]);
        if (more) {
#pragma unroll
            for (int k = 0; k < kBnBatch; ++k) { ca[k] = na[k]; cb[k] = nb[k]; ci[k] = ni[k]; }
        }
    }
}

// forward apply with the statistics folded from the conv's partials: y = act(z * scale + shift (+ res))
// (a __device__ body: the one-layer kernel passes blockIdx, the grouped kernel below the block's place inside its job).
// Branch-free per element on purpose (floor_v, the keep mask, zeros for a missing residual): measured against the `ch < c` form.
__device__ __forceinline__ void bn16_apply_pre_body(const Bn16FwdArgs& a, int blk, unsigned chunk) {
    __shared__ double s_tot[16];
    __shared__ double s_sm[4][16];
    __shared__ float s_scale[8], s_shift[8];
    const Bn16Span span(a.n, a.hw, a.c8, blk, chunk, a.chunks);
    const int ch = blk * 8 + (int)threadIdx.x;
    const bool coef = threadIdx.x < 8 && ch < a.c;
    const float gamma_v = coef ? a.chan.gamma[ch] : 0.f, beta_v = coef ? a.chan.beta[ch] : 0.f;
    float sc[8], sh[8];
    const float floor_v = a.relu ? 0.f : -__builtin_inff();
    const u32x4_t keep = bn16_channel_mask(blk, a.c);  // padding channels leave as zeros whatever the operands hold there
    u32x4_t* __restrict__ y = a.y;
    bn16_stream(
        span, a.z, a.res, a.res != nullptr,
        [&] {
            bn16_fold_parts(a.pre, blk, a.n_parts, s_tot, s_sm);
            Bn16Coeffs co = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (threadIdx.x < 8) {
                co = bn16_fwd_coeffs(threadIdx.x, blk, a.c, s_tot, gamma_v, beta_v, a.inv_count, a.unbias, a.eps);
                s_scale[threadIdx.x] = co.sc;
                s_shift[threadIdx.x] = co.sh;
            }
            __syncthreads();
            if (coef && chunk == 0) bn_fwd_publish(ch, co.mean, co.invstd, co.var_unbiased, a.out);
#pragma unroll
            for (int j = 0; j < 8; ++j) { sc[j] = s_scale[j]; sh[j] = s_shift[j]; }  // 0 / 0 on the padding channels: they stay zero
        },
        [&](const u32x4_t zq, const u32x4_t rq, size_t i) {
            const h16x8 zv = __builtin_bit_cast(h16x8, zq), rv = __builtin_bit_cast(h16x8, rq);
            h16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = bn16_affine((float)zv[j], sc[j], sh[j]);
                v += (float)rv[j];  // zeros without a residual: exact
                o[j] = (_Float16)fmaxf(v, floor_v);
            }
            y[i] = __builtin_bit_cast(u32x4_t, o) & keep;
        });
}

__global__ __launch_bounds__(256) void bn16_apply_pre_kernel(const Bn16FwdArgs a) { bn16_apply_pre_body(a, (int)blockIdx.x, blockIdx.y); }

// ---- grouped apply passes: up to four BatchNorms of ONE step of parallel chains (the k-th BatchNorm of every branch of an HRModule,
// hrnet.py:202-241) as one launch.  On the 32x24 ... 8x6 maps an apply pass is ~9 - 14 us of launch, fold and tail around 1 - 3 us of
// streaming; the branches' passes are independent, so a flat grid of [job 0's blocks | job 1's | ...] runs them under the largest
// one.  The job table travels by value; a block picks its whole record with compares on constant indices (no dynamic index into the
// argument struct - that would put it in scratch).
constexpr int kBnJobs = 4;
template <class Args> struct Bn16Jobs { Args job[kBnJobs]; };
// the job of this block: the last one whose first block is not behind it
__device__ __forceinline__ int bn16_job_of_block(unsigned first1, unsigned first2, unsigned first3) {
    const unsigned b = blockIdx.x;
    return (b >= first1 ? 1 : 0) + (b >= first2 ? 1 : 0) + (b >= first3 ? 1 : 0);
}

__global__ __launch_bounds__(256) void bn16_apply_pre_grouped_kernel(const Bn16Jobs<Bn16FwdArgs> t) {
    const int j = bn16_job_of_block(t.job[1].first, t.job[2].first, t.job[3].first);
    // picked on the kernel argument itself: through a reference to the table the compiler copies the table to scratch
    const Bn16FwdArgs a = j == 0 ? t.job[0] : j == 1 ? t.job[1] : j == 2 ? t.job[2] : t.job[3];
    const unsigned local = blockIdx.x - a.first;
    bn16_apply_pre_body(a, (int)(local % (unsigned)a.c8), local / (unsigned)a.c8);
}

// backward apply on a PRE-MASKED gradient g with sum g, sum g * z folded from the data-gradient conv's partials:
// dz = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)); the residual branch's gradient is g itself (nothing to write)
__device__ __forceinline__ void bn16_bwd_apply_pre_body(const Bn16BwdArgs& a, int blk, unsigned chunk) {
    __shared__ double s_tot[16];
    __shared__ double s_sm[4][16];
    __shared__ float s_k[8], s_mu[8], s_is[8], s_mb[8], s_mg[8];
    const Bn16Span span(a.n, a.hw, a.c8, blk, chunk, a.chunks);
    // the per-channel parameters are requested first: their latency runs under the fold's (they used to be a second, dependent
    // round trip behind it)
    const int ch = blk * 8 + (int)threadIdx.x;
    const bool coef = threadIdx.x < 8 && ch < a.c;
    const float mean_v = coef ? a.chan.mean[ch] : 0.f, invstd_v = coef ? a.chan.invstd[ch] : 0.f;
    const float gamma_v = coef ? a.chan.gamma[ch] : 0.f;
    float k[8], mu[8], is[8], mb[8], mg[8];
    const u32x4_t keep = bn16_channel_mask(blk, a.c);  // padding channels leave as zeros whatever the operands hold there
    u32x4_t* __restrict__ dz = a.dz;
    bn16_stream(
        span, a.g, a.z, true,
        [&] {
            bn16_fold_parts(a.pre, blk, a.n_parts, s_tot, s_sm);
            float db = 0.f, dg = 0.f;
            if (threadIdx.x < 8) {
                const int j = threadIdx.x;
                float k_v = 0.f, mb_v = 0.f, mg_v = 0.f;  // mean_v / invstd_v are zero on a padding channel already
                if (coef) {
                    // the conv epilogue summed g and g * z (raw z): sum g * xhat = invstd * (sum g z - mean * sum g), in fp64
                    db = (float)s_tot[2 * j];
                    dg = (float)((s_tot[2 * j + 1] - (double)mean_v * s_tot[2 * j]) * (double)invstd_v);
                    k_v = gamma_v * invstd_v;
                    mb_v = db * a.inv_count;
                    mg_v = dg * a.inv_count;
                }
                s_k[j] = k_v; s_mu[j] = mean_v; s_is[j] = invstd_v; s_mb[j] = mb_v; s_mg[j] = mg_v;
            }
            __syncthreads();
            // parameter gradients: published behind the barrier (the accumulating form reads the arena first)
            if (coef && chunk == 0) bn_bwd_publish(ch, db, dg, a.out);
#pragma unroll
            for (int j = 0; j < 8; ++j) { k[j] = s_k[j]; mu[j] = s_mu[j]; is[j] = s_is[j]; mb[j] = s_mb[j]; mg[j] = s_mg[j]; }  // zeros on padding channels
        },
        [&](const u32x4_t gq, const u32x4_t zq, size_t i) {
            const h16x8 gv = __builtin_bit_cast(h16x8, gq), zv = __builtin_bit_cast(h16x8, zq);
            h16x8 oz;
#pragma unroll
            for (int j = 0; j < 8; ++j) oz[j] = (_Float16)bn_dz(k[j], (float)gv[j], mb[j], bn_xhat((float)zv[j], mu[j], is[j]), mg[j]);
            dz[i] = __builtin_bit_cast(u32x4_t, oz) & keep;
        });
}

__global__ __launch_bounds__(256) void bn16_bwd_apply_pre_kernel(const Bn16BwdArgs a) { bn16_bwd_apply_pre_body(a, (int)blockIdx.x, blockIdx.y); }

__global__ __launch_bounds__(256) void bn16_bwd_apply_pre_grouped_kernel(const Bn16Jobs<Bn16BwdArgs> t) {
    const int j = bn16_job_of_block(t.job[1].first, t.job[2].first, t.job[3].first);
    // picked on the kernel argument itself: through a reference to the table the compiler copies the table to scratch
    const Bn16BwdArgs a = j == 0 ? t.job[0] : j == 1 ? t.job[1] : j == 2 ? t.job[2] : t.job[3];
    const unsigned local = blockIdx.x - a.first;
    bn16_bwd_apply_pre_body(a, (int)(local % (unsigned)a.c8), local / (unsigned)a.c8);
}

// ---- small maps: both passes of a BatchNorm direction in ONE launch --------------------------------------------------------------
// On the 32x24 / 16x12 / 8x6 maps (<= 12 MB per tensor at N = 128) the two dependent launches above cost 13 - 20 us whatever they
// move: the second pass waits for a kernel boundary.  Here a grid of <= 128 workgroups does pass 1 over its slice, publishes its
// partial sums, meets the other workgroups at a grid barrier (a counter slot owned by the library, one per stream, release /
// acquire at agent scope) and does pass 2 over the SAME slice, which its XCD's L2 still holds.
//
// Forward progress: a grid barrier needs every workgroup resident.  128 workgroups x 256 threads x <= 96 VGPRs x 1.2 KB LDS is a
// small fraction of the chip (6 such workgroups fit on ONE CU), so even with a cooperative kernel on each of the step's five streams
// all of them are resident together; other kernels in the way finish on their own.  The wait is bounded anyway (~0.5 s): on expiry
// the workgroup poisons its outputs with NaN - the step's overflow check then skips the update - instead of hanging the GPU.
// Same fixed partition and combine order every launch: bit-reproducible.
constexpr int kCoopMaxGrid = 128;

// slot = {arrival count, generation}, 64 bytes apart; launches on one slot are serialised by their stream.  The last arriver
// resets the count and bumps the generation: correct for any grid size, no host-side reset between launches.
// Everything that crosses workgroups here (the partial sums, the two counters) is written and read with agent-scope ATOMIC
// accesses, which go to the coherence point; the barrier itself therefore needs only workgroup-scope fences.  Agent-scope
// release / acquire FENCES were measured first: they write back and invalidate the whole L2 (the conv output of the previous
// kernel is still dirty in it), which cost 10 us per barrier and evicted the slice pass 2 wants to re-read.
__device__ __forceinline__ bool grid_barrier(unsigned long long* slot, unsigned total) {
    __shared__ int s_ok;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // this wave's (atomic, write-through) partial stores have completed
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* count = slot;
        unsigned long long* generation = slot + 8;
        const unsigned long long gen = __hip_atomic_load(generation, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const unsigned long long old = __hip_atomic_fetch_add(count, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int ok = 1;
        if (old == total - 1) {
            __hip_atomic_store(count, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_fetch_add(generation, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            ok = 0;
            for (int it = 0; it < (1 << 22); ++it) {
                if (__hip_atomic_load(generation, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != gen) { ok = 1; break; }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        s_ok = ok;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return s_ok != 0;
}

// totals of this block's 8 channels from the per-split partials: thread t = (channel t >> 5, split t & 31); fixed-order xor tree
__device__ __forceinline__ void coop_channel_sums(const double* part, int ch, int c, int nsplit, double& s0, double& s1) {
    s0 = 0.0;
    s1 = 0.0;
    const int sp = threadIdx.x & 31;
    if (ch < c && sp < nsplit) {  // written by other workgroups (other XCDs): read at the coherence point
        s0 = __hip_atomic_load(part + ((size_t)ch * nsplit + sp) * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s1 = __hip_atomic_load(part + ((size_t)ch * nsplit + sp) * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int off = 16; off >= 1; off >>= 1) {
        s0 += __shfl_xor(s0, off, 64);
        s1 += __shfl_xor(s1, off, 64);
    }
}

// grid (C8, S): block (blk, sp) owns elements [e0, e1) of the flat (image, pixel) space of channel block blk.
// mean_io / invstd_io: published by the forward, read by the backward; yres: the residual (forward) or y (backward, relu 1)
template <bool BWD>
__global__ __launch_bounds__(256) void bn16_coop_kernel(const u32x4_t* __restrict__ dy, const u32x4_t* __restrict__ z,
                                                        const u32x4_t* __restrict__ yres, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ mean_io,
                                                        float* __restrict__ invstd_io, float* __restrict__ moving_mean,
                                                        float* __restrict__ moving_var, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta, float* __restrict__ dgamma_acc,
                                                        float* __restrict__ dbeta_acc, u32x4_t* __restrict__ out,
                                                        u32x4_t* __restrict__ dres, double* __restrict__ part,
                                                        unsigned long long* __restrict__ counter, int n, int c, int c8, int hw, int relu,
                                                        float eps, float momentum) {
    const int blk = blockIdx.x, sp = blockIdx.y, nsplit = gridDim.y;
    const Bn16Span span(n, hw, c8, blk, sp, nsplit);
    const BnChannels chan = {gamma, beta, mean_io, invstd_io};
    const BnStatOut stats = {mean_io, invstd_io, moving_mean, moving_var, momentum};
    const BnGradOut grads = {dgamma, dbeta, dgamma_acc, dbeta_acc};
    const Bn16GradLanes L = bn16_grad_lanes<BWD>(blk, c, relu, chan);
    // ---- pass 1: partial sums of this slice
    float f[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = 0.f;
#pragma unroll 4
    for (unsigned e = span.e0 + threadIdx.x; e < span.e1; e += 256)
        bn16_accumulate<BWD>(f, bn16_load<BWD>(z, dy, yres, span.index_of(e), relu), relu, L);
    const double total = bn16_accumulated(f);
    if (threadIdx.x < 16) {
        const int ch = blk * 8 + (threadIdx.x >> 1);
        if (ch < c) __hip_atomic_store(part + ((size_t)ch * nsplit + sp) * 2 + (threadIdx.x & 1), total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // only the workgroups of ONE channel block depend on each other: one barrier slot per channel block, gridDim.y arrivals each
    // (an arrival is a cross-XCD atomic, ~70 ns serialised per address: 128 arrivals on one slot cost ~9 us)
    const bool ok = grid_barrier(counter + (size_t)blk * 16, gridDim.y);
    // ---- totals of the 8 channels, per-channel constants: (scale, shift, -) forward, bn_dz's (k, mb, mg) backward
    __shared__ float s_a[8], s_b[8], s_c[8];
    {
        const int j = threadIdx.x >> 5, ch = blk * 8 + j;
        double s0, s1;
        coop_channel_sums(part, ch, c, nsplit, s0, s1);
        if ((threadIdx.x & 31) == 0) {
            float a = 0.f, b = 0.f, cc = 0.f;
            if (ch < c) {
                if (BWD) {
                    const float db = (float)s0, dg = (float)s1, inv_count = (float)(1.0 / ((double)n * hw));
                    a = chan.gamma[ch] * chan.invstd[ch];
                    b = db * inv_count;
                    cc = dg * inv_count;
                    if (sp == 0) bn_bwd_publish(ch, db, dg, grads);
                } else {
                    const BnStats st = bn_stats(s0, s1, (double)n * hw, eps);
                    a = chan.gamma[ch] * st.invstd;
                    b = bn16_shift(chan.beta[ch], (float)st.mean, a);
                    if (sp == 0) bn_fwd_publish(ch, (float)st.mean, st.invstd, st.var_unbiased(), stats);
                }
                if (!ok) a = b = cc = __builtin_nanf("");  // barrier timed out: poison, never hang
            }
            s_a[j] = a; s_b[j] = b; s_c[j] = cc;
        }
    }
    __syncthreads();
    Bn16DzLanes D;  // forward: k = scale, mb = shift
#pragma unroll
    for (int j = 0; j < 8; ++j) { D.k[j] = s_a[j]; D.mb[j] = s_b[j]; D.mg[j] = s_c[j]; }
    // ---- pass 2 over the same slice (L2-resident)
#pragma unroll 4
    for (unsigned e = span.e0 + threadIdx.x; e < span.e1; e += 256) {
        const size_t i = span.index_of(e);
        if (BWD) {
            u32x4_t oz, og;
            bn16_bwd_elem(bn16_load<true>(z, dy, yres, i, relu), relu, blk, c, L, D, oz, og);
            out[i] = oz;
            if (dres) dres[i] = og;
        } else {
            const h16x8 zv = __builtin_bit_cast(h16x8, z[i]);
            h16x8 rv = zv;
            if (yres) rv = __builtin_bit_cast(h16x8, yres[i]);
            out[i] = bn16_fwd_elem(zv, rv, yres != nullptr, relu, blk, c, D.k, D.mb);
        }
    }
}

// Barrier slots: a zeroed device pool created on the first use outside a stream capture, 128 slots of 128 bytes per stream that ever
// launched a one-launch BatchNorm (the captured graph keeps the slot of its capture stream; kernels of one stream are ordered).
constexpr int kCoopSlots = 64;
static unsigned long long* coop_slot_for(hipStream_t s) {
    static std::mutex mu;
    static unsigned long long* pool = nullptr;
    static bool failed = false;
    static std::unordered_map<hipStream_t, int> slots;
    std::lock_guard<std::mutex> lock(mu);
    if (!pool) {
        if (failed) return nullptr;
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            return nullptr;  // not now: an allocation inside a capture is not allowed; the two-launch form runs instead
        }
        void* p = nullptr;
        if (hipMalloc(&p, (size_t)kCoopSlots * kCoopMaxGrid * 128) != hipSuccess ||
            hipMemset(p, 0, (size_t)kCoopSlots * kCoopMaxGrid * 128) != hipSuccess) {
            (void)hipGetLastError();
            failed = true;
            return nullptr;
        }
        pool = reinterpret_cast<unsigned long long*>(p);
    }
    auto it = slots.find(s);
    if (it == slots.end()) {
        if ((int)slots.size() >= kCoopSlots) return nullptr;
        it = slots.emplace(s, (int)slots.size()).first;
    }
    return pool + (size_t)it->second * kCoopMaxGrid * 16;  // kCoopMaxGrid slots of 128 bytes: one per channel block
}

// the one-launch form applies to: tensors of <= MP_BN16_COOP_MAX (default 512 K) 16-byte elements with C8 <= 128 - measured on the
// HRNet-W32 amp-O2 step at N = 128: threshold 0 / 256 K / 512 K / 1 M -> 36.06 / 35.31 / 35.04 / 36.64 ms
static unsigned long long* bn16_coop_plan(int n, int c8, int hw, hipStream_t s, int& nsplit) {
    static const long long max_elems = [] {
        const char* e = knob("MP_BN16_COOP_MAX");  // 0 switches the one-launch form off
        return e ? atoll(e) : (1LL << 19);
    }();
    if ((long long)n * c8 * hw > max_elems || c8 > kCoopMaxGrid) return nullptr;
    nsplit = kCoopMaxGrid / c8;
    if (nsplit > 32) nsplit = 32;
    while (nsplit > 1 && ((long long)n * hw + nsplit - 1) / nsplit < 256) --nsplit;
    return coop_slot_for(s);
}

// backward of the exchange-unit sum in the c8 layout: g = dy * (out > 0); term k gets the s_k x s_k block sums of g
__global__ __launch_bounds__(256) void fuse_sum16_bwd_kernel(const u32x4_t* __restrict__ dy, const u32x4_t* __restrict__ out,
                                                             u32x4_t* __restrict__ dt, int planes, int h, int w, int sh, int relu) {
    const int lh = h >> sh, lw = w >> sh, s = 1 << sh;
    const size_t total = (size_t)planes * lh * lw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lx = (int)(i % lw);
        const size_t r = i / lw;
        const int ly = (int)(r % lh);
        const size_t plane = r / lh;
        const size_t o = (plane * h + (size_t)ly * s) * w + (size_t)lx * s;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int a = 0; a < s; ++a)
            for (int b = 0; b < s; ++b) {
                const h16x8 gv = __builtin_bit_cast(h16x8, dy[o + (size_t)a * w + b]);
                h16x8 ov = gv;
                if (relu) ov = __builtin_bit_cast(h16x8, out[o + (size_t)a * w + b]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float g = (float)gv[j];
                    if (relu && !((float)ov[j] > 0.f)) g = 0.f;
                    acc[j] += g;
                }
            }
        h16x8 res;
#pragma unroll
        for (int j = 0; j < 8; ++j) res[j] = (_Float16)acc[j];
        dt[i] = __builtin_bit_cast(u32x4_t, res);
    }
}

// out = a + b (+ c) (+ d): the gradients that reach one tensor from its consumers (the exchange unit feeds every branch output to
// every row) summed in ONE pass with fp32 arithmetic - autograd would add them pairwise, k - 1 launches of 3 tensors each.
// fp16: 16-byte units of 8 halves, one rounding at the end.  `out` may alias an input (include/mindpose_hip.h; a running sum
// accumulated in place): every thread reads unit i of all operands before it stores unit i, so no pointer carries __restrict__.
template <bool HALF>
__global__ __launch_bounds__(256) void sum_tensors_kernel(const u32x4_t* a, const u32x4_t* b, const u32x4_t* c, const u32x4_t* d,
                                                          u32x4_t* out, size_t units) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (size_t)gridDim.x * 256) {
        const u32x4_t va = a[i], vb = b[i];
        u32x4_t vc = va, vd = va;
        if (c) vc = c[i];
        if (d) vd = d[i];
        if (HALF) {
            const h16x8 ha = __builtin_bit_cast(h16x8, va), hb = __builtin_bit_cast(h16x8, vb), hc = __builtin_bit_cast(h16x8, vc),
                        hd = __builtin_bit_cast(h16x8, vd);
            h16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float v = (float)ha[j] + (float)hb[j];
                if (c) v += (float)hc[j];
                if (d) v += (float)hd[j];
                o[j] = (_Float16)v;
            }
            out[i] = __builtin_bit_cast(u32x4_t, o);
        } else {
            const float4 fa = __builtin_bit_cast(float4, va), fb = __builtin_bit_cast(float4, vb), fc = __builtin_bit_cast(float4, vc),
                         fd = __builtin_bit_cast(float4, vd);
            float4 o = make_float4(fa.x + fb.x, fa.y + fb.y, fa.z + fb.z, fa.w + fb.w);
            if (c) { o.x += fc.x; o.y += fc.y; o.z += fc.z; o.w += fc.w; }
            if (d) { o.x += fd.x; o.y += fd.y; o.z += fd.z; o.w += fd.w; }
            out[i] = __builtin_bit_cast(u32x4_t, o);
        }
    }
}

// ---- the element-wise producers of a BatchNorm's output gradient, with that BatchNorm's backward sums (round 3) --------------------
// Where the gradient that reaches a BatchNorm does not come out of a data-gradient conv - the sum over the consumers of a branch
// output (FanOutFn), a term of the exchange unit's backward (FuseSum16Fn) - the kernel that writes it takes the conv epilogue's
// role: grid (C8, chunks) like the BatchNorm passes (a block stays inside ONE channel block, so per-channel sums live in registers),
// g = value * [y > 0] stored, partial sums of g and g * z per (channel block, chunk) in the conv epilogue's layout
// [C8][chunks][8][2] fp32.  Fixed partition, fixed order: bit-reproducible.
__device__ __forceinline__ void ew_stats_tail(float (&f)[16], float* __restrict__ part, int blk, int chunk, int n_parts) {
    const double total = bn16_accumulated(f);
    if (threadIdx.x < 16) part[((size_t)blk * n_parts + chunk) * 16 + threadIdx.x] = (float)total;
}

// out = fp16(((a + b) + c) + d) * [y > 0]  (mp_sum_tensors' arithmetic, then the mask)
__global__ __launch_bounds__(256) void sum_tensors16_stats_kernel(const u32x4_t* __restrict__ a, const u32x4_t* __restrict__ b,
                                                                  const u32x4_t* __restrict__ c, const u32x4_t* __restrict__ d,
                                                                  const u32x4_t* __restrict__ z, const u32x4_t* __restrict__ y,
                                                                  u32x4_t* __restrict__ out, float* __restrict__ part, int n, int c8,
                                                                  int hw, int relu) {
    const int blk = blockIdx.x;
    const Bn16Span span(n, hw, c8, blk, blockIdx.y, gridDim.y);
    float f[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = 0.f;
#pragma unroll 2
    for (unsigned e = span.e0 + threadIdx.x; e < span.e1; e += 256) {
        const size_t i = span.index_of(e);
        const h16x8 ha = __builtin_bit_cast(h16x8, a[i]), hb = __builtin_bit_cast(h16x8, b[i]);
        h16x8 hc = ha, hd = ha;
        if (c) hc = __builtin_bit_cast(h16x8, c[i]);
        if (d) hd = __builtin_bit_cast(h16x8, d[i]);
        const h16x8 zv = __builtin_bit_cast(h16x8, z[i]);
        h16x8 yv = zv;
        if (relu) yv = __builtin_bit_cast(h16x8, y[i]);
        h16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = (float)ha[j] + (float)hb[j];
            if (c) v += (float)hc[j];
            if (d) v += (float)hd[j];
            _Float16 h = (_Float16)v;
            if (relu && !((float)yv[j] > 0.f)) h = (_Float16)0.f;
            o[j] = h;
            f[2 * j] += (float)h;
            f[2 * j + 1] = __builtin_fmaf((float)h, (float)zv[j], f[2 * j + 1]);
        }
        out[i] = __builtin_bit_cast(u32x4_t, o);
    }
    ew_stats_tail(f, part, blk, blockIdx.y, gridDim.y);
}

// one term of the exchange unit's backward: dt = fp16(sum over the s x s block of dy * [out > 0]) * [y_t > 0]
// (SH = log2 of the scale as a template parameter: the s x s block is walked by fully unrolled loops whose 2 s loads per row
// are all issued before the first use - with a run-time s the thread had one load in flight at a time)
template <int SH>
__global__ __launch_bounds__(256) void fuse_sum16_bwd_stats_kernel(const u32x4_t* __restrict__ dy, const u32x4_t* __restrict__ outp,
                                                                   const u32x4_t* __restrict__ z, const u32x4_t* __restrict__ y,
                                                                   u32x4_t* __restrict__ dt, float* __restrict__ part, int n, int c8, int h,
                                                                   int w, int relu, int relu_t) {
    constexpr int sh = SH;
    const int blk = blockIdx.x;
    const int lh = h >> sh, lw = w >> sh, lhw = lh * lw;
    constexpr int s = 1 << SH;
    const unsigned per_blk = (unsigned)n * (unsigned)lhw;
    const unsigned len = (per_blk + gridDim.y - 1) / gridDim.y;
    const unsigned e0 = blockIdx.y * len, e1 = e0 + len < per_blk ? e0 + len : per_blk;
    float f[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = 0.f;
    for (unsigned e = e0 + threadIdx.x; e < e1; e += 256) {
        const unsigned img = e / (unsigned)lhw, pix = e - img * (unsigned)lhw;
        const unsigned ly = pix / (unsigned)lw, lx = pix - ly * (unsigned)lw;
        const size_t plane = (size_t)img * c8 + blk;
        const size_t i = plane * lhw + pix;
        const size_t o = (plane * h + (size_t)ly * s) * w + (size_t)lx * s;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // same summation order as before (row by row, left to right): same bits
#pragma unroll
        for (int a = 0; a < s; ++a) {
            u32x4_t gq[s], oq[s];
#pragma unroll
            for (int b = 0; b < s; ++b) {
                gq[b] = dy[o + (size_t)a * w + b];
                oq[b] = relu ? outp[o + (size_t)a * w + b] : gq[b];
            }
#pragma unroll
            for (int b = 0; b < s; ++b) {
                const h16x8 gv = __builtin_bit_cast(h16x8, gq[b]), ov = __builtin_bit_cast(h16x8, oq[b]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float g = (float)gv[j];
                    if (relu && !((float)ov[j] > 0.f)) g = 0.f;
                    acc[j] += g;
                }
            }
        }
        const h16x8 zv = __builtin_bit_cast(h16x8, z[i]);
        h16x8 yv = zv;
        if (relu_t) yv = __builtin_bit_cast(h16x8, y[i]);
        h16x8 res;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            _Float16 hv = (_Float16)acc[j];
            if (relu_t && !((float)yv[j] > 0.f)) hv = (_Float16)0.f;
            res[j] = hv;
            f[2 * j] += (float)hv;
            f[2 * j + 1] = __builtin_fmaf((float)hv, (float)zv[j], f[2 * j + 1]);
        }
        dt[i] = __builtin_bit_cast(u32x4_t, res);
    }
    ew_stats_tail(f, part, blk, blockIdx.y, gridDim.y);
}

// image groups x pixel chunks of the fp16 reductions: about 512+ blocks, fixed by the shape (deterministic)
static void bn16_split(int n, int c8, int hw, int& gi, int& gp) {
    int want = 512 / c8;  // a block should stream >= ~50 KB to amortise its reduction tail
    if (want < 32) want = 32;
    if (want > kBn16MaxSplit) want = kBn16MaxSplit;
    gi = n < want ? n : want;
    gp = want / gi;
    if (gp < 1) gp = 1;
    while (gp > 1 && (hw + gp - 1) / gp < 256) --gp;  // at least one element per thread
}

// pixel-range chunks per channel block of the apply kernels: ~768 blocks in all, each streaming at least 1024 elements
static unsigned bn16_apply_chunks(int n, int c8, int hw) {
    size_t chunks = (768 + c8 - 1) / c8;
    const size_t per_blk = (size_t)n * hw;
    while (chunks > 1 && per_blk / chunks < 1024) --chunks;
    return (unsigned)chunks;
}

static int log2_exact_t(int v) {
    for (int i = 0; i < 16; ++i)
        if ((1 << i) == v) return i;
    return -1;
}

// pixel-range chunks per channel block of the statistics-free apply kernels.  These passes are bound by the bytes they keep in
// flight (a thread has 4 x 16 B per operand tensor outstanding), not by the n_parts x 64 bytes of partials every block folds first:
// ~1024 blocks (four per CU) of >= 1024 elements measured best on every map size of the HRNet step - 512 fatter blocks ran the
// 64x48 maps at 2.2 TB/s, 1024 at 3.3 TB/s; 2048 and more lose again to the redundant folds (round 3 sweep with MP_BN_PRE_BLOCKS / MP_BN_PRE_MIN, tools/ab_train.sh).
static unsigned bn16_pre_chunks(int n, int c8, int hw) {
    size_t total = 1024, floor_elems = 1024;
    if (const char* e = knob("MP_BN_PRE_BLOCKS")) total = (size_t)atoi(e);
    if (const char* e = knob("MP_BN_PRE_MIN")) floor_elems = (size_t)atoi(e);
    size_t chunks = (total + c8 - 1) / c8;
    const size_t per_blk = (size_t)n * hw;
    while (chunks > 1 && per_blk / chunks < floor_elems) --chunks;
    return (unsigned)chunks;
}

// more slots than a consumer block folds: reduce them to one per channel block (into the workspace)
static int bn16_prefold(const float*& pre, int& n_parts, int c8, void* workspace, hipStream_t s) {
    int above = kMaxFoldParts;
    if (const char* e = knob("MP_BN_PREFOLD_ABOVE")) above = atoi(e);
    if (n_parts <= above) return MP_OK;
    float* folded = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(bn16_fold_kernel, dim3(c8, kFoldSplit), dim3(256), 0, s, pre, folded, n_parts);
    pre = folded;
    n_parts = kFoldSplit;
    return check_launch();
}

// the accumulating pair is taken only when both are given
static BnGradOut bn_grad_out(float* dgamma, float* dbeta, float* dgamma_acc, float* dbeta_acc) {
    const bool acc = dgamma_acc && dbeta_acc;
    return {dgamma, dbeta, acc ? dgamma_acc : nullptr, acc ? dbeta_acc : nullptr};
}

// What an fp16 BatchNorm entry checks, in the order it checks it, and the argument record its kernels take - one function per
// direction, for the one-layer entries and for every job of the grouped ones (an entry's arguments travel in the job's form).
// An apply-only entry also folds its partial slots when a block would not (bn16_prefold) - at fold_off of the workspace, which
// jobs of one grouped call may share (chains on one stream): job j folds into its own region behind those of the jobs before it.
enum Bn16Entry { kBn16Reducing, kBn16ApplyOnly, kBn16Finalize };
// the apply-only part of either direction: the partial slots (folded first when a block would not), the chunks of the grid
template <class Args, class Job> static int bn16_fill_pre(Args& a, const Job& q, size_t fold_off, hipStream_t s) {
    if (q.workspace_bytes < fold_off + (size_t)a.c8 * kFoldSplit * 16 * sizeof(float)) return MP_ERR_WORKSPACE;
    a.pre = q.partials_dev;
    a.n_parts = q.n_parts;
    a.chunks = bn16_pre_chunks(q.n, a.c8, q.hw);
    return bn16_prefold(a.pre, a.n_parts, a.c8, reinterpret_cast<char*>(q.workspace_dev) + fold_off, s);
}
static int bn16_fwd_fill(Bn16FwdArgs& a, const mp_f16_bn_fwd_job& q, Bn16Entry kind, float eps, float momentum, size_t fold_off, hipStream_t s) {
    const bool pre = kind != kBn16Reducing;
    if ((kind != kBn16Finalize && (!q.z_dev || !q.y_dev)) || !q.gamma_dev || !q.beta_dev || !q.save_mean_dev || !q.save_invstd_dev ||
        (pre && !q.partials_dev))
        return MP_ERR_NULL;
    if ((q.moving_mean_dev == nullptr) != (q.moving_var_dev == nullptr)) return MP_ERR_NULL;
    if (q.n <= 0 || q.c <= 0 || q.hw <= 0 || (pre && q.n_parts <= 0)) return MP_ERR_SHAPE;
    if (!q.workspace_dev || q.workspace_bytes < mp_bn_workspace_bytes(q.c)) return MP_ERR_WORKSPACE;
    a = Bn16FwdArgs{};
    a.z = reinterpret_cast<const u32x4_t*>(q.z_dev);
    a.res = reinterpret_cast<const u32x4_t*>(q.res_dev);
    a.y = reinterpret_cast<u32x4_t*>(q.y_dev);
    a.chan = {q.gamma_dev, q.beta_dev, nullptr, nullptr};
    a.out = {q.save_mean_dev, q.save_invstd_dev, q.moving_mean_dev, q.moving_var_dev, momentum};
    a.eps = eps;
    a.n = q.n, a.c = q.c, a.c8 = (q.c + 7) / 8, a.hw = q.hw, a.relu = q.relu ? 1 : 0;
    const double cnt = (double)q.n * q.hw;
    a.inv_count = 1.0 / cnt;
    a.unbias = cnt > 1.0 ? cnt / (cnt - 1.0) : 1.0;
    return pre ? bn16_fill_pre(a, q, fold_off, s) : MP_OK;
}

// y / beta / dres / relu: the reducing entry's (an apply-only entry takes its gradient pre-masked: relu 0)
static int bn16_bwd_fill(Bn16BwdArgs& a, const mp_f16_bn_bwd_job& q, const void* y, const float* beta, void* dres, int relu, bool pre,
                         size_t fold_off, hipStream_t s) {
    if (!q.g_dev || !q.z_dev || !q.gamma_dev || !q.save_mean_dev || !q.save_invstd_dev || !q.dz_dev || !q.dgamma_dev || !q.dbeta_dev ||
        (pre && !q.partials_dev))
        return MP_ERR_NULL;
    // ReLU mask: from the stored output y - or, for a layer without residual input, re-derived from z with the forward arithmetic
    // (y == NULL, beta given): y is then not read at all
    if (relu && !y && (!beta || dres)) return MP_ERR_NULL;
    if (q.n <= 0 || q.c <= 0 || q.hw <= 0 || (pre && q.n_parts <= 0)) return MP_ERR_SHAPE;
    if (!q.workspace_dev || q.workspace_bytes < mp_bn_workspace_bytes(q.c)) return MP_ERR_WORKSPACE;
    a = Bn16BwdArgs{};
    a.g = reinterpret_cast<const u32x4_t*>(q.g_dev);
    a.z = reinterpret_cast<const u32x4_t*>(q.z_dev);
    a.y = reinterpret_cast<const u32x4_t*>(y);
    a.dz = reinterpret_cast<u32x4_t*>(q.dz_dev);
    a.dres = reinterpret_cast<u32x4_t*>(dres);
    a.chan = {q.gamma_dev, beta, q.save_mean_dev, q.save_invstd_dev};
    a.out = bn_grad_out(q.dgamma_dev, q.dbeta_dev, q.dgamma_acc_dev, q.dbeta_acc_dev);
    a.inv_count = (float)(1.0 / ((double)q.n * q.hw));
    a.n = q.n, a.c = q.c, a.c8 = (q.c + 7) / 8, a.hw = q.hw, a.relu = relu ? (y ? 1 : 2) : 0;
    return pre ? bn16_fill_pre(a, q, fold_off, s) : MP_OK;
}

// the flat grid of a grouped launch: job j's blocks start at `first`; table entries behind the last job are never picked
template <class Args> static unsigned bn16_place_jobs(Bn16Jobs<Args>& t, int n_jobs) {
    unsigned total = 0;
    for (int j = 0; j < kBnJobs; ++j) {
        t.job[j].first = j < n_jobs ? total : 0xFFFFFFFFu;
        if (j < n_jobs) total += (unsigned)t.job[j].c8 * t.job[j].chunks;
    }
    return total;
}

}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_bn_workspace_bytes(int c) {
    if (c <= 0) return 0;
    // fp64 partials [C][splits][2] (32 splits in the fp32 passes, up to kBn16MaxSplit in the fp16 ones) + scale/shift
    return (size_t)c * kBn16MaxSplit * 2 * sizeof(double) + (size_t)c * 2 * sizeof(float) + 256;
}

int mp_bn_train_fwd(const float* z, const float* gamma, const float* beta, const float* res, float* y, float* save_mean,
                    float* save_invstd, float* moving_mean, float* moving_var, int n, int c, int hw, float eps,
                    float momentum, int relu, void* workspace, size_t workspace_bytes, mp_stream_t stream) {
    if (!z || !gamma || !beta || !y || !save_mean || !save_invstd) return MP_ERR_NULL;
    if ((moving_mean == nullptr) != (moving_var == nullptr)) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || hw <= 0) return MP_ERR_SHAPE;
    if (!workspace || workspace_bytes < mp_bn_workspace_bytes(c)) return MP_ERR_WORKSPACE;
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(bn_reduce_kernel<false>, dim3(c, kBnSplit), dim3(256), 0, s, nullptr, z, nullptr, nullptr, nullptr, part,
                       n, c, hw, 0);
    int rc = check_launch();
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(n * c), dim3(256), 0, s, z, part, gamma, beta, save_mean, save_invstd, moving_mean,
                       moving_var, res, y, c, hw, relu ? 1 : 0, (double)n * hw, eps, momentum);
    return check_launch();
}

int mp_bn_train_bwd(const float* dy, const float* z, const float* y, const float* gamma, const float* save_mean,
                    const float* save_invstd, float* dz, float* dres, float* dgamma, float* dbeta, int n, int c, int hw,
                    int relu, void* workspace, size_t workspace_bytes, mp_stream_t stream) {
    return mp_bn_train_bwd_acc(dy, z, y, gamma, save_mean, save_invstd, dz, dres, dgamma, dbeta, nullptr, nullptr, n, c, hw, relu,
                               workspace, workspace_bytes, stream);
}

int mp_bn_train_bwd_acc(const float* dy, const float* z, const float* y, const float* gamma, const float* save_mean,
                        const float* save_invstd, float* dz, float* dres, float* dgamma, float* dbeta, float* dgamma_acc,
                        float* dbeta_acc, int n, int c, int hw, int relu, void* workspace, size_t workspace_bytes,
                        mp_stream_t stream) {
    if (!dy || !z || !gamma || !save_mean || !save_invstd || !dz || !dgamma || !dbeta) return MP_ERR_NULL;
    if (relu && !y) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || hw <= 0) return MP_ERR_SHAPE;
    if (!workspace || workspace_bytes < mp_bn_workspace_bytes(c)) return MP_ERR_WORKSPACE;
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(bn_reduce_kernel<true>, dim3(c, kBnSplit), dim3(256), 0, s, dy, z, y, save_mean, save_invstd, part, n, c,
                       hw, relu ? 1 : 0);
    int rc = check_launch();
    if (rc != MP_OK) return rc;
    const BnGradOut acc = bn_grad_out(dgamma, dbeta, dgamma_acc, dbeta_acc);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(n * c), dim3(256), 0, s, dy, z, y, part, gamma, save_mean, save_invstd, dgamma, dbeta,
                       acc.dgamma_acc, acc.dbeta_acc, dz, dres, c, hw, relu ? 1 : 0, (float)(1.0 / ((double)n * hw)));
    return check_launch();
}

int mp_fuse_upsample_sum_bwd(const float* dy, const float* out, float* dbase, float* dt1, int s1, float* dt2, int s2,
                             float* dt3, int s3, int n, int c, int h, int w, int relu, mp_stream_t stream) {
    if (!dy || (relu && !out)) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    hipStream_t s = as_stream(stream);
    float* dts[4] = {dbase, dt1, dt2, dt3};
    const int ss[4] = {1, s1, s2, s3};
    for (int k = 0; k < 4; ++k) {
        if (!dts[k]) continue;
        const int sh = log2_exact_t(ss[k]);
        if (sh < 0 || (h % ss[k]) || (w % ss[k])) return MP_ERR_UNSUPPORTED;
        const size_t total = (size_t)n * c * (h >> sh) * (w >> sh);
        size_t blocks = (total + 255) / 256;
        if (blocks > 256 * 32) blocks = 256 * 32;
        hipLaunchKernelGGL(fuse_sum_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dy, out, dts[k], n * c, h, w, sh, relu ? 1 : 0);
        int rc = check_launch();
        if (rc != MP_OK) return rc;
    }
    return MP_OK;
}

// The reducing forms of a validated record (bn16_fwd_fill / bn16_bwd_fill): every kernel argument comes from the record, none from the
// entry's own parameters.  Small map: both passes in one launch; otherwise reduce, then apply.
static int bn16_fwd_reducing(const Bn16FwdArgs& a, double* part, hipStream_t s) {
    const BnChannels& ch = a.chan;
    const BnStatOut& o = a.out;
    int coop_split;
    if (unsigned long long* counter = bn16_coop_plan(a.n, a.c8, a.hw, s, coop_split)) {
        hipLaunchKernelGGL(bn16_coop_kernel<false>, dim3(a.c8, coop_split), dim3(256), 0, s, nullptr, a.z, a.res, ch.gamma, ch.beta, o.save_mean,
                           o.save_invstd, o.moving_mean, o.moving_var, nullptr, nullptr, nullptr, nullptr, a.y, nullptr, part, counter, a.n, a.c,
                           a.c8, a.hw, a.relu, a.eps, o.momentum);
        return check_launch();
    }
    int gi, gp;
    bn16_split(a.n, a.c8, a.hw, gi, gp);
    hipLaunchKernelGGL(bn16_reduce_kernel<false>, dim3(a.c8, gi * gp), dim3(256), 0, s, nullptr, a.z, nullptr, nullptr, nullptr, nullptr,
                       nullptr, part, a.n, a.c, a.c8, a.hw, 0, gi, gp);
    const int rc = check_launch();
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(bn16_apply_kernel, dim3(a.c8, bn16_apply_chunks(a.n, a.c8, a.hw)), dim3(256), 0, s, a.z, part, ch.gamma, ch.beta,
                       o.save_mean, o.save_invstd, o.moving_mean, o.moving_var, a.res, a.y, a.n, a.c, a.c8, a.hw, gi * gp,
                       (double)a.n * a.hw, a.eps, o.momentum, a.relu);
    return check_launch();
}

static int bn16_bwd_reducing(const Bn16BwdArgs& a, double* part, hipStream_t s) {
    const BnChannels& ch = a.chan;
    const BnGradOut& o = a.out;
    int coop_split;
    if (unsigned long long* counter = bn16_coop_plan(a.n, a.c8, a.hw, s, coop_split)) {
        hipLaunchKernelGGL(bn16_coop_kernel<true>, dim3(a.c8, coop_split), dim3(256), 0, s, a.g, a.z, a.y, ch.gamma, ch.beta,
                           const_cast<float*>(ch.mean), const_cast<float*>(ch.invstd), nullptr, nullptr, o.dgamma, o.dbeta, o.dgamma_acc,
                           o.dbeta_acc, a.dz, a.dres, part, counter, a.n, a.c, a.c8, a.hw, a.relu, 0.f, 0.f);
        return check_launch();
    }
    int gi, gp;
    bn16_split(a.n, a.c8, a.hw, gi, gp);
    hipLaunchKernelGGL(bn16_reduce_kernel<true>, dim3(a.c8, gi * gp), dim3(256), 0, s, a.g, a.z, a.y, ch.mean, ch.invstd, ch.gamma, ch.beta,
                       part, a.n, a.c, a.c8, a.hw, a.relu, gi, gp);
    const int rc = check_launch();
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(bn16_bwd_apply_kernel, dim3(a.c8, bn16_apply_chunks(a.n, a.c8, a.hw)), dim3(256), 0, s, a.g, a.z, a.y, part, ch.gamma,
                       ch.mean, ch.invstd, o.dgamma, o.dbeta, o.dgamma_acc, o.dbeta_acc, a.dz, a.dres, a.n, a.c, a.c8, a.hw, gi * gp, a.relu,
                       a.inv_count, ch.beta);
    return check_launch();
}

int mp_f16_bn_train_fwd(const void* z, const float* gamma, const float* beta, const void* res, void* y, float* save_mean,
                        float* save_invstd, float* moving_mean, float* moving_var, int n, int c, int hw, float eps, float momentum,
                        int relu, void* workspace, size_t workspace_bytes, mp_stream_t stream) {
    const mp_f16_bn_fwd_job q = {z, gamma, beta, res, y, save_mean, save_invstd, moving_mean, moving_var, nullptr, workspace, workspace_bytes,
                                 n, c, hw, relu, 0, 0};
    hipStream_t s = as_stream(stream);
    Bn16FwdArgs a;
    const int rc = bn16_fwd_fill(a, q, kBn16Reducing, eps, momentum, 0, s);
    return rc != MP_OK ? rc : bn16_fwd_reducing(a, reinterpret_cast<double*>(workspace), s);
}

int mp_f16_bn_train_bwd(const void* dy, const void* z, const void* y, const float* gamma, const float* beta, const float* save_mean,
                        const float* save_invstd, void* dz, void* dres, float* dgamma, float* dbeta, float* dgamma_acc, float* dbeta_acc,
                        int n, int c, int hw, int relu, void* workspace, size_t workspace_bytes, mp_stream_t stream) {
    const mp_f16_bn_bwd_job q = {dy, z, gamma, save_mean, save_invstd, dz, dgamma, dbeta, dgamma_acc, dbeta_acc, nullptr, workspace,
                                 workspace_bytes, n, c, hw, 0};
    hipStream_t s = as_stream(stream);
    Bn16BwdArgs a;
    const int rc = bn16_bwd_fill(a, q, y, beta, dres, relu, false, 0, s);
    return rc != MP_OK ? rc : bn16_bwd_reducing(a, reinterpret_cast<double*>(workspace), s);
}

int mp_f16_bn_train_fwd_stats(const void* z, const float* gamma, const float* beta, const void* res, void* y, float* save_mean,
                              float* save_invstd, float* moving_mean, float* moving_var, int n, int c, int hw, float eps,
                              float momentum, int relu, const float* partials, int n_parts, void* workspace, size_t workspace_bytes,
                              mp_stream_t stream) {
    const mp_f16_bn_fwd_job q = {z, gamma, beta, res, y, save_mean, save_invstd, moving_mean, moving_var, partials, workspace, workspace_bytes,
                                 n, c, hw, relu, n_parts, 0};
    hipStream_t s = as_stream(stream);
    Bn16FwdArgs a;
    const int rc = bn16_fwd_fill(a, q, kBn16ApplyOnly, eps, momentum, 0, s);
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(bn16_apply_pre_kernel, dim3(a.c8, a.chunks), dim3(256), 0, s, a);
    return check_launch();
}

int mp_f16_bn_train_finalize(const float* gamma, const float* beta, float* save_mean, float* save_invstd, float* moving_mean,
                             float* moving_var, int n, int c, int hw, float eps, float momentum, const float* partials, int n_parts,
                             float* scale, float* shift, void* workspace, size_t workspace_bytes, mp_stream_t stream) {
    if (!scale || !shift) return MP_ERR_NULL;
    const mp_f16_bn_fwd_job q = {nullptr, gamma, beta, nullptr, nullptr, save_mean, save_invstd, moving_mean, moving_var, partials, workspace,
                                 workspace_bytes, n, c, hw, 0, n_parts, 0};
    hipStream_t s = as_stream(stream);
    Bn16FwdArgs a;
    const int rc = bn16_fwd_fill(a, q, kBn16Finalize, eps, momentum, 0, s);
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(bn16_finalize_kernel, dim3(a.c8), dim3(256), 0, s, a, scale, shift);
    return check_launch();
}

int mp_f16_bn_train_bwd_stats(const void* g, const void* z, const float* gamma, const float* save_mean, const float* save_invstd,
                              void* dz, float* dgamma, float* dbeta, float* dgamma_acc, float* dbeta_acc, int n, int c, int hw,
                              const float* partials, int n_parts, void* workspace, size_t workspace_bytes, mp_stream_t stream) {
    const mp_f16_bn_bwd_job q = {g, z, gamma, save_mean, save_invstd, dz, dgamma, dbeta, dgamma_acc, dbeta_acc, partials, workspace,
                                 workspace_bytes, n, c, hw, n_parts};
    hipStream_t s = as_stream(stream);
    Bn16BwdArgs a;
    const int rc = bn16_bwd_fill(a, q, nullptr, nullptr, nullptr, 0, true, 0, s);
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(bn16_bwd_apply_pre_kernel, dim3(a.c8, a.chunks), dim3(256), 0, s, a);
    return check_launch();
}

// Grouped apply passes (kernels above): job j must satisfy what the one-layer entries check; a job with more than kMaxFoldParts
// partial slots is folded by its own bn16_fold_kernel launch first (its region of the workspace).
int mp_f16_bn_train_fwd_stats_grouped(const mp_f16_bn_fwd_job* jobs, int n_jobs, float eps, float momentum, mp_stream_t stream) {
    if (!jobs) return MP_ERR_NULL;
    if (n_jobs < 1 || n_jobs > kBnJobs) return MP_ERR_SHAPE;
    hipStream_t s = as_stream(stream);
    Bn16Jobs<Bn16FwdArgs> t{};
    size_t fold_off = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int rc = bn16_fwd_fill(t.job[j], jobs[j], kBn16ApplyOnly, eps, momentum, fold_off, s);
        if (rc != MP_OK) return rc;
        fold_off += ((size_t)t.job[j].c8 * kFoldSplit * 16 * sizeof(float) + 255) / 256 * 256;
    }
    const unsigned total = bn16_place_jobs(t, n_jobs);
    hipLaunchKernelGGL(bn16_apply_pre_grouped_kernel, dim3(total), dim3(256), 0, s, t);
    return check_launch();
}

int mp_f16_bn_train_bwd_stats_grouped(const mp_f16_bn_bwd_job* jobs, int n_jobs, mp_stream_t stream) {
    if (!jobs) return MP_ERR_NULL;
    if (n_jobs < 1 || n_jobs > kBnJobs) return MP_ERR_SHAPE;
    hipStream_t s = as_stream(stream);
    Bn16Jobs<Bn16BwdArgs> t{};
    size_t fold_off = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int rc = bn16_bwd_fill(t.job[j], jobs[j], nullptr, nullptr, nullptr, 0, true, fold_off, s);
        if (rc != MP_OK) return rc;
        fold_off += ((size_t)t.job[j].c8 * kFoldSplit * 16 * sizeof(float) + 255) / 256 * 256;
    }
    const unsigned total = bn16_place_jobs(t, n_jobs);
    hipLaunchKernelGGL(bn16_bwd_apply_pre_grouped_kernel, dim3(total), dim3(256), 0, s, t);
    return check_launch();
}

int mp_f16_fuse_upsample_sum_bwd(const void* dy, const void* out, void* dbase, void* dt1, int s1, void* dt2, int s2, void* dt3,
                                 int s3, int n, int c, int h, int w, int relu, mp_stream_t stream) {
    if (!dy || (relu && !out)) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    hipStream_t s = as_stream(stream);
    void* dts[4] = {dbase, dt1, dt2, dt3};
    const int ss[4] = {1, s1, s2, s3};
    const int planes = n * ((c + 7) / 8);
    for (int k = 0; k < 4; ++k) {
        if (!dts[k]) continue;
        const int sh = log2_exact_t(ss[k]);
        if (sh < 0 || (h % ss[k]) || (w % ss[k])) return MP_ERR_UNSUPPORTED;
        const size_t total = (size_t)planes * (h >> sh) * (w >> sh);
        size_t blocks = (total + 255) / 256;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(fuse_sum16_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const u32x4_t*>(dy),
                           reinterpret_cast<const u32x4_t*>(out), reinterpret_cast<u32x4_t*>(dts[k]), planes, h, w, sh, relu ? 1 : 0);
        int rc = check_launch();
        if (rc != MP_OK) return rc;
    }
    return MP_OK;
}

int mp_f16_ew_stats_parts(int n, int c, int hw) {
    if (n <= 0 || c <= 0 || hw <= 0) return 0;
    return (int)bn16_apply_chunks(n, (c + 7) / 8, hw);
}

// a term at scale s sums s x s gradient elements per output element: blocks of >= 1024 / s^2 outputs (>= 64) keep the chip busy on
// the low-resolution terms
int mp_f16_fuse_term_stats_parts(int n, int c, int h, int w, int s) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || s <= 0 || (h % s) || (w % s)) return 0;
    const int c8 = (c + 7) / 8;
    const size_t per_blk = (size_t)n * (h / s) * (w / s);
    size_t min_elems = 1024 / ((size_t)s * s);
    if (min_elems < 64) min_elems = 64;
    size_t chunks = (768 + c8 - 1) / c8;
    while (chunks > 1 && per_blk / chunks < min_elems) --chunks;
    return (int)chunks;
}

int mp_f16_sum_tensors_stats(const void* a, const void* b, const void* c, const void* d, void* out, const void* z, const void* y,
                             int relu, int n, int ch, int hw, float* partials, size_t partials_bytes, mp_stream_t stream) {
    if (!a || !b || !out || !z || !partials || (relu && !y)) return MP_ERR_NULL;
    if (d && !c) return MP_ERR_NULL;
    if (n <= 0 || ch <= 0 || hw <= 0) return MP_ERR_SHAPE;
    const int c8 = (ch + 7) / 8, parts = mp_f16_ew_stats_parts(n, ch, hw);
    if (partials_bytes < (size_t)c8 * parts * 16 * sizeof(float)) return MP_ERR_WORKSPACE;
    hipLaunchKernelGGL(sum_tensors16_stats_kernel, dim3(c8, parts), dim3(256), 0, as_stream(stream), reinterpret_cast<const u32x4_t*>(a),
                       reinterpret_cast<const u32x4_t*>(b), reinterpret_cast<const u32x4_t*>(c), reinterpret_cast<const u32x4_t*>(d),
                       reinterpret_cast<const u32x4_t*>(z), reinterpret_cast<const u32x4_t*>(y), reinterpret_cast<u32x4_t*>(out), partials, n,
                       c8, hw, relu ? 1 : 0);
    return check_launch();
}

int mp_f16_fuse_sum_bwd_term_stats(const void* dy, const void* out, void* dt, int s, int n, int c, int h, int w, int relu, const void* z_t,
                                   const void* y_t, int relu_t, float* partials, size_t partials_bytes, mp_stream_t stream) {
    if (!dy || !dt || !z_t || !partials || (relu && !out) || (relu_t && !y_t)) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    const int sh = log2_exact_t(s);
    if (sh < 0 || (h % s) || (w % s)) return MP_ERR_UNSUPPORTED;
    const int c8 = (c + 7) / 8, parts = mp_f16_fuse_term_stats_parts(n, c, h, w, s);
    if (partials_bytes < (size_t)c8 * parts * 16 * sizeof(float)) return MP_ERR_WORKSPACE;
    if (sh > 3) return MP_ERR_UNSUPPORTED;  // HRNet's exchange units up-sample by 2, 4 and 8 (1: the identity term)
    auto kern = sh == 0 ? fuse_sum16_bwd_stats_kernel<0> : sh == 1 ? fuse_sum16_bwd_stats_kernel<1>
              : sh == 2 ? fuse_sum16_bwd_stats_kernel<2> : fuse_sum16_bwd_stats_kernel<3>;
    hipLaunchKernelGGL(kern, dim3(c8, parts), dim3(256), 0, as_stream(stream), reinterpret_cast<const u32x4_t*>(dy),
                       reinterpret_cast<const u32x4_t*>(out), reinterpret_cast<const u32x4_t*>(z_t), reinterpret_cast<const u32x4_t*>(y_t),
                       reinterpret_cast<u32x4_t*>(dt), partials, n, c8, h, w, relu ? 1 : 0, relu_t ? 1 : 0);
    return check_launch();
}

int mp_sum_tensors(const void* a, const void* b, const void* c, const void* d, void* out, size_t bytes, int half, mp_stream_t stream) {
    if (!a || !b || !out) return MP_ERR_NULL;
    if (d && !c) return MP_ERR_NULL;
    if (bytes == 0 || (bytes & 15)) return MP_ERR_SHAPE;
    const size_t units = bytes / 16;
    size_t blocks = (units + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    const u32x4_t *pa = reinterpret_cast<const u32x4_t*>(a), *pb = reinterpret_cast<const u32x4_t*>(b),
                  *pc = reinterpret_cast<const u32x4_t*>(c), *pd = reinterpret_cast<const u32x4_t*>(d);
    if (half)
        hipLaunchKernelGGL(sum_tensors_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), pa, pb, pc, pd,
                           reinterpret_cast<u32x4_t*>(out), units);
    else
        hipLaunchKernelGGL(sum_tensors_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), pa, pb, pc, pd,
                           reinterpret_cast<u32x4_t*>(out), units);
    return check_launch();
}

}  // extern "C"
