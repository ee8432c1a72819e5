// Bottom-up (associative-embedding) training ends: the masked heat-map MSE, the AE push / pull loss, both with their analytic
// backward, and the batched target generator.  Reference: mindpose/models/loss/mse.py:47-72 (JointsMSELossWithMask),
// mindpose/models/loss/ae.py:40-89 (AELoss), mindpose/data/transform/bottomup_transform.py:527-598 (BottomUpGenerateTarget).
// Plain HIP C++: no inline assembly, no atomics; every reduction has a fixed order, so two runs are bit-identical.
#include "common.h"
#include "reduce.h"

namespace mp {
namespace {

// ------------------------------------------------------------------------------------------
// JointsMSELossWithMask: L = sum((pred - target)^2 * mask[n,h,w]) / (N K H W).  The operands are views (the first K channels of
// a stage output, a corner of the padded target, a corner of the mask), read in place through element strides; the column
// stride is 1.  One workgroup per (n, k) plane -> fp32 partial, one workgroup sums the partials in fp64 in a fixed order.
// ------------------------------------------------------------------------------------------
struct MseMaskParams {
    const float* pred;
    const float* tgt;
    const void* mask;
    const float* gout;  // backward only
    float* out;         // forward: partials; backward: gradient
    long long ps_n, ps_c, ps_r, ts_n, ts_c, ts_r, ms_n, ms_r, gs_n, gs_c, gs_r;
    int k, h, w;
    float scale;  // backward: 2 / (N K H W)
};

__device__ __forceinline__ void load_mask4(const float* p, float (&m)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
}
__device__ __forceinline__ void load_mask4(const uint8_t* p, float (&m)[4]) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    m[0] = (float)(v & 0xffu); m[1] = (float)((v >> 8) & 0xffu); m[2] = (float)((v >> 16) & 0xffu); m[3] = (float)(v >> 24);
}

template <typename MaskT, bool VEC>
__global__ __launch_bounds__(256) void mse_mask_fwd_kernel(MseMaskParams p) {
    const int row = blockIdx.x, n = row / p.k, c = row - n * p.k;
    const float* a = p.pred + n * p.ps_n + c * p.ps_c;
    const float* b = p.tgt + n * p.ts_n + c * p.ts_c;
    const MaskT* mk = reinterpret_cast<const MaskT*>(p.mask) + n * p.ms_n;
    float acc = 0.f;
    if (VEC) {
        const int wq = p.w >> 2, nq = p.h * wq;
        for (int q = threadIdx.x; q < nq; q += blockDim.x) {
            const int y = q / wq, x = (q - y * wq) << 2;
            const float4 u = *reinterpret_cast<const float4*>(a + y * p.ps_r + x);
            const float4 v = *reinterpret_cast<const float4*>(b + y * p.ts_r + x);
            float m[4];
            load_mask4(mk + y * p.ms_r + x, m);
            const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
            acc += (d0 * d0) * m[0];
            acc += (d1 * d1) * m[1];
            acc += (d2 * d2) * m[2];
            acc += (d3 * d3) * m[3];
        }
    } else {
        const int hw = p.h * p.w;
        for (int i = threadIdx.x; i < hw; i += blockDim.x) {
            const int y = i / p.w, x = i - y * p.w;
            const float d = a[y * p.ps_r + x] - b[y * p.ts_r + x];
            acc += (d * d) * (float)mk[y * p.ms_r + x];
        }
    }
    __shared__ float ws[4];
    acc = block_sum_lane0(wave_sum(acc), ws);
    if (threadIdx.x == 0) p.out[row] = acc;
}

__global__ __launch_bounds__(256) void mse_mask_final_kernel(const float* __restrict__ partial, float* __restrict__ loss, int rows,
                                                             double inv_count) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < rows; i += blockDim.x) acc += (double)partial[i];
    __shared__ double sm4[4];
    acc = block_sum_all(acc, sm4);
    if (threadIdx.x == 0) loss[0] = (float)(acc * inv_count);
}

template <typename MaskT, bool VEC>
__global__ __launch_bounds__(256) void mse_mask_bwd_kernel(MseMaskParams p) {
    const int row = blockIdx.x, n = row / p.k, c = row - n * p.k;
    const float* a = p.pred + n * p.ps_n + c * p.ps_c;
    const float* b = p.tgt + n * p.ts_n + c * p.ts_c;
    const MaskT* mk = reinterpret_cast<const MaskT*>(p.mask) + n * p.ms_n;
    float* o = p.out + n * p.gs_n + c * p.gs_c;
    const float g = (p.gout ? p.gout[0] : 1.f) * p.scale;
    if (VEC) {
        const int wq = p.w >> 2, nq = p.h * wq;
        for (int q = threadIdx.x; q < nq; q += blockDim.x) {
            const int y = q / wq, x = (q - y * wq) << 2;
            const float4 u = *reinterpret_cast<const float4*>(a + y * p.ps_r + x);
            const float4 v = *reinterpret_cast<const float4*>(b + y * p.ts_r + x);
            float m[4];
            load_mask4(mk + y * p.ms_r + x, m);
            float4 r;
            r.x = (u.x - v.x) * (m[0] * g);
            r.y = (u.y - v.y) * (m[1] * g);
            r.z = (u.z - v.z) * (m[2] * g);
            r.w = (u.w - v.w) * (m[3] * g);
            *reinterpret_cast<float4*>(o + y * p.gs_r + x) = r;
        }
    } else {
        const int hw = p.h * p.w;
        for (int i = threadIdx.x; i < hw; i += blockDim.x) {
            const int y = i / p.w, x = i - y * p.w;
            o[y * p.gs_r + x] = (a[y * p.ps_r + x] - b[y * p.ts_r + x]) * ((float)mk[y * p.ms_r + x] * g);
        }
    }
}

inline bool aligned_to(const void* ptr, size_t bytes) { return (reinterpret_cast<uintptr_t>(ptr) % bytes) == 0; }
inline bool mult4(long long v) { return (v & 3) == 0; }

// ------------------------------------------------------------------------------------------
// AELoss (ae.py:40-89).  tag_ind [n, M, K, 2] = (flat index into the H*W plane, flag); the reference scatters the flag into a
// mask and works on [N, M, K, H, W] tensors, of which at most M*K entries per image are non-zero: this gathers those.
// Per person m:  k_m = sum_k f,  h_m = sum_{f != 0} t / (k_m + eps),  pull_m = sum_k ((h_m - t) f)^2 / (k_m + eps),
// valid_m = k_m > 0,  mc = sum valid;  pull = sum_m pull_m / (mc + eps);
// push = 0.5 (sum_{i,j} valid_i valid_j exp(-(h_i - h_j)^2) - mc) / (mc (mc - 1) + eps).  Everything behind the gather is fp64.
// An index outside [0, H*W) is treated as a flag of 0 (the reference's scatter has no defined result for it).
// ------------------------------------------------------------------------------------------
constexpr int kAeMaxPersons = 256;
constexpr double kAeEps = 0.01;

struct AeShared {
    double h[kAeMaxPersons];   // reference embedding
    double kn[kAeMaxPersons];  // k_m
    double d1[kAeMaxPersons];  // sum_k f^2 (h - t)
    double d2[kAeMaxPersons];  // sum_k (f (h - t))^2
    double red[4];
};

// one wave per person, lanes over the joints; ends with a barrier
__device__ void ae_person_stats(const float* __restrict__ tags, const int32_t* __restrict__ ind, int m, int k, int hw, AeShared& sh) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nwaves = blockDim.x >> 6;
    for (int p = wave; p < m; p += nwaves) {
        double s = 0.0, kn = 0.0;
        for (int j = lane; j < k; j += 64) {
            const int idx = ind[((size_t)p * k + j) * 2];
            float f = (float)ind[((size_t)p * k + j) * 2 + 1];
            if (idx < 0 || idx >= hw) f = 0.f;
            if (f != 0.f) s += (double)tags[(size_t)j * hw + idx];
            kn += (double)f;
        }
        s = wave_sum(s);
        kn = wave_sum(kn);
        const double h = s / (kn + kAeEps);
        double d1 = 0.0, d2 = 0.0;
        for (int j = lane; j < k; j += 64) {
            const int idx = ind[((size_t)p * k + j) * 2];
            float f = (float)ind[((size_t)p * k + j) * 2 + 1];
            if (idx < 0 || idx >= hw) f = 0.f;
            if (f != 0.f) {
                const double d = (h - (double)tags[(size_t)j * hw + idx]) * (double)f;
                d1 += d * (double)f;
                d2 += d * d;
            }
        }
        d1 = wave_sum(d1);
        d2 = wave_sum(d2);
        if (lane == 0) {
            sh.h[p] = h;
            sh.kn[p] = kn;
            sh.d1[p] = d1;
            sh.d2[p] = d2;
        }
    }
    __syncthreads();
}

// one workgroup per image -> partial[n] = (push_n, pull_n)
__global__ __launch_bounds__(256) void ae_fwd_kernel(const float* __restrict__ tags, long long tag_bs, const int32_t* __restrict__ ind,
                                                     double* __restrict__ partial, int m, int k, int hw) {
    __shared__ AeShared sh;
    const int n = blockIdx.x;
    ae_person_stats(tags + n * tag_bs, ind + (size_t)n * m * k * 2, m, k, hw, sh);
    double mc = 0.0, pull = 0.0, push = 0.0;
    for (int p = threadIdx.x; p < m; p += blockDim.x) {
        mc += sh.kn[p] > 0.0 ? 1.0 : 0.0;
        pull += sh.d2[p] / (sh.kn[p] + kAeEps);
    }
    for (int q = threadIdx.x; q < m * m; q += blockDim.x) {
        const int i = q / m, j = q - i * m;
        if (sh.kn[i] > 0.0 && sh.kn[j] > 0.0) {
            const double d = sh.h[i] - sh.h[j];
            push += exp(-(d * d));
        }
    }
    mc = block_sum_all(mc, sh.red);
    pull = block_sum_all(pull, sh.red);
    push = block_sum_all(push, sh.red);
    if (threadIdx.x == 0) {
        partial[2 * n + 0] = 0.5 * (push - mc) / (mc * (mc - 1.0) + kAeEps);
        partial[2 * n + 1] = pull / (mc + kAeEps);
    }
}

__global__ __launch_bounds__(256) void ae_final_kernel(const double* __restrict__ partial, float* __restrict__ out, int n) {
    __shared__ double red[4];
    double push = 0.0, pull = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        push += partial[2 * i + 0];
        pull += partial[2 * i + 1];
    }
    push = block_sum_all(push, red);
    pull = block_sum_all(pull, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(push / (double)n);
        out[1] = (float)(pull / (double)n);
    }
}

// One workgroup per (n, k) tag plane of the gradient: zero stores of the whole plane first, the per-person terms (recomputed per
// plane: at most M*K gathers and M*M exponentials) under them, then the indexed pixels behind a workgroup barrier.
//   d loss / d t_{m,k} = nz (A_m + B_m d1_m) / (k_m + eps) - B_m f^2 (h_m - t),   nz = (f != 0),
//   A_m = g_push / N * 0.5 / (mc (mc - 1) + eps) * valid_m * sum_j valid_j (-4) (h_m - h_j) exp(-(h_m - h_j)^2),
//   B_m = g_pull / N / (mc + eps) * 2 / (k_m + eps).
// Persons that share a pixel of this plane are summed by the lowest of them, in ascending m.
template <bool VEC>
__global__ __launch_bounds__(256) void ae_bwd_kernel(const float* __restrict__ tags, long long tag_bs, const int32_t* __restrict__ ind,
                                                     const float* __restrict__ gout, float* __restrict__ grad, long long grad_bs, int n_img,
                                                     int m, int k, int hw) {
    __shared__ AeShared sh;
    __shared__ double val[kAeMaxPersons];
    __shared__ int pix[kAeMaxPersons];
    const int n = blockIdx.x / k, kk = blockIdx.x - n * k;
    float* out = grad + n * grad_bs + (size_t)kk * hw;
    if (VEC) {
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = threadIdx.x; q < (hw >> 2); q += blockDim.x) reinterpret_cast<float4*>(out)[q] = z4;
    } else {
        for (int i = threadIdx.x; i < hw; i += blockDim.x) out[i] = 0.f;
    }
    const float* t_img = tags + n * tag_bs;
    const int32_t* i_img = ind + (size_t)n * m * k * 2;
    ae_person_stats(t_img, i_img, m, k, hw, sh);
    double mc = 0.0;
    for (int p = threadIdx.x; p < m; p += blockDim.x) mc += sh.kn[p] > 0.0 ? 1.0 : 0.0;
    mc = block_sum_all(mc, sh.red);
    const double inv_n = 1.0 / (double)n_img;
    const double c_push = (double)gout[0] * inv_n * 0.5 / (mc * (mc - 1.0) + kAeEps);
    const double c_pull = (double)gout[1] * inv_n / (mc + kAeEps);
    for (int p = threadIdx.x; p < m; p += blockDim.x) {
        const int idx = i_img[((size_t)p * k + kk) * 2];
        float f = (float)i_img[((size_t)p * k + kk) * 2 + 1];
        if (idx < 0 || idx >= hw) f = 0.f;
        double v = 0.0;
        if (f != 0.f) {
            const double hp = sh.h[p], kne = sh.kn[p] + kAeEps;
            double ds = 0.0;
            if (sh.kn[p] > 0.0) {
                for (int j = 0; j < m; ++j) {
                    if (sh.kn[j] > 0.0) {
                        const double d = hp - sh.h[j];
                        ds += -4.0 * d * exp(-(d * d));
                    }
                }
            }
            const double b = c_pull * 2.0 / kne;
            v = (c_push * ds + b * sh.d1[p]) / kne - b * ((double)f * (double)f) * (hp - (double)t_img[(size_t)kk * hw + idx]);
        }
        val[p] = v;
        pix[p] = f != 0.f ? idx : -1;
    }
    __syncthreads();  // the zero stores above are ordered before the stores below; val / pix are complete
    for (int p = threadIdx.x; p < m; p += blockDim.x) {
        const int idx = pix[p];
        if (idx < 0) continue;
        bool owner = true;
        for (int q = 0; q < p; ++q) owner = owner && pix[q] != idx;
        if (!owner) continue;
        double s = val[p];
        for (int q = p + 1; q < m; ++q)
            if (pix[q] == idx) s += val[q];
        out[idx] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------
// BottomUpGenerateTarget for a batch (bottomup_transform.py:527-598).  One workgroup per (n, stage, joint) plane of the padded
// target: the persons' windows go to LDS, then every pixel is computed once - the maximum over the persons whose window covers
// it, 0 elsewhere and in the padding - and stored once.  The exponent's argument is the reference's fp32 arithmetic operation by
// operation (numpy keeps fp32 scalars fp32 against Python numbers); the exponential is numpy's float32 one (numpy_expf below).
// ------------------------------------------------------------------------------------------
constexpr int kBuMaxStages = 8;
constexpr int kBuMaxPersons = 256;

struct BuTargetParams {
    const float* kp;    // [n, s, m, k, 3]
    const int* counts;  // [n]
    float* target;      // [n, s, k, hmax, wmax]
    int32_t* tag_ind;   // [n, s, max_num, k, 2] or [n, s, max_num, 2]
    int n, s, m, k, hmax, wmax, max_num, tpj;
    int sw[kBuMaxStages], sh[kBuMaxStages];
    double tmp_size;  // 3 sigma
    float c0;         // size // 2
    float den;        // 2 sigma^2
};

struct BuCentre {
    int mu_x, mu_y;
    bool vis;  // pt[2] > 0 and finite coordinates
};

__device__ __forceinline__ BuCentre bu_centre(const float* pt) {
    BuCentre c;
    const float px = pt[0], py = pt[1];
    c.vis = pt[2] > 0.f && px == px && py == py;
    // Python round() of a float32: half-to-even; the clamp only keeps the conversion defined, such centres are far outside
    c.mu_x = (int)rintf(fminf(fmaxf(px, -1.0e9f), 1.0e9f));
    c.mu_y = (int)rintf(fminf(fmaxf(py, -1.0e9f), 1.0e9f));
    return c;
}

// numpy's vectorised float32 exp (the AVX2 / AVX512F loop of numpy >= 1.17, which the reference's np.exp runs on an x86-64 host),
// operation by operation: n = rint(x log2(e)) by the 1.5 * 2^23 trick, Cody-Waite reduction r = fma(n, c2, fma(n, c1, x)), a (5, 2)
// rational minimax p(r) / q(r) in Horner form with fused multiply-adds, one IEEE division, scaling by 2^n.  It is up to 2 ulp off
// the correctly rounded value on about 39 % of arguments in [-36, 0], so only the same arithmetic reproduces the reference's
// targets; the constants are those of numpy's public sources (npy_math / loops_exponent_log).  x <= 0 here: no overflow branch.
__device__ __forceinline__ float numpy_expf(float x) {
#pragma clang fp contract(off)
    if (!(x >= -103.97208404541015625f)) return 0.f;
    float q = x * 1.442695040888963407359924681001892137f;
    q = (q + 12582912.0f) - 12582912.0f;
    float r = __builtin_fmaf(q, -6.93145752e-1f, x);
    r = __builtin_fmaf(q, -1.42860677e-6f, r);
    float num = __builtin_fmaf(5.082762527590693718096e-04f, r, 6.757896990527504603057e-03f);
    num = __builtin_fmaf(num, r, 5.114512081637298353406e-02f);
    num = __builtin_fmaf(num, r, 2.473615434895520810817e-01f);
    num = __builtin_fmaf(num, r, 7.257664613233124478488e-01f);
    num = __builtin_fmaf(num, r, 9.999999999980870924916e-01f);
    float den = __builtin_fmaf(2.159509375685829852307e-02f, r, -2.742335390411667452936e-01f);
    den = __builtin_fmaf(den, r, 1.0f);
    return ldexpf(num / den, (int)q);
}

template <int VEC>
__global__ __launch_bounds__(256) void bu_target_kernel(BuTargetParams p) {
#pragma clang fp contract(off)
    __shared__ int s_ulx[kBuMaxPersons], s_uly[kBuMaxPersons], s_brx[kBuMaxPersons], s_bry[kBuMaxPersons];
    __shared__ float s_x0p[kBuMaxPersons], s_y0p[kBuMaxPersons];
    __shared__ int s_tag[kBuMaxPersons];  // flat index of the centre, -1 = no tag
    const int kk = blockIdx.x % p.k;
    const int si = (blockIdx.x / p.k) % p.s;
    const int n = blockIdx.x / (p.k * p.s);
    const int W = p.sw[si], H = p.sh[si];
    int cnt = p.counts[n];
    cnt = max(0, min(cnt, min(p.m, min(p.max_num, kBuMaxPersons))));
    const float* kp_img = p.kp + ((size_t)n * p.s + si) * p.m * p.k * 3;
    for (int q = threadIdx.x; q < cnt; q += blockDim.x) {
        const float* pt = kp_img + ((size_t)q * p.k + kk) * 3;
        const BuCentre c = bu_centre(pt);
        const int ulx = (int)((double)c.mu_x - p.tmp_size), uly = (int)((double)c.mu_y - p.tmp_size);
        const int brx = (int)((double)c.mu_x + p.tmp_size + 1.0), bry = (int)((double)c.mu_y + p.tmp_size + 1.0);
        const bool stamp = c.vis && !(ulx >= W || uly >= H || brx < 0 || bry < 0);
        s_ulx[q] = stamp ? ulx : 0x3fffffff;  // an empty column range: the person covers nothing
        s_brx[q] = stamp ? brx : -0x3fffffff;
        s_uly[q] = uly;
        s_bry[q] = bry;
        s_x0p[q] = (p.c0 + pt[0]) - (float)c.mu_x;
        s_y0p[q] = (p.c0 + pt[1]) - (float)c.mu_y;
        s_tag[q] = (c.vis && c.mu_x >= 0 && c.mu_x < W && c.mu_y >= 0 && c.mu_y < H) ? c.mu_y * W + c.mu_x : -1;
    }
    __syncthreads();

    float* out = p.target + (size_t)blockIdx.x * p.hmax * p.wmax;
    const int wq = p.wmax / VEC, nq = p.hmax * wq;
    for (int q = threadIdx.x; q < nq; q += blockDim.x) {
        const int y = q / wq, x0 = (q - y * wq) * VEC;
        float v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = 0.f;
        if (y < H && x0 < W) {
            for (int j = 0; j < cnt; ++j) {
                const int ulx = s_ulx[j], brx = s_brx[j], uly = s_uly[j];
                if (y < uly || y >= s_bry[j] || x0 + VEC <= ulx || x0 >= brx) continue;
                const float dy = (float)(y - uly) - s_y0p[j];
                const float dy2 = dy * dy;
                const float x0p = s_x0p[j];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int x = x0 + e;
                    if (x < ulx || x >= brx || x >= W) continue;
                    const float dx = (float)(x - ulx) - x0p;
                    const float dx2 = dx * dx;
                    const float arg = -(dx2 + dy2) / p.den;
                    v[e] = fmaxf(v[e], numpy_expf(arg));
                }
            }
        }
        if (VEC == 4) {
            *reinterpret_cast<float4*>(out + (size_t)y * p.wmax + x0) = make_float4(v[0], v[VEC > 1 ? 1 : 0], v[VEC > 2 ? 2 : 0], v[VEC > 3 ? 3 : 0]);
        } else {
            out[(size_t)y * p.wmax + x0] = v[0];
        }
    }

    if (p.tpj) {
        int32_t* ti = p.tag_ind + ((size_t)n * p.s + si) * p.max_num * p.k * 2;
        for (int q = threadIdx.x; q < p.max_num; q += blockDim.x) {
            const int tag = q < cnt ? s_tag[q] : -1;
            ti[((size_t)q * p.k + kk) * 2 + 0] = tag >= 0 ? tag : 0;
            ti[((size_t)q * p.k + kk) * 2 + 1] = tag >= 0 ? 1 : 0;
        }
    } else if (kk == 0) {  // one entry per person: the last visible joint whose centre is inside the map wins
        int32_t* ti = p.tag_ind + ((size_t)n * p.s + si) * p.max_num * 2;
        for (int q = threadIdx.x; q < p.max_num; q += blockDim.x) {
            int tag = -1;
            if (q < cnt) {
                for (int j = 0; j < p.k; ++j) {
                    const BuCentre c = bu_centre(kp_img + ((size_t)q * p.k + j) * 3);
                    if (c.vis && c.mu_x >= 0 && c.mu_x < W && c.mu_y >= 0 && c.mu_y < H) tag = c.mu_y * W + c.mu_x;
                }
            }
            ti[(size_t)q * 2 + 0] = tag >= 0 ? tag : 0;
            ti[(size_t)q * 2 + 1] = tag >= 0 ? 1 : 0;
        }
    }
}

int validate_mse_mask(const float* pred, const float* target, const void* mask, const void* out, int n, int k, int h, int w,
                      const long long* strides, int n_strides) {
    if (!pred || !target || !mask || !out) return MP_ERR_NULL;
    if (n <= 0 || k <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    if ((long long)n * k > 0x7fffffffLL || (long long)h * w > 0x7fffffffLL) return MP_ERR_SHAPE;
    for (int i = 0; i < n_strides; ++i)
        if (strides[i] < 0) return MP_ERR_SHAPE;
    return MP_OK;
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_joints_mse_mask_workspace_bytes(int n, int k) {
    if (n <= 0 || k <= 0) return 0;
    return ((size_t)n * k * sizeof(float) + 255) & ~(size_t)255;
}

int mp_joints_mse_mask_fwd(const float* pred, long long pred_sn, long long pred_sc, long long pred_sr, const float* target,
                           long long target_sn, long long target_sc, long long target_sr, const void* mask, int mask_is_u8,
                           long long mask_sn, long long mask_sr, float* loss, void* workspace, size_t workspace_bytes, int n, int k,
                           int h, int w, mp_stream_t stream) {
    const long long st[8] = {pred_sn, pred_sc, pred_sr, target_sn, target_sc, target_sr, mask_sn, mask_sr};
    int rc = validate_mse_mask(pred, target, mask, loss, n, k, h, w, st, 8);
    if (rc != MP_OK) return rc;
    if (pred_sr < w || target_sr < w || mask_sr < w) return MP_ERR_SHAPE;
    if (!workspace || workspace_bytes < mp_joints_mse_mask_workspace_bytes(n, k)) return MP_ERR_WORKSPACE;
    MseMaskParams p{};
    p.pred = pred; p.tgt = target; p.mask = mask; p.out = reinterpret_cast<float*>(workspace);
    p.ps_n = pred_sn; p.ps_c = pred_sc; p.ps_r = pred_sr; p.ts_n = target_sn; p.ts_c = target_sc; p.ts_r = target_sr;
    p.ms_n = mask_sn; p.ms_r = mask_sr; p.k = k; p.h = h; p.w = w;
    const size_t mb = mask_is_u8 ? 4 : 16;
    const bool vec = (w & 3) == 0 && aligned_to(pred, 16) && aligned_to(target, 16) && aligned_to(mask, mb) && mult4(pred_sn) &&
                     mult4(pred_sc) && mult4(pred_sr) && mult4(target_sn) && mult4(target_sc) && mult4(target_sr) && mult4(mask_sn) &&
                     mult4(mask_sr);
    const dim3 grid(n * k), block(256);
    hipStream_t s = as_stream(stream);
    if (mask_is_u8) {
        if (vec) hipLaunchKernelGGL((mse_mask_fwd_kernel<uint8_t, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((mse_mask_fwd_kernel<uint8_t, false>), grid, block, 0, s, p);
    } else {
        if (vec) hipLaunchKernelGGL((mse_mask_fwd_kernel<float, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((mse_mask_fwd_kernel<float, false>), grid, block, 0, s, p);
    }
    rc = check_launch();
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(mse_mask_final_kernel, dim3(1), dim3(256), 0, s, p.out, loss, n * k,
                       1.0 / ((double)n * k * (double)h * (double)w));
    return check_launch();
}

int mp_joints_mse_mask_bwd(const float* pred, long long pred_sn, long long pred_sc, long long pred_sr, const float* target,
                           long long target_sn, long long target_sc, long long target_sr, const void* mask, int mask_is_u8,
                           long long mask_sn, long long mask_sr, const float* grad_out, float* grad_pred, long long grad_sn,
                           long long grad_sc, long long grad_sr, int n, int k, int h, int w, mp_stream_t stream) {
    const long long st[11] = {pred_sn, pred_sc, pred_sr, target_sn, target_sc, target_sr, mask_sn, mask_sr, grad_sn, grad_sc, grad_sr};
    int rc = validate_mse_mask(pred, target, mask, grad_pred, n, k, h, w, st, 11);
    if (rc != MP_OK) return rc;
    if (pred_sr < w || target_sr < w || mask_sr < w || grad_sr < w) return MP_ERR_SHAPE;
    // the gradient is written through its strides: planes and images must not overlap
    if (grad_sc < grad_sr * (long long)h || grad_sn < grad_sc * (long long)k) return MP_ERR_SHAPE;
    MseMaskParams p{};
    p.pred = pred; p.tgt = target; p.mask = mask; p.gout = grad_out; p.out = grad_pred;
    p.ps_n = pred_sn; p.ps_c = pred_sc; p.ps_r = pred_sr; p.ts_n = target_sn; p.ts_c = target_sc; p.ts_r = target_sr;
    p.ms_n = mask_sn; p.ms_r = mask_sr; p.gs_n = grad_sn; p.gs_c = grad_sc; p.gs_r = grad_sr; p.k = k; p.h = h; p.w = w;
    p.scale = (float)(2.0 / ((double)n * k * (double)h * (double)w));
    const size_t mb = mask_is_u8 ? 4 : 16;
    const bool vec = (w & 3) == 0 && aligned_to(pred, 16) && aligned_to(target, 16) && aligned_to(mask, mb) && aligned_to(grad_pred, 16) &&
                     mult4(pred_sn) && mult4(pred_sc) && mult4(pred_sr) && mult4(target_sn) && mult4(target_sc) && mult4(target_sr) &&
                     mult4(mask_sn) && mult4(mask_sr) && mult4(grad_sn) && mult4(grad_sc) && mult4(grad_sr);
    const dim3 grid(n * k), block(256);
    hipStream_t s = as_stream(stream);
    if (mask_is_u8) {
        if (vec) hipLaunchKernelGGL((mse_mask_bwd_kernel<uint8_t, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((mse_mask_bwd_kernel<uint8_t, false>), grid, block, 0, s, p);
    } else {
        if (vec) hipLaunchKernelGGL((mse_mask_bwd_kernel<float, true>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((mse_mask_bwd_kernel<float, false>), grid, block, 0, s, p);
    }
    return check_launch();
}

size_t mp_ae_loss_workspace_bytes(int n) {
    if (n <= 0) return 0;
    return ((size_t)n * 2 * sizeof(double) + 255) & ~(size_t)255;
}

static int validate_ae(const float* tags, const int32_t* tag_ind, const void* a, const void* b, long long tag_bs, int n, int m, int k,
                       int hw) {
    if (!tags || !tag_ind || !a || !b) return MP_ERR_NULL;
    if (n <= 0 || m <= 0 || k <= 0 || hw <= 0) return MP_ERR_SHAPE;
    if ((long long)k * hw > 0x7fffffffLL || (long long)n * k > 0x7fffffffLL) return MP_ERR_SHAPE;
    if (tag_bs < (long long)k * hw) return MP_ERR_SHAPE;
    if (m > kAeMaxPersons) return MP_ERR_UNSUPPORTED;
    return MP_OK;
}

int mp_ae_loss_fwd(const float* tags, long long tag_batch_stride, const int32_t* tag_ind, float* loss2, void* workspace,
                   size_t workspace_bytes, int n, int m, int k, int hw, mp_stream_t stream) {
    int rc = validate_ae(tags, tag_ind, loss2, loss2, tag_batch_stride, n, m, k, hw);
    if (rc != MP_OK) return rc;
    if (!workspace || workspace_bytes < mp_ae_loss_workspace_bytes(n)) return MP_ERR_WORKSPACE;
    double* partial = reinterpret_cast<double*>(workspace);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ae_fwd_kernel, dim3(n), dim3(256), 0, s, tags, tag_batch_stride, tag_ind, partial, m, k, hw);
    rc = check_launch();
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(ae_final_kernel, dim3(1), dim3(256), 0, s, partial, loss2, n);
    return check_launch();
}

int mp_ae_loss_bwd(const float* tags, long long tag_batch_stride, const int32_t* tag_ind, const float* grad_out2, float* grad_tags,
                   long long grad_batch_stride, int n, int m, int k, int hw, mp_stream_t stream) {
    int rc = validate_ae(tags, tag_ind, grad_out2, grad_tags, tag_batch_stride, n, m, k, hw);
    if (rc != MP_OK) return rc;
    if (grad_batch_stride < (long long)k * hw) return MP_ERR_SHAPE;
    const bool vec = (hw & 3) == 0 && aligned_to(grad_tags, 16) && mult4(grad_batch_stride);
    hipStream_t s = as_stream(stream);
    if (vec)
        hipLaunchKernelGGL(ae_bwd_kernel<true>, dim3(n * k), dim3(256), 0, s, tags, tag_batch_stride, tag_ind, grad_out2, grad_tags,
                           grad_batch_stride, n, m, k, hw);
    else
        hipLaunchKernelGGL(ae_bwd_kernel<false>, dim3(n * k), dim3(256), 0, s, tags, tag_batch_stride, tag_ind, grad_out2, grad_tags,
                           grad_batch_stride, n, m, k, hw);
    return check_launch();
}

int mp_bottomup_target(const float* keypoints, const int* counts, const int* stage_wh_host, float* target, int32_t* tag_ind, int n,
                       int s, int m, int k, int hmax, int wmax, int max_num, int tag_per_joint, double sigma, mp_stream_t stream) {
    if (!keypoints || !counts || !stage_wh_host || !target || !tag_ind) return MP_ERR_NULL;
    if (n <= 0 || s <= 0 || m <= 0 || k <= 0 || hmax <= 0 || wmax <= 0 || max_num <= 0) return MP_ERR_SHAPE;
    if (!(sigma > 0.0)) return MP_ERR_SHAPE;
    if ((long long)hmax * wmax > 0x7fffffffLL || (long long)n * s * k > 0x7fffffffLL) return MP_ERR_SHAPE;
    for (int i = 0; i < s && i < kBuMaxStages; ++i) {
        const int w = stage_wh_host[2 * i], h = stage_wh_host[2 * i + 1];
        if (w <= 0 || h <= 0 || w > wmax || h > hmax) return MP_ERR_SHAPE;
    }
    const double tmp = sigma * 3.0;
    // the reference's patch (arange(0, 6 sigma + 1)) and its window (int(mu -+ 3 sigma)) agree only for a whole 3 sigma
    if (s > kBuMaxStages || m > kBuMaxPersons || max_num > kBuMaxPersons || tmp != (double)(long long)tmp || tmp > 1.0e6)
        return MP_ERR_UNSUPPORTED;
    BuTargetParams p{};
    p.kp = keypoints; p.counts = counts; p.target = target; p.tag_ind = tag_ind;
    p.n = n; p.s = s; p.m = m; p.k = k; p.hmax = hmax; p.wmax = wmax; p.max_num = max_num; p.tpj = tag_per_joint ? 1 : 0;
    for (int i = 0; i < s; ++i) {
        p.sw[i] = stage_wh_host[2 * i];
        p.sh[i] = stage_wh_host[2 * i + 1];
    }
    p.tmp_size = tmp;
    p.c0 = (float)(double)(long long)((2.0 * tmp + 1.0) / 2.0);  // size // 2
    p.den = (float)(2.0 * (sigma * sigma));
    const dim3 grid(n * s * k), block(256);
    if ((wmax & 3) == 0 && aligned_to(target, 16))
        hipLaunchKernelGGL(bu_target_kernel<4>, grid, block, 0, as_stream(stream), p);
    else
        hipLaunchKernelGGL(bu_target_kernel<1>, grid, block, 0, as_stream(stream), p);
    return check_launch();
}

}  // extern "C"
