// The fp32 element-wise plan ops: the stem's max-pool, the exchange unit's up-sampling sum.  No fp multiply: contraction is moot.
#include "common.h"

#include <math.h>

namespace mp {

// nn.MaxPool2d(3, 2, pad_mode="same") resnet.py:190: out = ceil(in/2); pad only bottom/right (even H, W).
__global__ __launch_bounds__(256) void maxpool3x3s2_same_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                int planes, int h, int w, int oh, int ow, int pt,
                                                                int pl) {
    const size_t total = (size_t)planes * oh * ow;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int ox = (int)(i % ow);
        size_t t = i / ow;
        int oy = (int)(t % oh);
        size_t pl_i = t / oh;
        const float* src = x + pl_i * (size_t)h * w;
        float m = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            int yy = oy * 2 - pt + dy;
            if (yy < 0 || yy >= h) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                int xx = ox * 2 - pl + dx;
                if (xx < 0 || xx >= w) continue;
                m = fmaxf(m, src[yy * w + xx]);
            }
        }
        out[i] = m;
    }
}

// HRModule exchange unit, up-sampling side: out = act(((base + up(t1)) + up(t2)) + up(t3)), nearest up-sampling by
// s_k = 1 << sh_k.  One thread per 4 output columns (16 B loads/stores of base/out); a low-resolution term
// contributes one value per s_k columns, served from L2 (each low-res row is re-read by s_k output rows).
struct FuseSumParams {
    const float* base;
    const float* t[3];
    float* out;
    int sh[3];  // log2(scale), -1 = absent
    int n_planes, h, w, relu;
};

__global__ __launch_bounds__(256) void fuse_sum_scalar_kernel(FuseSumParams p) {
    const size_t total = (size_t)p.n_planes * p.h * p.w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % p.w);
        const size_t r = i / p.w;
        const int y = (int)(r % p.h);
        const size_t plane = r / p.h;
        float v = p.base[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (p.sh[k] < 0) continue;
            const int sh = p.sh[k];
            v += p.t[k][(plane * (p.h >> sh) + (y >> sh)) * (p.w >> sh) + (x >> sh)];
        }
        if (p.relu) v = fmaxf(v, 0.f);
        p.out[i] = v;
    }
}

__global__ __launch_bounds__(256) void fuse_sum_kernel(FuseSumParams p) {
    const int wq = p.w >> 2;
    const size_t total = (size_t)p.n_planes * p.h * wq;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xq = (int)(i % wq);
        const size_t r = i / wq;
        const int y = (int)(r % p.h);
        const size_t plane = r / p.h;
        const size_t o = (plane * p.h + y) * p.w + (size_t)xq * 4;
        float4 v = *reinterpret_cast<const float4*>(p.base + o);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (p.sh[k] < 0) continue;
            const int sh = p.sh[k];
            const int lw = p.w >> sh, lh = p.h >> sh;
            const float* row = p.t[k] + (plane * lh + (y >> sh)) * lw;
            const int x0 = xq * 4;
            v.x += row[(x0 + 0) >> sh];
            v.y += row[(x0 + 1) >> sh];
            v.z += row[(x0 + 2) >> sh];
            v.w += row[(x0 + 3) >> sh];
        }
        if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        *reinterpret_cast<float4*>(p.out + o) = v;
    }
}

static int log2_exact(int v) {
    for (int i = 0; i < 16; ++i)
        if ((1 << i) == v) return i;
    return -1;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_fuse_upsample_sum(const float* base, const float* t1, int s1, const float* t2, int s2, const float* t3, int s3,
                         float* out, int n, int c, int h, int w, int relu, mp_stream_t stream) {
    if (!base || !t1 || !out) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    FuseSumParams p{};
    p.base = base; p.out = out; p.n_planes = n * c; p.h = h; p.w = w; p.relu = relu ? 1 : 0;
    const float* ts[3] = {t1, t2, t3};
    const int ss[3] = {s1, s2, s3};
    for (int k = 0; k < 3; ++k) {
        p.t[k] = ts[k];
        p.sh[k] = -1;
        if (!ts[k]) continue;
        const int sh = log2_exact(ss[k]);
        if (sh < 0 || (h % ss[k]) || (w % ss[k])) return MP_ERR_UNSUPPORTED;
        p.sh[k] = sh;
    }
    const bool vec = (w & 3) == 0;
    const size_t total = vec ? (size_t)n * c * h * (w >> 2) : (size_t)n * c * h * w;
    size_t blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (vec) hipLaunchKernelGGL(fuse_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), p);
    else hipLaunchKernelGGL(fuse_sum_scalar_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), p);
    return check_launch();
}

int mp_maxpool3x3s2_same(const float* x, float* out, int n, int c, int h, int w, mp_stream_t stream) {
    if (!x || !out) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    const int oh = (h + 1) / 2, ow = (w + 1) / 2;
    const int ph = max((oh - 1) * 2 + 3 - h, 0), pw = max((ow - 1) * 2 + 3 - w, 0);
    const size_t total = (size_t)n * c * oh * ow;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(maxpool3x3s2_same_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), x, out, n * c, h, w, oh,
                       ow, ph / 2, pw / 2);
    return check_launch();
}

}  // extern "C"
