// What the fp32 (conv_wgrad.hip) and the fp16 (wgrad_f16.hip) weight-gradient kernels share: descriptor acceptance, the slab
// reduce (kernels and launch live in conv_wgrad.hip, one copy in the library; the fp32 entry keeps a plain kernel of its own beside
// them, see there) and the launch-words writer.
#pragma once
#include "common.h"
#include "conv_f16_dev.h"

namespace mp {

// 1x1 / 3x3 with padding k/2, or the 4x4 stride-2 padding-1 form (the transposed convolution's weight gradient, roles of input and
// output gradient exchanged by the caller)
inline int wgrad_desc_ok(const mp_conv_desc* d) {
    if (!d) return MP_ERR_NULL;
    if (d->n <= 0 || d->cin <= 0 || d->cout <= 0 || d->h <= 0 || d->w <= 0 || d->conv_h <= 0 || d->conv_w <= 0) return MP_ERR_SHAPE;
    if (d->kh != d->kw || !(d->kh == 1 || d->kh == 3 || d->kh == 4)) return MP_ERR_UNSUPPORTED;
    if (!(d->stride == 1 || d->stride == 2)) return MP_ERR_UNSUPPORTED;
    if (d->pad_top != d->pad_left) return MP_ERR_UNSUPPORTED;
    if (d->kh == 4 ? (d->stride != 2 || d->pad_top != 1) : (d->pad_top != d->kh / 2)) return MP_ERR_UNSUPPORTED;
    return MP_OK;
}

// floats of dW = of one slab; the workspace holds jobs x splits slabs
inline size_t wgrad_count(const mp_conv_desc* d) { return (size_t)d->cout * d->cin * d->kh * d->kw; }

constexpr int kWgradJobs = 8;
struct WgradDst {  // destinations of a reduce: blockIdx.y = job
    float* dw[kWgradJobs];
};

// The slab reduce a launch takes: G threads per element (0 = the plain kernel), workgroups per job.  <= 18 K weights (32-channel
// 3x3) under many slabs: 16 threads per element; <= 74 K weights (64-channel 3x3, the 1x1 convs): 4 per element.
struct WgradReduce {
    int G;
    unsigned blocks;
};
inline WgradReduce wgrad_reduce_choice(size_t count, int splits) {
    if (count <= 18432 && splits >= 64) return {16, (unsigned)((count + 15) / 16)};
    if (count <= 73728 && splits >= 16) return {4, (unsigned)((count + 63) / 64)};
    const size_t blocks = (count + 255) / 256;
    return {0, (unsigned)(blocks > 4096 ? 4096 : blocks)};
}
// dst.dw[j] (+)= scale * the fixed-order sum of the `splits` slabs of job j, slabs = [jobs][splits][count]
int wgrad_reduce_launch(const float* slabs, const WgradDst& dst, int jobs, size_t count, int splits, float scale, int accumulate,
                        hipStream_t s);

// mp_conv_wgrad_launch_words: the return code, and the body after an accepted geometry
inline int wgrad_words_out(int64_t* out, int cap, int rc, std::initializer_list<int64_t> body) {
    const int n = 1 + (rc == MP_OK ? (int)body.size() : 0);
    if (cap < n) return MP_ERR_WORKSPACE;
    int i = 0;
    out[i++] = rc;
    if (rc == MP_OK)
        for (int64_t v : body) out[i++] = v;
    return n;
}
int wgrad16_launch_words(const mp_conv_desc* desc, int n_jobs, int64_t* out, int cap);  // wgrad_f16.hip

}  // namespace mp
