// Loader-side pixel kernels: each reads HWC uint8 sources and writes what the network or the loss takes in one pass.
// The interpolations restate OpenCV's 8-bit fixed-point paths [cv2-knowledge, PARITY UNPINNED: cv2 is not installed here].  They are
// spelled out here once; each is ONE set of device functions below, shared by every kernel that needs it.
//   warp, both modes (cv::warpAffine without WARP_INVERSE_MAP, BORDER_CONSTANT 0): the 2x3 matrix is inverted in double
//     (invert_affine); destination (x, y) maps through AB_BITS = 10 fixed point, the per-row and per-column terms rounded separately
//     with cvRound: X = cvRound((i01 y + i02) 1024) + round_delta + cvRound(i00 x 1024), likewise Y (row_terms + the column term).
//   INTER_LINEAR (sample_linear): round_delta 16, X >> 5 is the coordinate in 1/32 pixel (INTER_BITS = 5), its integer part
//     saturate_cast<short>; the four bilinear weights are the exact products (32-fx)(32-fy)*32 ... of the 15-bit table, the result is
//     (sum + 2^14) >> 15.
//   INTER_NEAREST (augment_mask_group): round_delta 512, X >> 10, saturate_cast<short>; the source pixel when it lies inside.
//   resize, INTER_LINEAR (resize_term + resize_pad_normalize_kernel): scale = src / dst in double; f = (float)((d + 0.5) * scale -
//     0.5), s = floor(f), f -= s; s < 0 -> (0, 0), s >= src - 1 -> (src - 1, 0); coefficients saturate_cast<short>((1 - f) * 2048),
//     saturate_cast<short>(f * 2048) (INTER_RESIZE_COEF_BITS = 11); horizontal pass int32 S[sx] * a0 + S[sx + 1] * a1; vertical pass
//     (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, saturated to 0..255.
// Everything up to the normalise is integer arithmetic on those terms, so no result depends on the thread mapping.
#include "common.h"

#pragma clang fp contract(off)  // the rounding points of the coordinate arithmetic are part of the result

namespace mp {
namespace {

__device__ __forceinline__ int cv_round(double v) { return (int)rint(v); }  // cvRound: nearest, ties to even

__device__ __forceinline__ int saturate_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

__device__ __forceinline__ void invert_affine(const double* M, double inv[6]) {
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0.0 ? 1.0 / D : 0.0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    const double i0 = A11, i1 = M[1] * (-D), i3 = M[3] * (-D), i4 = A22;
    inv[0] = i0; inv[1] = i1; inv[3] = i3; inv[4] = i4;
    inv[2] = -i0 * M[2] - i1 * M[5];
    inv[5] = -i3 * M[2] - i4 * M[5];
}

// the fixed-point terms of destination row y
__device__ __forceinline__ void row_terms(const double* inv, int y, int round_delta, int& X0, int& Y0) {
    X0 = cv_round((inv[1] * y + inv[2]) * 1024.0) + round_delta;
    Y0 = cv_round((inv[4] * y + inv[5]) * 1024.0) + round_delta;
}

// The INTER_LINEAR sample of destination column x of the row whose terms are (X0, Y0): v[c] in 0..255.  mirror_src reads the source
// at the mirrored column - cv2.flip(image, 1) BEFORE the warp; the coordinates and weights do not change, so it is bit-identical
// to warping a flipped copy.
__device__ __forceinline__ void sample_linear(const double* inv, const uint8_t* __restrict__ img, int H, int W, bool mirror_src, int X0,
                                              int Y0, int x, int v[3]) {
    const int X = (X0 + cv_round(inv[0] * x * 1024.0)) >> 5, Y = (Y0 + cv_round(inv[3] * x * 1024.0)) >> 5;
    const int sx = saturate_short(X >> 5), sy = saturate_short(Y >> 5);
    const int fx = X & 31, fy = Y & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    int acc[3] = {0, 0, 0};
    auto tap = [&](int yy, int xx, int w) {
        if (w != 0 && yy >= 0 && yy < H && xx >= 0 && xx < W) {
            const uint8_t* px = img + ((size_t)yy * W + (mirror_src ? W - 1 - xx : xx)) * 3;
            acc[0] += w * px[0]; acc[1] += w * px[1]; acc[2] += w * px[2];
        }
    };
    tap(sy, sx, w00); tap(sy, sx + 1, w01); tap(sy + 1, sx, w10); tap(sy + 1, sx + 1, w11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = (acc[c] + (1 << 14)) >> 15;
        v[c] = v[c] > 255 ? 255 : v[c];
    }
}

struct NormConst { float m[3], s[3]; };  // vision.Normalize: mean and std of the 0..255 range

// false for a zero std (MP_ERR_SHAPE at every entry point)
inline bool fill_norm(const float mean[3], const float stddev[3], NormConst& nc) {
    for (int c = 0; c < 3; ++c) { nc.m[c] = mean[c]; nc.s[c] = stddev[c]; }
    return stddev[0] != 0.f && stddev[1] != 0.f && stddev[2] != 0.f;
}

// Normalize + HWC2CHW of VEC adjacent pixels u[e][c]: (u - mean) / std, a true division, into the three planes that start at o -
// one 16-byte store per plane for VEC == 4, a scalar store otherwise
template <int VEC>
__device__ __forceinline__ void normalize_store(const NormConst& nc, const int (&u)[VEC][3], float* __restrict__ o, size_t plane) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float f[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] = ((float)u[e][c] - nc.m[c]) / nc.s[c];
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(o + c * plane) = make_float4(f[0], f[1], f[2], f[3]);
        else o[c * plane] = f[0];
    }
}

// four adjacent pixels per thread leave by one store of 4 * elem_bytes: the row width and the base address must allow it
inline bool wide_stores(int width, const void* base, size_t elem_bytes) {
    return width % 4 == 0 && (uintptr_t)base % (4 * elem_bytes) == 0;
}

// ---- cv2.warpAffine(image, trans, (w, h), flags=INTER_LINEAR) (topdown_transform.py:211-216 / :249-254), with NORMALIZE fused with
// vision.Normalize(mean*255, std*255) + vision.HWC2CHW() (data_factory.py:129-133): one thread per destination pixel reads <= 4
// source pixels and writes three fp32 planes, or the warped uint8 HWC pixel when only the warp is wanted.
template <bool NORMALIZE>
__global__ __launch_bounds__(256) void warp_affine_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ src_off,
                                                          const int* __restrict__ src_hw, const int* __restrict__ flip,
                                                          const double* __restrict__ trans, void* __restrict__ out, int out_h, int out_w,
                                                          NormConst nc) {
    const int n = blockIdx.y;
    __shared__ double inv[6];
    if (threadIdx.x == 0) invert_affine(trans + (size_t)n * 6, inv);
    __syncthreads();
    const int H = src_hw[2 * n], W = src_hw[2 * n + 1];
    const bool mirror = flip && flip[n] != 0;  // TopDownHorizontalRandomFlip: the flip precedes the warp
    const uint8_t* __restrict__ img = src + src_off[n];
    const int total = out_h * out_w;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int y = i / out_w, x = i - y * out_w;
        int X0, Y0, v[1][3];
        row_terms(inv, y, 16, X0, Y0);
        sample_linear(inv, img, H, W, mirror, X0, Y0, x, v[0]);
        if constexpr (NORMALIZE) {
            normalize_store<1>(nc, v, reinterpret_cast<float*>(out) + (size_t)n * 3 * total + i, total);
        } else {
            uint8_t* o = reinterpret_cast<uint8_t*>(out) + ((size_t)n * total + i) * 3;
            o[0] = (uint8_t)v[0][0]; o[1] = (uint8_t)v[0][1]; o[2] = (uint8_t)v[0][2];
        }
    }
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" int mp_warp_affine(const uint8_t* src, const long long* src_offsets, const int* src_hw, const int* flip,
                              const double* trans, void* out, int n, int out_h, int out_w, int normalize, const float mean[3], const float stddev[3],
                              mp_stream_t stream) {
    if (!src || !src_offsets || !src_hw || !trans || !out) return MP_ERR_NULL;
    if (n <= 0 || out_h <= 0 || out_w <= 0 || n > 65535) return MP_ERR_SHAPE;
    if (normalize && (!mean || !stddev)) return MP_ERR_NULL;
    NormConst nc{};
    if (normalize && !fill_norm(mean, stddev, nc)) return MP_ERR_SHAPE;
    const int total = out_h * out_w;
    int bx = (total + 255) / 256;
    if (bx > 1024) bx = 1024;
    const auto kernel = normalize ? warp_affine_kernel<true> : warp_affine_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(bx, n), dim3(256), 0, as_stream(stream), src, src_offsets, src_hw, flip, trans, out, out_h, out_w, nc);
    return check_launch();
}

// ---- horizontal flip of an NCHW fp32 batch: the second run of the flip test (topdown_inferencer.py:168-170, ops.ReverseV2 on
// the width axis).  out[n, c, y, x] = in[n, c, y, W - 1 - x]; one pass, written straight into the network's input buffer (the
// host mirror used torch.flip + a copy: two passes through PyTorch kernels).  in and out must not overlap.
namespace mp {
namespace {
__global__ __launch_bounds__(256) void flip_width_kernel(const float* __restrict__ in, float* __restrict__ out, size_t rows, int w) {
    // one thread per output element quad where W % 4 == 0 (16-byte stores, reversed 16-byte loads), else per element
    const size_t total = rows * (size_t)w;
    if ((w & 3) == 0) {
        const size_t quads = total >> 2;
        const int wq = w >> 2;
        for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
            const size_t row = q / wq;
            const int xq = (int)(q - row * wq);
            const float4 v = *reinterpret_cast<const float4*>(in + row * w + (size_t)(wq - 1 - xq) * 4);
            *reinterpret_cast<float4*>(out + q * 4) = make_float4(v.w, v.z, v.y, v.x);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
            const size_t row = i / w;
            const int x = (int)(i - row * w);
            out[i] = in[row * w + (w - 1 - x)];
        }
    }
}
}  // namespace
}  // namespace mp

extern "C" int mp_flip_width(const float* in, float* out, int n, int c, int h, int w, mp_stream_t stream) {
    if (!in || !out) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    if (in == out) return MP_ERR_UNSUPPORTED;
    const size_t rows = (size_t)n * c * h;
    const size_t work = (w & 3) == 0 ? rows * (size_t)w / 4 : rows * (size_t)w;
    size_t blocks = (work + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(mp::flip_width_kernel, dim3((unsigned)blocks), dim3(256), 0, mp::as_stream(stream), in, out, rows, w);
    return mp::check_launch();
}

// ---- bottom-up evaluation input: BottomUpRescale + BottomUpPad + Normalize + HWC2CHW in one pass (bottomup_transform.py:143-208,
// :601-645, data_factory.py:129-133).  cv2.resize(image, (tw, th), INTER_LINEAR) on uint8 HWC, zero pad on the right and bottom to
// (PH, PW), written as three fp32 planes; the mask (1 inside the resized image) leaves by the same launch.
// The pad happens on the uint8 image, BEFORE Normalize: a padded pixel is (0 - mean) / std, not 0.
namespace mp {
namespace {

constexpr int kRpnMaxImages = 32;  // (tw, th) of every image of a launch travel in the kernel arguments

struct RpnParams {
    const uint8_t* src;
    const long long* src_off;
    const int* src_hw;
    float* out;     // [n, 3, PH, PW]
    uint8_t* mask;  // [n, PH, PW]
    int ph, pw;
    NormConst norm;
    int twh[kRpnMaxImages][2];
};

// source index and the two 11-bit coefficients of destination coordinate d (either axis)
__device__ __forceinline__ void resize_term(int d, double scale, int src_size, int& s, int& c0, int& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src_size - 1) { s = src_size - 1; f = 0.f; }
    const float a0 = rintf((1.f - f) * 2048.f), a1 = rintf(f * 2048.f);  // saturate_cast<short>: cvRound, then the short range
    c0 = (int)fminf(fmaxf(a0, -32768.f), 32767.f);
    c1 = (int)fminf(fmaxf(a1, -32768.f), 32767.f);
}

// VEC adjacent destination pixels of one row per thread: VEC = 4 writes each plane with one 16-byte store and the mask with one
// 4-byte store (PW % 4 == 0), VEC = 1 is the scalar form for any other width
template <int VEC>
__global__ __launch_bounds__(256) void resize_pad_normalize_kernel(RpnParams p) {
    const int n = blockIdx.z, y = blockIdx.y;
    const int H = p.src_hw[2 * n], W = p.src_hw[2 * n + 1];
    const int tw = p.twh[n][0], th = p.twh[n][1];
    __shared__ int row[4];  // the per-row terms, once per row: sy, sy + 1 (clamped), b0, b1
    if (threadIdx.x == 0 && y < th) {
        int sy, b0, b1;
        resize_term(y, (double)H / (double)th, H, sy, b0, b1);
        row[0] = sy; row[1] = min(sy + 1, H - 1); row[2] = b0; row[3] = b1;
    }
    __syncthreads();
    const uint8_t* __restrict__ img = p.src + p.src_off[n];
    const size_t plane = (size_t)p.ph * p.pw;
    float* __restrict__ o = p.out + (size_t)n * 3 * plane + (size_t)y * p.pw;
    uint8_t* __restrict__ mk = p.mask + (size_t)n * plane + (size_t)y * p.pw;
    const double scale_x = (double)W / (double)tw;
    const int groups = (p.pw + VEC - 1) / VEC;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        int u[VEC][3];
        uint8_t in[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int x = g * VEC + e;
            in[e] = (y < th && x < tw) ? 1 : 0;
            u[e][0] = u[e][1] = u[e][2] = 0;  // the pad
            if (in[e]) {
                int sx, a0, a1;
                resize_term(x, scale_x, W, sx, a0, a1);
                const int sx1 = min(sx + 1, W - 1);
                const uint8_t* r0 = img + (size_t)row[0] * W * 3;
                const uint8_t* r1 = img + (size_t)row[1] * W * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int h0 = r0[sx * 3 + c] * a0 + r0[sx1 * 3 + c] * a1;
                    const int h1 = r1[sx * 3 + c] * a0 + r1[sx1 * 3 + c] * a1;
                    const int t = (((row[2] * (h0 >> 4)) >> 16) + ((row[3] * (h1 >> 4)) >> 16) + 2) >> 2;
                    u[e][c] = t < 0 ? 0 : (t > 255 ? 255 : t);
                }
            }
        }
        normalize_store<VEC>(p.norm, u, o + (size_t)g * VEC, plane);
        if constexpr (VEC == 4) *reinterpret_cast<uchar4*>(mk + (size_t)g * 4) = make_uchar4(in[0], in[1], in[2], in[3]);
        else mk[g] = in[0];
    }
}

}  // namespace
}  // namespace mp

extern "C" int mp_resize_pad_normalize(const uint8_t* src, const long long* src_offsets, const int* src_hw, const int* dst_wh_host,
                                       float* out, uint8_t* mask, int n, int pad_h, int pad_w, const float mean[3], const float stddev[3],
                                       mp_stream_t stream) {
    if (!src || !src_offsets || !src_hw || !dst_wh_host || !out || !mask || !mean || !stddev) return MP_ERR_NULL;
    if (n <= 0 || pad_h <= 0 || pad_w <= 0 || pad_h > 65535) return MP_ERR_SHAPE;
    mp::NormConst nc;
    if (!mp::fill_norm(mean, stddev, nc)) return MP_ERR_SHAPE;
    for (int i = 0; i < n; ++i) {
        const int tw = dst_wh_host[2 * i], th = dst_wh_host[2 * i + 1];
        if (tw <= 0 || th <= 0 || tw > pad_w || th > pad_h) return MP_ERR_SHAPE;
    }
    const size_t plane = (size_t)pad_h * pad_w;
    const bool wide = mp::wide_stores(pad_w, out, 4) && mp::wide_stores(pad_w, mask, 1);
    const int groups = wide ? pad_w / 4 : pad_w;
    int bx = (groups + 255) / 256;
    if (bx > 64) bx = 64;
    const auto kernel = wide ? mp::resize_pad_normalize_kernel<4> : mp::resize_pad_normalize_kernel<1>;
    for (int i0 = 0; i0 < n; i0 += mp::kRpnMaxImages) {  // one launch for a batch of up to 32 images
        const int cnt = n - i0 < mp::kRpnMaxImages ? n - i0 : mp::kRpnMaxImages;
        mp::RpnParams p{};
        p.src = src;
        p.src_off = src_offsets + i0;
        p.src_hw = src_hw + 2 * i0;
        p.out = out + (size_t)i0 * 3 * plane;
        p.mask = mask + (size_t)i0 * plane;
        p.ph = pad_h;
        p.pw = pad_w;
        p.norm = nc;
        for (int i = 0; i < cnt; ++i) { p.twh[i][0] = dst_wh_host[2 * (i0 + i)]; p.twh[i][1] = dst_wh_host[2 * (i0 + i) + 1]; }
        hipLaunchKernelGGL(kernel, dim3(bx, pad_h, cnt), dim3(256), 0, mp::as_stream(stream), p);
        const int rc = mp::check_launch();
        if (rc != MP_OK) return rc;
    }
    return MP_OK;
}

// ---- bottom-up train-time augmentation of a batch in ONE launch: BottomUpRandomAffine + BottomUpHorizontalRandomFlip + Normalize +
// HWC2CHW (bottomup_transform.py:304-460, :88-140, data_factory.py:129-133).  Per image the 2x3 matrices of the s heat-map stages and
// of the image arrive together; a workgroup owns 256 thread-groups of ONE plane - the image or the mask of one stage - so the inverse
// matrix is formed once per workgroup and the plane kind never diverges inside a wave.
//   image: sample_linear + normalize_store, i.e. mp_warp_affine's planes to the bit
//   mask:  cv2.warpAffine(mask, M, (W_i, H_i), flags=INTER_NEAREST), written into the [:H_i, :W_i] corner of the stage's
//          [hmax, wmax] plane, 0 in the padding.  The source plane of stage i is the image's one [H, W] mask, or - with a per-image
//          stage stride (mp_bottomup_train_augment_stages) - plane i of its [S, H, W] mask.
// The flip follows the warp (the reference's order): the value computed for column x is stored at column W - 1 - x.  It cannot be
// folded into the matrix bit-exactly, because the fixed-point column terms are rounded per destination column - so the thread that
// stores columns [4g, 4g + 4) computes the mirrored columns and the 16-byte vector leaves in reversed order.  (warp_affine_kernel's
// mirror is the other one: of the SOURCE, before the warp.)
// Every byte of both outputs is written here (no memset pass), no atomics.
namespace mp {
namespace {

constexpr int kAugMaxStages = 8;  // (W_i, H_i) of every stage travel in the kernel arguments

struct AugParams {
    const uint8_t* src;
    const long long* src_off;
    const int* src_hw;
    const uint8_t* msrc;
    const long long* msrc_off;
    const long long* msrc_stage;  // NULL, or per image the byte stride from one stage's source plane to the next
    const double* trans;  // [n, s + 1, 6]: stages first, the image last
    const int* flip;
    float* image;   // [n, 3, out_h, out_w]
    uint8_t* mask;  // [n, s, hmax, wmax]
    int s, out_h, out_w, hmax, wmax;
    int img_tiles, mask_tiles;  // workgroups per image plane set / per stage plane
    NormConst norm;
    int wh[kAugMaxStages][2];
};

// VEC adjacent destination pixels of one image row, all three planes
template <int VEC>
__device__ __forceinline__ void augment_image_group(const AugParams& p, const double* inv, const uint8_t* __restrict__ img, int H, int W,
                                                    bool mirror, int n, int g) {
    const int gpr = p.out_w / VEC;
    if (g >= p.out_h * gpr) return;
    const int y = g / gpr, x0 = (g - y * gpr) * VEC;
    int X0, Y0, u[VEC][3];
    row_terms(inv, y, 16, X0, Y0);
#pragma unroll
    for (int e = 0; e < VEC; ++e)  // the value stored at column x0 + e is computed for the mirrored column
        sample_linear(inv, img, H, W, false, X0, Y0, mirror ? p.out_w - 1 - (x0 + e) : x0 + e, u[e]);
    const size_t plane = (size_t)p.out_h * p.out_w;
    normalize_store<VEC>(p.norm, u, p.image + (size_t)n * 3 * plane + (size_t)y * p.out_w + x0, plane);
}

// VEC adjacent pixels of one row of one stage's [hmax, wmax] mask plane
template <int VEC>
__device__ __forceinline__ void augment_mask_group(const AugParams& p, const double* inv, const uint8_t* __restrict__ msk, int H, int W,
                                                   bool mirror, int n, int stage, int g) {
    const int gpr = p.wmax / VEC;
    if (g >= p.hmax * gpr) return;
    const int y = g / gpr, x0 = (g - y * gpr) * VEC;
    const int sw = p.wh[stage][0], sh = p.wh[stage][1];
    uint8_t v[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) v[e] = 0;
    if (y < sh) {
        int X0, Y0;
        row_terms(inv, y, 512, X0, Y0);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (x0 + e >= sw) continue;
            const int x = mirror ? sw - 1 - (x0 + e) : x0 + e;
            const int sx = saturate_short((X0 + cv_round(inv[0] * x * 1024.0)) >> 10);
            const int sy = saturate_short((Y0 + cv_round(inv[3] * x * 1024.0)) >> 10);
            if (sx >= 0 && sx < W && sy >= 0 && sy < H) v[e] = msk[(size_t)sy * W + sx];
        }
    }
    uint8_t* __restrict__ o = p.mask + (((size_t)n * p.s + stage) * p.hmax + y) * p.wmax + x0;
    if constexpr (VEC == 4) *reinterpret_cast<uchar4*>(o) = make_uchar4(v[0], v[1], v[2], v[3]);
    else o[0] = v[0];
}

// VI / VM = 4: four destination pixels per thread, one 16-byte store per fp32 plane / one 4-byte store of the mask; 1 = the scalar
// form for widths (or base addresses) that do not allow it
template <int VI, int VM>
__global__ __launch_bounds__(256) void bottomup_train_augment_kernel(AugParams p) {
    const int n = blockIdx.y;
    int tile = blockIdx.x;
    const bool is_image = tile < p.img_tiles;
    int stage = p.s;  // the index of this plane's matrix
    if (!is_image) {
        tile -= p.img_tiles;
        stage = tile / p.mask_tiles;
        tile -= stage * p.mask_tiles;
    }
    __shared__ double inv[6];
    if (threadIdx.x == 0) invert_affine(p.trans + ((size_t)n * (p.s + 1) + stage) * 6, inv);
    __syncthreads();
    const int H = p.src_hw[2 * n], W = p.src_hw[2 * n + 1];
    const bool mirror = p.flip && p.flip[n] != 0;
    const int g = tile * 256 + threadIdx.x;
    if (is_image) augment_image_group<VI>(p, inv, p.src + p.src_off[n], H, W, mirror, n, g);
    else augment_mask_group<VM>(p, inv, p.msrc + p.msrc_off[n] + (p.msrc_stage ? p.msrc_stage[n] * stage : 0), H, W, mirror, n, stage, g);
}

}  // namespace
}  // namespace mp

extern "C" int mp_bottomup_train_augment_stages(const uint8_t* src, const long long* src_offsets, const int* src_hw, const uint8_t* mask_src,
                                                const long long* mask_offsets, const long long* mask_stage_stride, const double* trans,
                                                const int* flip, const int* stage_wh_host, float* image, uint8_t* mask, int n, int s,
                                                int out_h, int out_w, int hmax, int wmax, const float mean[3], const float stddev[3],
                                                mp_stream_t stream) {
    if (!src || !src_offsets || !src_hw || !mask_src || !mask_offsets || !trans || !stage_wh_host || !image || !mask || !mean || !stddev)
        return MP_ERR_NULL;
    if (s < 1 || s > mp::kAugMaxStages) return MP_ERR_UNSUPPORTED;
    if (n <= 0 || n > 65535 || out_h <= 0 || out_w <= 0 || hmax <= 0 || wmax <= 0) return MP_ERR_SHAPE;
    mp::AugParams p{};
    if (!mp::fill_norm(mean, stddev, p.norm)) return MP_ERR_SHAPE;
    for (int i = 0; i < s; ++i) {
        const int w = stage_wh_host[2 * i], h = stage_wh_host[2 * i + 1];
        if (w <= 0 || h <= 0 || w > wmax || h > hmax) return MP_ERR_SHAPE;
        p.wh[i][0] = w; p.wh[i][1] = h;
    }
    if ((long long)out_h * out_w > (1LL << 30) || (long long)hmax * wmax > (1LL << 30)) return MP_ERR_SHAPE;  // group indices are int
    const bool wide_i = mp::wide_stores(out_w, image, 4), wide_m = mp::wide_stores(wmax, mask, 1);
    p.src = src; p.src_off = src_offsets; p.src_hw = src_hw;
    p.msrc = mask_src; p.msrc_off = mask_offsets; p.msrc_stage = mask_stage_stride;
    p.trans = trans; p.flip = flip;
    p.image = image; p.mask = mask;
    p.s = s; p.out_h = out_h; p.out_w = out_w; p.hmax = hmax; p.wmax = wmax;
    const long long img_groups = (long long)out_h * (out_w / (wide_i ? 4 : 1)), mask_groups = (long long)hmax * (wmax / (wide_m ? 4 : 1));
    p.img_tiles = (int)((img_groups + 255) / 256);
    p.mask_tiles = (int)((mask_groups + 255) / 256);
    const long long tiles = (long long)p.img_tiles + (long long)s * p.mask_tiles;
    if (tiles > 0x7fffffffLL) return MP_ERR_SHAPE;
    const auto kernel = wide_i ? (wide_m ? mp::bottomup_train_augment_kernel<4, 4> : mp::bottomup_train_augment_kernel<4, 1>)
                               : (wide_m ? mp::bottomup_train_augment_kernel<1, 4> : mp::bottomup_train_augment_kernel<1, 1>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)n), dim3(256), 0, mp::as_stream(stream), p);
    return mp::check_launch();
}

// one source mask plane per image, tiled over the stages: the stride-0 case
extern "C" int mp_bottomup_train_augment(const uint8_t* src, const long long* src_offsets, const int* src_hw, const uint8_t* mask_src,
                                         const long long* mask_offsets, const double* trans, const int* flip, const int* stage_wh_host,
                                         float* image, uint8_t* mask, int n, int s, int out_h, int out_w, int hmax, int wmax,
                                         const float mean[3], const float stddev[3], mp_stream_t stream) {
    return mp_bottomup_train_augment_stages(src, src_offsets, src_hw, mask_src, mask_offsets, nullptr, trans, flip, stage_wh_host, image, mask,
                                            n, s, out_h, out_w, hmax, wmax, mean, stddev, stream);
}
