// HBM-bound kernels of the top-down pose hot path (gfx950): decoder, flip-test aggregation, Gaussian target generation.  One 64-lane
// wavefront per (sample, joint) map for the reductions; float4 (16 B / lane) coalesced streaming for the element-wise passes.
//
// fp contraction is OFF in this file: the decoder / target arithmetic restates reference expressions
// evaluated without FMA (numpy / MindSpore CPU), and index / coordinate results are compared
// bit-for-bit with the CPU oracle.
#include "common.h"
#include "reduce.h"

#include <math.h>

#pragma clang fp contract(off)

namespace mp {

struct DecodeParams {
    const float* hm;          // [N,K,H,W]
    const float* hf;          // flipped run output [N,K,H,W] or nullptr
    const int32_t* flip_index;
    float* avg_out;           // optional
    const float* center;
    const float* scale;
    const float* score;
    float* preds;
    float* boxes;
    int32_t* argmax;
    const float* blur;
    float* dark_terms;        // optional debug output [N*K][16] (mp_decode_topdown_debug), else nullptr
    int n, k, h, w;
    int refine, use_udp, to_original, ks, shift_heatmap;
    float pixel_std;
};

// value of the (possibly flip-aggregated) heat-map at (y, x) of one (n, k) plane
// topdown_inferencer.py:171-187: flipped_back[k][y][x] = flipped[flip_index[k]][y][W-1-x'],
// x' = x-1 for x >= 1 when shift_heatmap (column 0 keeps its own value), then (h + fb) * 0.5
template <bool FLIP>
__device__ __forceinline__ float plane_val(const float* __restrict__ a, const float* __restrict__ b, int w,
                                           int shift, int y, int x) {
    float v = a[y * w + x];
    if (FLIP) {
        int xs = (shift && x >= 1) ? x - 1 : x;
        float f = b[y * w + (w - 1 - xs)];
        v = (v + f) * 0.5f;
    }
    return v;
}

// the map one wave decodes: plane a of the run, under the flip test averaged with plane b of the mirrored run
template <bool FLIP>
struct Map {
    const float* a;
    const float* b;
    int h, w, shift;
    __device__ __forceinline__ float at(int y, int x) const { return plane_val<FLIP>(a, b, w, shift, y, x); }
    __device__ __forceinline__ bool inside(int y, int x) const { return y >= 0 && y < h && x >= 0 && x < w; }
};

// One wave per (n, k) map.  top_down_decoder.py:72-205.
constexpr int kDarkFastKs = 17;                                  // largest blur kernel of the register-patch path: (17 + 2)^2 = 361 <= 6 x 64
constexpr int kDarkPatchPerLane = 6;
constexpr int kDarkTable = (kDarkFastKs + 4) * (kDarkFastKs + 4);  // the blur table with a two-wide zero border

// The lane's share of the map, streamed once: its running arg-max (strict >, indices ascend per lane, so the first of equal values
// stays; in locals - through the references the guarded updates compile to selects) and, under the flip test, the average.
template <bool FLIP>
__device__ __forceinline__ void stream_argmax(const Map<FLIP>& m, float* avg, int lane, float& best_out, int& bidx_out) {
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    const float *a = m.a, *b = m.b;
    const int h = m.h, w = m.w, hw = h * w;
    if ((hw & 3) == 0 && (!FLIP || (w & 3) == 0)) {
        // float4 streaming: lane reads 16 B at float4 index lane + 64 t (indices ascend per lane), FOUR quads requested before the
        // first is looked at (a 64x48 map is 12 quads per lane: three round trips instead of twelve).  Flip test: the four values of
        // the mirrored run that meet pixels x .. x + 3 of row y are b[y][W-1-xs], xs = x - 1 (x >= 1, shift) - four consecutive
        // floats read backwards, one element off 16-byte alignment when shifted: scalar loads of one cache line
        const float4* a4 = reinterpret_cast<const float4*>(a);
        float4* avg4 = reinterpret_cast<float4*>(avg);
        const int nq = hw >> 2, wq = w >> 2;
        // (twelve quads in flight per lane - the whole 64x48 map in one round trip - measured no faster than four: 8.9 vs 8.1 us
        // HBM-resident, 5.4 vs 5.1 us cache-resident)
        constexpr int B = 4;
        for (int q0 = lane; q0 < nq; q0 += 64 * B) {
            float4 v[B], f[B];
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int q = q0 + 64 * j;
                if (q < nq) {
                    v[j] = a4[q];
                    if (FLIP) {
                        const int y = q / wq, x = (q - y * wq) << 2;
                        const float* br = b + y * w;
                        const int s = m.shift ? 1 : 0;
                        f[j].x = br[w - 1 - (x >= 1 ? x - s : x)];
                        f[j].y = br[w - 1 - (x + 1 - s)];
                        f[j].z = br[w - 1 - (x + 2 - s)];
                        f[j].w = br[w - 1 - (x + 3 - s)];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int q = q0 + 64 * j;
                if (q < nq) {
                    float4 u = v[j];
                    if (FLIP) {  // the expression of plane_val: (v + f) * 0.5f
                        u.x = (u.x + f[j].x) * 0.5f; u.y = (u.y + f[j].y) * 0.5f; u.z = (u.z + f[j].z) * 0.5f; u.w = (u.w + f[j].w) * 0.5f;
                        if (avg) avg4[q] = u;
                    }
                    const int i = q << 2;
                    if (u.x > best) { best = u.x; bidx = i; }
                    if (u.y > best) { best = u.y; bidx = i + 1; }
                    if (u.z > best) { best = u.z; bidx = i + 2; }
                    if (u.w > best) { best = u.w; bidx = i + 3; }
                }
            }
        }
    } else {
        for (int y = 0; y < h; ++y) {
            for (int x = lane; x < w; x += 64) {
                float v = m.at(y, x);
                if (avg) avg[y * w + x] = v;
                if (v > best) { best = v; bidx = y * w + x; }
            }
        }
    }
    best_out = best, bidx_out = bidx;
}

// no value beat -inf: numpy's argmax of an all -inf / NaN map is 0, and the maximum is the value there
template <bool FLIP>
__device__ __forceinline__ void empty_map_rule(const Map<FLIP>& m, float& best, int& bidx) {
    if (bidx == 0x7fffffff) {
        bidx = 0;
        best = m.at(0, 0);
    }
}

// :118-141  a quarter pixel toward the larger neighbour; dx defined for 1 <= x <= W-2 (any y), dy for 1 <= y <= H-2 (any x)
template <bool FLIP>
__device__ __forceinline__ void quarter_pixel_shift(const Map<FLIP>& m, int yi, int xi, float& cx, float& cy) {
    float dx = 0.f, dy = 0.f;
    if (xi >= 1 && xi <= m.w - 2) dx = m.at(yi, xi + 1) - m.at(yi, xi - 1);
    if (yi >= 1 && yi <= m.h - 2) dy = m.at(yi + 1, xi) - m.at(yi - 1, xi);
    float sx = (dx > 0.f) ? 1.f : ((dx < 0.f) ? -1.f : 0.f);
    float sy = (dy > 0.f) ? 1.f : ((dy < 0.f) ? -1.f : 0.f);
    cx = cx + sx * 0.25f;
    cy = cy + sy * 0.25f;
}

// a position's blurred value -> its log-value: clip [1e-3, 50] -> log ; outside the map: the zero pad, applied AFTER log
__device__ __forceinline__ float dark_log(float sum, bool inside) {
    return inside ? logf(fminf(fmaxf(sum, 0.001f), 50.f)) : 0.f;
}

// :171-205  L[oy + 1][ox + 1] = the log of the k x k blur at (yi + oy, xi + ox): only the 3x3 neighbourhood of the arg-max needs the
// blur.  The nine blurred values read a (ks + 2)^2 patch around the arg-max.  fast: the blur table is in s_blur (decode_kernel).
template <bool FLIP>
__device__ __forceinline__ void dark_log_values(const Map<FLIP>& m, const float* __restrict__ blur, const float* s_blur, int ks, bool fast,
                                                int yi, int xi, int lane, float (&L)[3][3]) {
    const int r = ks >> 1;
    if (fast) {
        float part[3][3];
        // every pixel of the patch is fetched ONCE (<= 6 per lane, all requested before the first is used; zero outside the map =
        // the blur's padding) and feeds the windows of all nine positions from registers: window (oy, ox) meets patch pixel
        // (iy, ix) with tap (iy - 1 - oy, ix - 1 - ox) = padded-table entry (iy + 1 - oy, ix + 1 - ox).  Nine wave sums.
        const int side = ks + 2, tw = ks + 4, np = side * side;
        float pv[kDarkPatchPerLane];
        int tb[kDarkPatchPerLane];
#pragma unroll
        for (int e = 0; e < kDarkPatchPerLane; ++e) {
            const int idx = min(lane + 64 * e, np - 1);
            const int iy = idx / side, ix = idx - iy * side;
            const int yy = yi + iy - (r + 1), xx = xi + ix - (r + 1);
            const bool ok = lane + 64 * e < np && m.inside(yy, xx);
            pv[e] = ok ? m.at(yy, xx) : 0.f;
            tb[e] = (iy + 1) * tw + ix + 1;
        }
#pragma unroll
        for (int oy = 0; oy < 3; ++oy)
#pragma unroll
            for (int ox = 0; ox < 3; ++ox) part[oy][ox] = 0.f;
#pragma unroll
        for (int e = 0; e < kDarkPatchPerLane; ++e) {
            if (64 * e >= np) break;  // wave-uniform
#pragma unroll
            for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
                for (int ox = -1; ox <= 1; ++ox) part[oy + 1][ox + 1] += s_blur[tb[e] - oy * tw - ox] * pv[e];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)  // the nine butterflies advance together (independent chains)
#pragma unroll
            for (int i = 0; i < 9; ++i) part[i / 3][i % 3] += __shfl_xor(part[i / 3][i % 3], off, 64);
#pragma unroll
        for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
            for (int ox = -1; ox <= 1; ++ox) L[oy + 1][ox + 1] = dark_log(part[oy + 1][ox + 1], m.inside(yi + oy, xi + ox));
    } else {
        // per tap: the lanes share one window's taps, a position outside the map reads nothing
        const int taps = ks * ks;
#pragma unroll
        for (int oy = -1; oy <= 1; ++oy) {
#pragma unroll
            for (int ox = -1; ox <= 1; ++ox) {
                const int py = yi + oy, px = xi + ox;
                float s = 0.f;
                if (m.inside(py, px)) {
                    for (int t = lane; t < taps; t += 64) {
                        int ti = t / ks, tj = t - ti * ks;
                        int yy = py + ti - r, xx = px + tj - r;
                        if (m.inside(yy, xx)) s += blur[t] * m.at(yy, xx);
                    }
                }
                L[oy + 1][ox + 1] = dark_log(wave_sum(s), m.inside(py, px));
            }
        }
    }
}

// one Newton step on the log-values: central differences, Hessian + 1e-7 I.  terms: the row's 16 debug values (lane 0) or nullptr
__device__ __forceinline__ void hessian_step(const float (&L)[3][3], float* terms, int lane, float& cx, float& cy) {
    const float i_ = L[1][1], ix1 = L[1][2], ix1_ = L[1][0], iy1 = L[2][1], iy1_ = L[0][1];
    const float ix1y1 = L[2][2], ix1_y1_ = L[0][0];
    const float dx = 0.5f * (ix1 - ix1_);
    const float dy = 0.5f * (iy1 - iy1_);
    const float dxx = ix1 - 2.f * i_ + ix1_;
    const float dyy = iy1 - 2.f * i_ + iy1_;
    const float dxy = 0.5f * (ix1y1 - ix1 - iy1 + i_ + i_ - ix1_ - iy1_ + ix1_y1_);
    const float ha = dxx + 1e-7f, hd = dyy + 1e-7f;  // Hessian + 1e-7 I
    const float det = ha * hd - dxy * dxy;
    if (terms && lane == 0) {  // intermediates of the refinement for the parity tests (uniform branch)
#pragma unroll
        for (int i = 0; i < 9; ++i) terms[i] = L[i / 3][i % 3];
        terms[9] = dx; terms[10] = dy; terms[11] = dxx; terms[12] = dyy; terms[13] = dxy; terms[14] = det; terms[15] = 0.f;
    }
    cx = cx - (hd * dx - dxy * dy) / det;
    cy = cy - (ha * dy - dxy * dx) / det;
}

// :143-169  heat-map pixels -> the original image, by the sample's box
__device__ __forceinline__ void to_original_image(const DecodeParams& p, float sxs, float sys, float ctx, float cty, float& cx, float& cy) {
    const float s_x = sxs * p.pixel_std, s_y = sys * p.pixel_std;
    const float den_x = p.use_udp ? (float)(p.w - 1) : (float)p.w;
    const float den_y = p.use_udp ? (float)(p.h - 1) : (float)p.h;
    const float kx = s_x / den_x, ky = s_y / den_y;
    cx = cx * kx + ctx - s_x * 0.5f;
    cy = cy * ky + cty - s_y * 0.5f;
}

template <bool FLIP>
__global__ __launch_bounds__(256) void decode_kernel(DecodeParams p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int rows = p.n * p.k;
    // DARK: the k x k blur table goes to LDS ONCE per block, zero-padded by two on every side - the nine windows around the arg-max
    // then read their taps at fixed offsets from one address per patch pixel, no bounds test and no dependent global load per tap
    // (27 scattered table loads per lane were most of the refinement's 5 us)
    __shared__ float s_blur[kDarkTable];
    const bool dark_fast = p.refine == MP_REFINE_DARK && p.ks <= kDarkFastKs;
    if (dark_fast) {
        const int tw = p.ks + 4;
        for (int i = threadIdx.x; i < tw * tw; i += 256) {
            const int ty = i / tw - 2, tx = i - (i / tw) * tw - 2;
            s_blur[i] = (ty >= 0 && ty < p.ks && tx >= 0 && tx < p.ks) ? p.blur[ty * p.ks + tx] : 0.f;
        }
        __syncthreads();
    }
    if (row >= rows) return;  // whole wave exits; no block-level barrier below
    const int n = row / p.k, k = row - n * p.k;
    const int w = p.w, hw = p.h * w;
    const Map<FLIP> m{p.hm + (size_t)row * hw, FLIP ? p.hf + ((size_t)n * p.k + p.flip_index[k]) * hw : nullptr, p.h, w,
                      p.shift_heatmap};
    float* avg = (FLIP && p.avg_out) ? p.avg_out + (size_t)row * hw : nullptr;

    float best;  // and bidx: set by stream_argmax
    int bidx;
    stream_argmax<FLIP>(m, avg, lane, best, bidx);
    wave_argmax(best, bidx);
    empty_map_rule<FLIP>(m, best, bidx);
    const int yi = bidx / w, xi = bidx - yi * w;
    float cx = (float)xi, cy = (float)yi;  // :111-112 (exact: idx < 2^24)

    if (p.refine == MP_REFINE_SHIFT) {
        quarter_pixel_shift<FLIP>(m, yi, xi, cx, cy);
    } else if (p.refine == MP_REFINE_DARK) {
        float L[3][3];
        dark_log_values<FLIP>(m, p.blur, s_blur, p.ks, dark_fast, yi, xi, lane, L);
        hessian_step(L, p.dark_terms ? p.dark_terms + (size_t)row * 16 : nullptr, lane, cx, cy);
    }

    if (lane == 0) {
        const float sxs = p.scale[n * 2 + 0], sys = p.scale[n * 2 + 1];
        const float ctx = p.center[n * 2 + 0], cty = p.center[n * 2 + 1];
        if (p.to_original) to_original_image(p, sxs, sys, ctx, cty, cx, cy);
        float* pr = p.preds + (size_t)row * 3;
        pr[0] = cx;
        pr[1] = cy;
        pr[2] = best;
        if (p.argmax) p.argmax[row] = bidx;
        if (k == 0) {
            float* bx = p.boxes + (size_t)n * 6;  // :88-92
            bx[0] = ctx;
            bx[1] = cty;
            bx[2] = sxs;
            bx[3] = sys;
            bx[4] = (sxs * p.pixel_std) * (sys * p.pixel_std);
            bx[5] = p.score[n];
        }
    }
}

// stand-alone aggregation (EvalNet output_raw wants the averaged heat-map): block per (n, k) plane
__global__ __launch_bounds__(256) void flip_aggregate_kernel(const float* __restrict__ hm, const float* __restrict__ hf,
                                                             const int32_t* __restrict__ flip_index,
                                                             float* __restrict__ out, int k, int h, int w, int shift) {
    const int row = blockIdx.x;  // (n, k)
    const int nn = row / k, kk = row - nn * k;
    const int hw = h * w;
    const float* a = hm + (size_t)row * hw;
    const float* b = hf + ((size_t)nn * k + flip_index[kk]) * hw;
    float* o = out + (size_t)row * hw;
    for (int i = threadIdx.x; i < hw; i += blockDim.x) {
        int y = i / w, x = i - y * w;
        o[i] = plane_val<true>(a, b, w, shift, y, x);
    }
}

// ------------------------------------------------------------------------------------------
// Gaussian target: one 256-thread block per (n, k) plane; zero stores of the whole plane (16 B / lane
// when W % 4 == 0) first, the stamp's pixels behind them.  topdown_transform.py:324-430.
// ------------------------------------------------------------------------------------------
struct TargetParams {
    const float* kp;
    const float* patch;
    const double* jw;
    float* target;
    float* tw;
    int n, k, h, w, side, use_udp;
    double fsx, fsy, sigma;
};

// the stamp's value at map pixel (x, y) of its window: (ix0, iy0) the window's first pixel, (gx0, gy0) what it shows of the stamp
__device__ __forceinline__ float target_value(const TargetParams& p, int y, int x, int ix0, int iy0, int gx0, int gy0, double x0p,
                                              double y0p, double two_sigma2) {
    int gx = gx0 + (x - ix0), gy = gy0 + (y - iy0);
    if (p.use_udp) {
        double dx = (double)gx - x0p, dy = (double)gy - y0p;
        double e = -(dx * dx + dy * dy) / two_sigma2;
        return (float)exp(e);
    }
    gx = min(gx, p.side - 1);
    gy = min(gy, p.side - 1);
    return p.patch[gy * p.side + gx];
}

__global__ __launch_bounds__(256) void gaussian_target_kernel(TargetParams p) {
    const int row = blockIdx.x;
    const int k = row % p.k;
    const int h = p.h, w = p.w;
    float* out = p.target + (size_t)row * h * w;
    // The plane is zeros but for one (6 sigma + 1)^2 stamp, and WHERE the stamp lies takes a chain of fp64 divisions and roundings:
    // the zero stores go out first - nothing of them depends on the key point - and the set-up runs under them (round 4 did the
    // set-up first: 8.2 us for 26.7 MB of stores, 0.40 of the HBM peak).  The stamp's pixels are stored a second time behind a
    // workgroup barrier (same block, so the barrier's release orders them behind the zeros): <= 5 % more bytes.
    if ((w & 3) == 0) {
        const int nq = (h * w) >> 2;
        const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int q = threadIdx.x; q < nq; q += blockDim.x) reinterpret_cast<float4*>(out)[q] = z4;
    } else {
        for (int i = threadIdx.x; i < h * w; i += blockDim.x) out[i] = 0.f;
    }
    const float kx = p.kp[(size_t)row * 3 + 0], ky = p.kp[(size_t)row * 3 + 1], vis = p.kp[(size_t)row * 3 + 2];
    double fx = (double)kx / p.fsx, fy = (double)ky / p.fsy;  // fp32 scalar / fp64 scalar -> fp64
    fx = fmin(fmax(fx, -1.0e9), 1.0e9);
    fy = fmin(fmax(fy, -1.0e9), 1.0e9);
    int mu_x, mu_y;
    if (p.use_udp) {
        mu_x = (int)(fx + 0.5);  // :399-400 int() truncates toward zero
        mu_y = (int)(fy + 0.5);
    } else {
        mu_x = (int)rint(fx);  // :350-351 Python round(): half-to-even
        mu_y = (int)rint(fy);
    }
    const double tmp = p.sigma * 3.0;
    const int ulx = (int)((double)mu_x - tmp), uly = (int)((double)mu_y - tmp);
    const int brx = (int)((double)mu_x + tmp + 1.0), bry = (int)((double)mu_y + tmp + 1.0);
    const bool oob = (ulx >= w) || (uly >= h) || (brx < 0) || (bry < 0);
    float weight = oob ? 0.f : vis;
    const bool stamp = (!oob) && (weight > 0.5f);
    const int gx0 = max(0, -ulx), gy0 = max(0, -uly);
    const int ix0 = max(0, ulx), ix1 = min(brx, w);
    const int iy0 = max(0, uly), iy1 = min(bry, h);
    const double size = 2.0 * tmp + 1.0;
    const double c0 = floor(size / 2.0);  // size // 2
    const double x0p = c0 + fx - (double)mu_x, y0p = c0 + fy - (double)mu_y;
    const double two_sigma2 = 2.0 * (p.sigma * p.sigma);

    __syncthreads();  // (uniform: every thread of the block gets here)
    if (stamp && ix1 > ix0 && iy1 > iy0) {
        const int sw = ix1 - ix0, cnt = sw * (iy1 - iy0);
        for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
            const int dy = i / sw, y = iy0 + dy, x = ix0 + (i - dy * sw);
            out[y * w + x] = target_value(p, y, x, ix0, iy0, gx0, gy0, x0p, y0p, two_sigma2);
        }
    }
    if (threadIdx.x == 0) {
        if (p.jw) weight = (float)((double)weight * p.jw[k]);  // :371-372 np.multiply(fp32, fp64)
        p.tw[row] = weight;
    }
}

// the operands every decode entry has, in the C ABI's order; the flip test's and the debug entry's stay zero: their entries set them
static DecodeParams decode_params(const float* heatmap, const float* center, const float* scale, const float* score, float* preds,
                                  float* boxes, int32_t* argmax_idx, int n, int k, int h, int w, int refine_mode, int use_udp,
                                  int to_original, float pixel_std, const float* blur_kernel, int kernel_size) {
    DecodeParams p{};
    p.hm = heatmap; p.center = center; p.scale = scale; p.score = score; p.preds = preds; p.boxes = boxes; p.argmax = argmax_idx;
    p.n = n; p.k = k; p.h = h; p.w = w; p.refine = refine_mode; p.use_udp = use_udp; p.to_original = to_original;
    p.pixel_std = pixel_std; p.blur = blur_kernel; p.ks = kernel_size;
    return p;
}

// refuses what the kernel does not serve, then launches; debug: the two extra refusals of mp_decode_topdown_debug
static int run_decode(const DecodeParams& p, bool debug, mp_stream_t stream) {
    if (!p.hm || !p.center || !p.scale || !p.score || !p.preds || !p.boxes) return MP_ERR_NULL;
    if (p.n <= 0 || p.k <= 0 || p.h <= 0 || p.w <= 0) return MP_ERR_SHAPE;
    if ((long long)p.h * p.w >= (1 << 24)) return MP_ERR_UNSUPPORTED;
    if (p.refine < MP_REFINE_NONE || p.refine > MP_REFINE_DARK) return MP_ERR_UNSUPPORTED;
    if (p.refine == MP_REFINE_DARK) {
        const int ks = p.ks;
        if (!p.blur) return MP_ERR_NULL;
        if (ks < 1 || (ks & 1) == 0 || ks > 63) return MP_ERR_UNSUPPORTED;
    }
    if (debug && p.refine != MP_REFINE_DARK) return MP_ERR_UNSUPPORTED;
    if (debug && !p.dark_terms) return MP_ERR_NULL;
    const dim3 grid((p.n * p.k + 3) / 4), block(256);
    if (p.hf)
        hipLaunchKernelGGL(decode_kernel<true>, grid, block, 0, as_stream(stream), p);
    else
        hipLaunchKernelGGL(decode_kernel<false>, grid, block, 0, as_stream(stream), p);
    return check_launch();
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_decode_topdown(const float* heatmap, const float* center, const float* scale, const float* score, float* preds,
                      float* boxes, int32_t* argmax_idx, int n, int k, int h, int w, int refine_mode, int use_udp,
                      int to_original, float pixel_std, const float* blur_kernel, int kernel_size,
                      mp_stream_t stream) {
    return run_decode(decode_params(heatmap, center, scale, score, preds, boxes, argmax_idx, n, k, h, w, refine_mode, use_udp, to_original,
                                    pixel_std, blur_kernel, kernel_size), false, stream);
}

int mp_decode_topdown_debug(const float* heatmap, const float* center, const float* scale, const float* score, float* preds,
                            float* boxes, int32_t* argmax_idx, int n, int k, int h, int w, int refine_mode, int use_udp,
                            int to_original, float pixel_std, const float* blur_kernel, int kernel_size, float* dark_terms,
                            mp_stream_t stream) {
    DecodeParams p = decode_params(heatmap, center, scale, score, preds, boxes, argmax_idx, n, k, h, w, refine_mode, use_udp, to_original,
                                   pixel_std, blur_kernel, kernel_size);
    p.dark_terms = dark_terms;
    return run_decode(p, true, stream);
}

int mp_flip_aggregate(const float* heatmap, const float* flipped, const int32_t* flip_index, float* avg_out, int n,
                      int k, int h, int w, int shift_heatmap, mp_stream_t stream) {
    if (!heatmap || !flipped || !flip_index || !avg_out) return MP_ERR_NULL;
    if (n <= 0 || k <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    if ((long long)n * k > 0x7fffffffLL) return MP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(flip_aggregate_kernel, dim3(n * k), dim3(256), 0, as_stream(stream), heatmap, flipped,
                       flip_index, avg_out, k, h, w, shift_heatmap ? 1 : 0);
    return check_launch();
}

int mp_flip_aggregate_decode(const float* heatmap, const float* flipped, const int32_t* flip_index, int shift_heatmap,
                             float* avg_out, const float* center, const float* scale, const float* score, float* preds,
                             float* boxes, int32_t* argmax_idx, int n, int k, int h, int w, int refine_mode,
                             int use_udp, int to_original, float pixel_std, const float* blur_kernel, int kernel_size,
                             mp_stream_t stream) {
    if (!flipped || !flip_index) return MP_ERR_NULL;
    DecodeParams p = decode_params(heatmap, center, scale, score, preds, boxes, argmax_idx, n, k, h, w, refine_mode, use_udp, to_original,
                                   pixel_std, blur_kernel, kernel_size);
    p.hf = flipped; p.flip_index = flip_index; p.avg_out = avg_out; p.shift_heatmap = shift_heatmap ? 1 : 0;
    return run_decode(p, false, stream);
}

int mp_gaussian_target(const float* keypoints, const float* patch, int patch_side, const double* joint_weights,
                       float* target, float* target_weight, int n, int k, int h, int w, double feat_stride_x,
                       double feat_stride_y, double sigma, int use_udp, mp_stream_t stream) {
    if (!keypoints || !target || !target_weight) return MP_ERR_NULL;
    if (!use_udp && !patch) return MP_ERR_NULL;
    if (n <= 0 || k <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    if (!(sigma > 0.0) || !(feat_stride_x > 0.0) || !(feat_stride_y > 0.0)) return MP_ERR_SHAPE;
    if (!use_udp && patch_side <= 0) return MP_ERR_SHAPE;
    TargetParams p{};
    p.kp = keypoints; p.patch = patch; p.jw = joint_weights; p.target = target; p.tw = target_weight;
    p.n = n; p.k = k; p.h = h; p.w = w; p.side = patch_side; p.use_udp = use_udp ? 1 : 0;
    p.fsx = feat_stride_x; p.fsy = feat_stride_y; p.sigma = sigma;
    hipLaunchKernelGGL(gaussian_target_kernel, dim3(n * k), dim3(256), 0, as_stream(stream), p);
    return check_launch();
}

}  // extern "C"
