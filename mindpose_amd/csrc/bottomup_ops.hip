// Bottom-up (associative-embedding) decoder of HigherHRNet on gfx950, plus the channel concatenation of its head and the column-band
// copy with which the plan runs convolutions too wide for their kernels (the 512 / 832-pixel images of the bottom-up recipe).
//
// Replaces bottom_up_decoder.py:81-203 of the reference (about ten MindSpore ops, each a full pass over the maps) with two launches:
//
//   bu_parse_kernel  one workgroup per (16 x 64 output tile, joint, image).  It builds the stage mean of the tile plus an NMS halo
//                    in LDS (every stage resized to H x W, masked), writes heatmap_raw and the resized tags of the tile, applies the
//                    max-pool NMS from LDS and sorts the tile's 1024 (value, flat index) keys; the first max_num keys go to a slab
//                    in the workspace.  No atomics: the slab and everything after it is deterministic.
//   bu_gather_kernel one workgroup per (joint, image) merges the slab into the global top max_num (chunks of 4096 keys, the
//                    running top max_num kept at the front of each chunk), then writes val_k, ind_k (with the +-0.25 shift) and
//                    tag_k gathered from the tagging map the first kernel wrote.
//
// Semantics restated from MindSpore behaviour [MS-knowledge]:
//   - ops.ResizeBilinear((H, W)) = align_corners=False, half_pixel_centers=False: src = dst * (in / out), x0 = floor(src),
//     x1 = min(x0 + 1, in - 1), fp32 lerp.  NOT torch's F.interpolate(align_corners=False), which uses half-pixel centres.
//   - stage mean: base = stage[-1]; base += resize(stage[i]) for i in order; base /= num_stages (a true division; skipped for
//     one stage).
//   - ops.ResizeNearestNeighbor of the mask: src = floor(dst * in / out); masked_fill(~mask, 0) before the NMS; heatmap_raw is the
//     masked map before the NMS.
//   - nn.MaxPool2d(k, stride 1, pad_mode="same") of the NMS pads with -inf; a pixel is kept when the window maximum equals it,
//     else it becomes 0.
//   - ops.top_k: values in descending order, equal values in ascending flat index (a key (ordered value, ~index) sorted
//     descending gives exactly that order; -0.0 is folded into +0.0 so that it ties with the zeros).
//   - shift_coordinate quirk: masked_select returns the max_num selected pixels in FLAT-INDEX order, but the offsets are added
//     to ind_k, which is in VALUE order: entry m gets sign(diff) * 0.25 of the m-th smallest selected flat index.
//
// Flip test (bottomup_inferencer.py:252-297 of the reference, _MultiRunNet): bu_parse_flip_kernel is the same kernel body reading a
// second set of stage tensors, the outputs of the horizontally mirrored image.  Every tap of a heat map is
// (a[k][y][x] + b[f[k]][y][ws - 1 - x]) * 0.5f at STAGE resolution (the resize has no half-pixel centres, so mirroring and resizing
// do not commute), and the tags of the mirrored run, b[K + f[k]][y][ws - 1 - x], follow the plain ones on the last axis of
// tagging (num_tags = 2 L).  The mirrored maps are never flipped, gathered, averaged or concatenated in memory.
//
// Multi-scale test (this project's protocol): bu_parse_multi_kernel is the same kernel body again, its heat map the
// mean over up to four runs of the network on the batch resized by one scale factor each: per run the stage mean above with EVERY
// stage resized to the scale-1 run's map (only that run's last stage is the map and is read directly), the runs summed in order and
// divided by their count.  Tags come from the scale-1 run alone.  mp_resize_bilinear_nchw makes the scaled inputs with the same
// resize_bilinear sample, so a source pixel q sits on s * q of the scaled image and the map resize reads exactly there.
//
// Behind the grouping (bottomup_match.hip) the file also holds the missing-joint refinement (bu_refine_kernel) and the tail of a
// batch on the persons the grouping left in device memory (bu_finish_score_kernel, bu_finish_refine_kernel); see their own comments.
//
// fp contraction is OFF in this file: the resize / mean arithmetic restates MindSpore's fp32 expressions and is compared
// bit-for-bit with a CPU restatement on dyadic inputs.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace mp {

constexpr int kBuTileH = 16;
constexpr int kBuTileW = 64;  // one wavefront per tile row: 256 B coalesced reads and writes
constexpr int kBuTilePix = kBuTileH * kBuTileW;
constexpr int kBuThreads = 256;
constexpr int kBuMaxStages = 4;
constexpr int kBuMaxRadius = 3;  // nms_kernel <= 7
constexpr int kBuHaloPix = (kBuTileH + 2 * kBuMaxRadius) * (kBuTileW + 2 * kBuMaxRadius);
constexpr int kBuMaxM = 64;
constexpr int kBuMergeKeys = 4096;
constexpr int kBuMergeThreads = 512;
constexpr int kBuMaxTags = 4;
constexpr int kBuFlipMaxJoints = 64;  // the flip form carries the joint permutation by value in its kernel parameters
constexpr int kBuMaxRuns = 4;         // scale factors of the multi-scale test

struct BuStage {
    const float* data;  // [N, C, Hs, Ws]
    int c, h, w;
    int tag_slot;       // position on the last axis of tagging, -1 = no tags in this stage
    float sy, sx;       // in / out
};

struct BuParseParams {
    BuStage st[kBuMaxStages];
    int ns;                       // st[ns - 1] is the full-resolution stage
    const uint8_t* mask;          // [N, MH, MW]
    int mh, mw;
    float msy, msx;
    int n, k, h, w, ktag, tag_per_joint, num_tags, r, m, tiles_x, tiles;
    float* raw;                   // [N, K, H, W]
    float* tagging;               // [N, KTAG, H, W, L]
    unsigned long long* slab;     // [N, K, tiles, M]
};

// the mirrored run of the flip test: the stage tensors of net(flip_W(image)), shaped as st[], and the joint permutation
struct BuFlip {
    const float* data[kBuMaxStages];
    int index[kBuFlipMaxJoints];  // joint k reads channel index[k] of the mirrored run; every entry validated on the host
};

// the runs of the multi-scale test, the scale-1 run (base) among them: heat-map stages only (tag_slot unused), sy / sx towards the
// base run's map; flipped = the mirrored partners under the flip test.  By value in the kernel parameters (648 bytes).
struct BuRuns {
    BuStage st[kBuMaxRuns][kBuMaxStages];
    const float* flipped[kBuMaxRuns][kBuMaxStages];
    int num_runs, base;
};

// One pixel of a stage plane as the resize sees it.  kTapPlain: the plane itself.  kTapMean: the flip test's heat map, the mean of
// the plane and the mirrored run's plane read at the mirrored column (one add, one multiply).  kTapMirror: the mirrored run alone.
enum { kTapPlain, kTapMean, kTapMirror };

template <int TAP>
struct BuTap {
    const float* __restrict__ a;  // plane of the plain run (unused by kTapMirror)
    const float* __restrict__ b;  // plane of the mirrored run (unused by kTapPlain)
    int iw;
    __device__ __forceinline__ float operator()(int y, int x) const {
        if (TAP == kTapPlain) return a[(size_t)y * iw + x];
        const float m = b[(size_t)y * iw + (iw - 1 - x)];
        return TAP == kTapMirror ? m : (a[(size_t)y * iw + x] + m) * 0.5f;
    }
};

__device__ __forceinline__ unsigned ordered_bits(float v) {
    unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float unordered_float(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ unsigned long long topk_key(float v, int flat) {
    if (v == 0.0f) v = 0.0f;  // -0.0 ties with +0.0, as in a value comparison
    return ((unsigned long long)ordered_bits(v) << 32) | (unsigned long long)(0xffffffffu - (unsigned)flat);
}

// ResizeBilinear sample (align_corners=False, half_pixel_centers=False) of one plane at output pixel (y, x)
template <int TAP>
__device__ __forceinline__ float resize_bilinear(const BuTap<TAP>& tap, int ih, int iw, float sy, float sx, int y, int x) {
    const float fy = (float)y * sy, fx = (float)x * sx;
    const int y0 = min((int)floorf(fy), ih - 1), x0 = min((int)floorf(fx), iw - 1);
    const int y1 = min(y0 + 1, ih - 1), x1 = min(x0 + 1, iw - 1);
    const float dy = fy - (float)y0, dx = fx - (float)x0;
    const float a = tap(y0, x0), b = tap(y0, x1);
    const float c = tap(y1, x0), d = tap(y1, x1);
    const float top = a + (b - a) * dx;
    const float bot = c + (d - c) * dx;
    return top + (bot - top) * dy;
}

// plane of channel c of image n of stage s, in the plain run and (FLIP) in the mirrored run at channel cf
template <int TAP>
__device__ __forceinline__ BuTap<TAP> stage_tap(const BuStage& s, const float* flipped, int n, int c, int cf) {
    const size_t hw = (size_t)s.h * s.w;
    return BuTap<TAP>{s.data + ((size_t)n * s.c + c) * hw, TAP == kTapPlain ? nullptr : flipped + ((size_t)n * s.c + cf) * hw, s.w};
}

// stage mean of one run at map pixel (y, x) of (n, k): the last stage first - read at (y, x) when it IS the map (AT_MAP: the
// scale-1 run), else resized like the others - then the lower stages in order.  FLIP: of the flip test's averaged heat maps, kf =
// the mirrored run's channel, flipped[i] = its stage i.
template <bool FLIP, bool AT_MAP>
__device__ __forceinline__ float stage_mean(const BuStage* st, const float* const* flipped, int ns, int n, int k, int kf, int y, int x) {
    constexpr int kTap = FLIP ? kTapMean : kTapPlain;
    const BuStage& full = st[ns - 1];
    const BuTap<kTap> last = stage_tap<kTap>(full, FLIP ? flipped[ns - 1] : nullptr, n, k, kf);
    float v = AT_MAP ? last(y, x) : resize_bilinear(last, full.h, full.w, full.sy, full.sx, y, x);
    for (int i = 0; i < ns - 1; ++i) {
        const BuStage& s = st[i];
        v = v + resize_bilinear(stage_tap<kTap>(s, FLIP ? flipped[i] : nullptr, n, k, kf), s.h, s.w, s.sy, s.sx, y, x);
    }
    if (ns > 1) v = v / (float)ns;
    return v;
}

// v where the nearest-resized mask of image n keeps map pixel (y, x), else 0
__device__ __forceinline__ float masked(const BuParseParams& p, float v, int n, int y, int x) {
    const int my = min((int)floorf((float)y * p.msy), p.mh - 1), mx = min((int)floorf((float)x * p.msx), p.mw - 1);
    return p.mask[((size_t)n * p.mh + my) * p.mw + mx] ? v : 0.0f;
}

// masked stage mean at (n, k, y, x), inside the map
template <bool FLIP>
__device__ __forceinline__ float aggregate(const BuParseParams& p, const BuFlip* fl, int n, int k, int kf, int y, int x) {
    return masked(p, stage_mean<FLIP, true>(p.st, FLIP ? fl->data : nullptr, p.ns, n, k, kf, y, x), n, y, x);
}

// the multi-scale test: the stage means of all runs summed in run order and divided by their count, then masked.  The scale-1 run
// (base; its stages are p.st too) is read as aggregate() reads it, so one run gives aggregate()'s value operation for operation.
template <bool FLIP>
__device__ __forceinline__ float aggregate_runs(const BuParseParams& p, const BuRuns& rs, int n, int k, int kf, int y, int x) {
    float total = 0.0f;
    for (int r = 0; r < rs.num_runs; ++r) {
        const float v = r == rs.base ? stage_mean<FLIP, true>(rs.st[r], rs.flipped[r], p.ns, n, k, kf, y, x)
                                     : stage_mean<FLIP, false>(rs.st[r], rs.flipped[r], p.ns, n, k, kf, y, x);
        total = r == 0 ? v : total + v;
    }
    if (rs.num_runs > 1) total = total / (float)rs.num_runs;
    return masked(p, total, n, y, x);
}

// descending bitonic sort of P keys in LDS by NT threads (P a power of two, P / 2 a multiple of NT)
template <int P, int NT>
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long* s) {
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int q = 0; q < P / 2 / NT; ++q) {
                const int t = (int)threadIdx.x + q * NT;
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i + j;
                const unsigned long long a = s[i], b = s[l];
                const bool desc = (i & kk) == 0;
                if (desc ? (a < b) : (a > b)) {
                    s[i] = b;
                    s[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

// the body of every parse kernel; FLIP folds the mirrored run in (fl, else unused).  tag_per_joint is set under FLIP.  MULTI: the heat
// map is the mean over the runs rs (else unused); p and fl describe the scale-1 run, the only one whose tags are read.
template <bool FLIP, bool MULTI>
__device__ __forceinline__ void bu_parse_body(const BuParseParams& p, const BuFlip* fl, const BuRuns* rs) {
    __shared__ float halo[kBuHaloPix];
    __shared__ unsigned long long keys[kBuTilePix];
    const int tile = blockIdx.x, k = blockIdx.y, n = blockIdx.z;
    const int kf = FLIP ? fl->index[k] : k;  // uniform per workgroup
    const int ty0 = (tile / p.tiles_x) * kBuTileH, tx0 = (tile % p.tiles_x) * kBuTileW;
    const int r = p.r, hw = kBuTileW + 2 * r, hh = kBuTileH + 2 * r;

    for (int i = threadIdx.x; i < hh * hw; i += kBuThreads) {
        const int y = ty0 + i / hw - r, x = tx0 + i % hw - r;
        float v = -INFINITY;
        if (y >= 0 && y < p.h && x >= 0 && x < p.w) v = MULTI ? aggregate_runs<FLIP>(p, *rs, n, k, kf, y, x) : aggregate<FLIP>(p, fl, n, k, kf, y, x);
        halo[i] = v;
    }
    __syncthreads();

    // tags of this tile: joint k writes tag channel k (tag_per_joint) or joint 0 writes the single channel
    const bool tags_here = p.tag_per_joint || k == 0;
    const int kt = p.tag_per_joint ? k : 0;
    const size_t plane = (size_t)p.h * p.w;
#pragma unroll
    for (int q = 0; q < kBuTilePix / kBuThreads; ++q) {
        const int pix = (int)threadIdx.x + q * kBuThreads;
        const int ly = pix / kBuTileW, lx = pix % kBuTileW;
        const int y = ty0 + ly, x = tx0 + lx;
        unsigned long long key = 0;  // below every real key: pixels outside the map never win
        if (y < p.h && x < p.w) {
            const int flat = y * p.w + x;
            const float v = halo[(ly + r) * hw + lx + r];
            p.raw[((size_t)n * p.k + k) * plane + flat] = v;
            float mx = v;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) mx = fmaxf(mx, halo[(ly + r + dy) * hw + lx + r + dx]);
            key = topk_key(mx == v ? v : 0.0f, flat);
            if (tags_here) {
                float* tg = p.tagging + (((size_t)n * p.ktag + kt) * plane + flat) * p.num_tags;
                for (int i = 0; i < p.ns; ++i) {
                    const BuStage& s = p.st[i];
                    if (s.tag_slot < 0) continue;
                    tg[s.tag_slot] = resize_bilinear(stage_tap<kTapPlain>(s, nullptr, n, p.k + kt, 0), s.h, s.w, s.sy, s.sx, y, x);
                    if (FLIP)  // the mirrored run's tags take the second half of the axis, in the same stage order
                        tg[p.num_tags / 2 + s.tag_slot] =
                            resize_bilinear(stage_tap<kTapMirror>(s, fl->data[i], n, 0, p.k + kf), s.h, s.w, s.sy, s.sx, y, x);
                }
            }
        }
        keys[pix] = key;
    }
    __syncthreads();
    bitonic_sort_desc<kBuTilePix, kBuThreads>(keys);
    unsigned long long* out = p.slab + (((size_t)n * p.k + k) * p.tiles + tile) * p.m;
    for (int i = threadIdx.x; i < p.m; i += kBuThreads) out[i] = keys[i];
}

__global__ __launch_bounds__(kBuThreads) void bu_parse_kernel(BuParseParams p) { bu_parse_body<false, false>(p, nullptr, nullptr); }

__global__ __launch_bounds__(kBuThreads) void bu_parse_flip_kernel(BuParseParams p, BuFlip fl) {
    bu_parse_body<true, false>(p, &fl, nullptr);
}

template <bool FLIP>
__global__ __launch_bounds__(kBuThreads) void bu_parse_multi_kernel(BuParseParams p, BuFlip fl, BuRuns rs) {
    bu_parse_body<FLIP, true>(p, &fl, &rs);
}

// ResizeBilinear of whole planes with the decoder's own sample: V consecutive output pixels of a row per thread, one V * 4-byte store
template <int V>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ in, float* __restrict__ out, size_t total,
                                                              int ih, int iw, int oh, int ow, float sy, float sx) {
    const unsigned per_row = (unsigned)(ow / V);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / per_row, plane = row / (unsigned)oh;
        const int x = (int)(i - row * per_row) * V, y = (int)(row - plane * (unsigned)oh);
        const BuTap<kTapPlain> tap{in + plane * ((size_t)ih * iw), nullptr, iw};
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = resize_bilinear(tap, ih, iw, sy, sx, y, x + j);
        float* dst = out + row * (unsigned)ow + x;
        if constexpr (V == 4)
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        else
            dst[0] = v[0];
    }
}

struct BuGatherParams {
    const float* raw;
    const float* tagging;
    const unsigned long long* slab;
    int n, k, h, w, ktag, tag_per_joint, num_tags, m, tiles, shift;
    float* val_k;  // [N, K, M]
    float* ind_k;  // [N, K, M, 2]
    float* tag_k;  // [N, K, M, L]
};

__global__ __launch_bounds__(kBuMergeThreads) void bu_gather_kernel(BuGatherParams p) {
    __shared__ unsigned long long keys[kBuMergeKeys];
    __shared__ int by_index[kBuMaxM];
    const int k = blockIdx.x, n = blockIdx.y;
    const unsigned long long* src = p.slab + ((size_t)n * p.k + k) * p.tiles * p.m;
    const int total = p.tiles * p.m;
    // running top-M in keys[0, M); every pass fills the rest of the buffer with the next slab keys and sorts
    for (int pos = 0, front = 0; pos < total; front = p.m) {
        const int cnt = min(total - pos, kBuMergeKeys - front);
        for (int i = threadIdx.x; i < kBuMergeKeys - front; i += kBuMergeThreads) keys[front + i] = i < cnt ? src[pos + i] : 0ull;
        __syncthreads();
        bitonic_sort_desc<kBuMergeKeys, kBuMergeThreads>(keys);
        pos += cnt;
    }

    const int t = threadIdx.x;
    const size_t nk = (size_t)n * p.k + k;
    int flat = 0;
    if (t < p.m) {
        const unsigned long long key = keys[t];
        flat = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
        p.val_k[nk * p.m + t] = unordered_float((unsigned)(key >> 32));
        const int kt = p.tag_per_joint ? k : 0;
        const float* tg = p.tagging + (((size_t)n * p.ktag + kt) * p.h * p.w + flat) * p.num_tags;
        for (int l = 0; l < p.num_tags; ++l) p.tag_k[(nk * p.m + t) * p.num_tags + l] = tg[l];
        // rank of this pixel among the selected ones in flat-index order (indices are distinct)
        int rank = 0;
        for (int j = 0; j < p.m; ++j) rank += (int)(0xffffffffu - (unsigned)(keys[j] & 0xffffffffull)) < flat;
        by_index[rank] = flat;
    }
    __syncthreads();
    if (t < p.m) {
        float x = (float)(flat % p.w), y = (float)(flat / p.w);
        if (p.shift) {
            // value-order entry t takes the offset of the t-th smallest selected flat index (the reference's masked_select order)
            const int f = by_index[t];
            const int fx = f % p.w, fy = f / p.w;
            const float* plane = p.raw + nk * p.h * p.w;
            const float dx = (fx >= 1 && fx <= p.w - 2) ? plane[f + 1] - plane[f - 1] : 0.0f;
            const float dy = (fy >= 1 && fy <= p.h - 2) ? plane[f + p.w] - plane[f - p.w] : 0.0f;
            x = x + (float)((dx > 0.0f) - (dx < 0.0f)) * 0.25f;
            y = y + (float)((dy > 0.0f) - (dy < 0.0f)) * 0.25f;
        }
        p.ind_k[(nk * p.m + t) * 2 + 0] = x;
        p.ind_k[(nk * p.m + t) * 2 + 1] = y;
    }
}

// out[n] = a[n] followed by b[n], in 16-byte words when every size and pointer allows it, else in 4-byte words
template <typename T>
__global__ __launch_bounds__(256) void concat_kernel(const T* __restrict__ a, size_t aw, const T* __restrict__ b, size_t bw,
                                                     T* __restrict__ out, size_t total) {
    const size_t per = aw + bw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t img = i / per, o = i - img * per;
        out[i] = o < aw ? a[img * aw + o] : b[img * bw + (o - aw)];
    }
}

// out[r][0, w_out) = in[r][start, start + w_out) for every row r: a column band of an activation (one T = one pixel: a float of fp32
// NCHW or the 16-byte channel block of the c8 layout)
template <typename T>
__global__ __launch_bounds__(256) void col_slice_kernel(const T* __restrict__ in, int w_in, int start, T* __restrict__ out, int w_out,
                                                        size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / (unsigned)w_out, col = i - row * (unsigned)w_out;
        out[i] = in[row * (unsigned)w_in + start + col];
    }
}

// ---- refine_missing_joint on the device (bottomup_inferencer.py:189-250 of the reference).  One workgroup per (joint, person): over
// the H * W pixels of the joint's map of the person's image, the first arg-max in flat index of
//     heatmap_raw - rintf(sqrtf(sum_l (tag_l - mean_tag_l)^2))
// in fp32, the squares summed in l order (numpy's norm along the last axis; np.round = round half to even = rintf), then the
// winner's centre (+0.5) shifted +-0.25 by the two clamped neighbour comparisons and its heat-map value.  Every lane keeps the best
// (value, index) of its pixels, a wave shuffle reduce and an LDS merge pick the workgroup's; ties go to the lowest flat index
// (np.argmax).  Inputs are assumed finite.
constexpr int kBuRefineThreads = 256;

struct BuRefineParams {
    const float* raw;       // [N, K, H, W]
    const float* tagging;   // [N, KTAG, H, W, L]
    const float* mean_tag;  // [P, L]
    const int* person_img;  // [P]
    int n, k, h, w, ktag, tag_per_joint, num_tags;
    float* found;           // [P, K, 3]
};

__device__ __forceinline__ bool refine_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// The arg-max of one (joint, person) by a whole workgroup of kBuRefineThreads: plane = the joint's H x W map, tags = its tag map
// [H * W, L], mean = the person's mean tag.  True on thread 0 alone, with found = (x, y, value) of the winner.  Every thread of the
// workgroup calls it (it holds a barrier); wave_v / wave_i are kBuRefineThreads / kWave LDS words each.
template <int L>
__device__ __forceinline__ bool bu_refine_argmax(const float* __restrict__ plane, const float* __restrict__ tags, const float (&mean)[L],
                                                 int h, int w, float* wave_v, int* wave_i, float (&found)[3]) {
    const int hw = h * w;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < hw; i += kBuRefineThreads) {  // ascending per lane: '>' keeps the lane's first maximum
        float sum = 0.0f;
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const float d = tags[(size_t)i * L + l] - mean[l];
            sum = sum + d * d;
        }
        const float v = plane[i] - rintf(sqrtf(sum));
        if (v > bv) { bv = v; bi = i; }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ov = __shfl_down(bv, off, kWave);
        const int oi = __shfl_down(bi, off, kWave);
        if (refine_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) { wave_v[wave] = bv; wave_i[wave] = bi; }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int q = 1; q < kBuRefineThreads / kWave; ++q)
        if (refine_better(wave_v[q], wave_i[q], bv, bi)) { bv = wave_v[q]; bi = wave_i[q]; }
    if (bi >= hw) bi = 0;  // no finite value anywhere (outside the contract): stay inside the map
    const int y = bi / w, x = bi - y * w;
    float xs = (float)x + 0.5f, ys = (float)y + 0.5f;
    const float* row = plane + (size_t)y * w;
    xs += row[min(x + 1, w - 1)] > row[max(x - 1, 0)] ? 0.25f : -0.25f;
    ys += plane[(size_t)min(y + 1, h - 1) * w + x] > plane[(size_t)max(y - 1, 0) * w + x] ? 0.25f : -0.25f;
    found[0] = xs;
    found[1] = ys;
    found[2] = plane[bi];
    return true;
}

template <int L>
__global__ __launch_bounds__(kBuRefineThreads) void bu_refine_kernel(BuRefineParams p) {
    __shared__ float wave_v[kBuRefineThreads / kWave];
    __shared__ int wave_i[kBuRefineThreads / kWave];
    const int k = blockIdx.x, person = blockIdx.y;
    const int img = p.person_img[person];
    if (img < 0 || img >= p.n) return;  // (uniform per workgroup) an index outside the batch reads nothing
    const int hw = p.h * p.w;
    const float* __restrict__ plane = p.raw + ((size_t)img * p.k + k) * hw;
    const float* __restrict__ tags = p.tagging + ((size_t)img * p.ktag + (p.tag_per_joint ? k : 0)) * (size_t)hw * L;
    float mean[L];
#pragma unroll
    for (int l = 0; l < L; ++l) mean[l] = p.mean_tag[(size_t)person * L + l];
    float found[3];
    if (bu_refine_argmax<L>(plane, tags, mean, p.h, p.w, wave_v, wave_i, found)) {
        float* out = p.found + ((size_t)person * p.k + k) * 3;
        out[0] = found[0];
        out[1] = found[1];
        out[2] = found[2];
    }
}

// ---- the tail of a bottom-up batch on the persons the grouping kernel left in device memory (bottomup_inferencer.py:120-150 of the
// reference: the per-person score, then refine_missing_joint): two launches whose grids are sized from the capacity K * M, so that
// no host value depends on the person counts.  Every workgroup reads counts[img] (clamped to the capacity) and status[img] itself
// and exits for a person that does not exist or an image that was handed to the host function.
//
//   bu_finish_score_kernel<L>   one wave64 per (person, image): lane j holds joint j (K <= 64).  score = np.mean(person[:, 2]); mean tag
//                               = np.mean over the joints with value > 0 in joint order (a ballot compacts them into LDS) of the tag
//                               at ((int)x, (int)y), truncated toward zero and clamped as _refine_on_device clamps.  Both are numpy's
//                               float32 means, rule (b) of bottomup_match.hip: bu_numpy_sum below for a 1-D view (the value column; the
//                               tags with L == 1), a sequential sum in joint order per component for L >= 2, one division.
//   bu_finish_refine_kernel<L>  one workgroup per (joint, person, image), behind the first in stream order: the arg-max above, only
//                               where person[j, 2] == 0 and the person has a located joint; the reference's fill rule (winner's value
//                               > 0) writes person[j, 0:3] in place.  A (joint, person) pair is read and written by its own
//                               workgroup alone.
struct BuFinishParams {
    float* people;         // [N, K * M, K, 3 + L]
    const int* counts;     // [N]
    const int* status;     // [N]
    const float* raw;      // [N, K, H, W]
    const float* tagging;  // [N, KTAG, H, W, L]
    int k, groups, h, w, ktag, tag_per_joint;
    float* scores;         // [N, K * M]
    float* mean_tag;       // [N, K * M, L]
    int* located;          // [N, K * M]: joints with value > 0
};

// persons of image img that exist on the device: none for an image handed over, else counts[img] inside the capacity
__device__ __forceinline__ int bu_finish_count(const BuFinishParams& p, int img) {
    return p.status[img] != 0 ? 0 : min(max(p.counts[img], 0), p.groups);
}

// numpy's float32 sum of the n <= 64 values a[0 .. n) in LDS by one wave (n uniform), valid on lane 0: n < 8 sequential from 0;
// else lanes 0 .. 7 are the eight accumulators over the whole blocks of eight, combined pairwise by shuffles, the tail in order
__device__ __forceinline__ float bu_numpy_sum(const float* a, int n, int lane) {
    float res = 0.0f;
    if (n < 8) {
        for (int i = 0; i < n; ++i) res = res + a[i];
        return res;
    }
    const int j = lane & 7;
    float r = a[j];
    for (int i = 8; i + 8 <= n; i += 8) r = r + a[i + j];
    r = r + __shfl_down(r, 1, kWave);  // lanes 0, 2, 4, 6: r0 + r1, r2 + r3, r4 + r5, r6 + r7
    r = r + __shfl_down(r, 2, kWave);  // lanes 0, 4
    res = r + __shfl_down(r, 4, kWave);
    for (int i = n & ~7; i < n; ++i) res = res + a[i];
    return res;
}

// (int)v as numpy's astype(int32) truncates, clamped to [0, size - 1]; a NaN reads 0 and nothing leaves the map
__device__ __forceinline__ int bu_map_coord(float v, int size) {
    if (!(v == v)) return 0;
    return min(max((int)fminf(fmaxf(v, -2.0f), (float)size), 0), size - 1);
}

template <int L>
__global__ __launch_bounds__(kWave) void bu_finish_score_kernel(BuFinishParams p) {
    __shared__ float vals[kWave];
    __shared__ float tags[kWave][L];
    constexpr int W = 3 + L;
    const int person = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
    if (person >= bu_finish_count(p, img)) return;  // (uniform per workgroup)
    const size_t slot = (size_t)img * p.groups + person;
    const float* __restrict__ row = p.people + (slot * p.k + lane) * W;
    float x = 0.0f, y = 0.0f, v = 0.0f;
    if (lane < p.k) { x = row[0]; y = row[1]; v = row[2]; }
    vals[lane] = v;
    const bool has = lane < p.k && v > 0.0f;
    const unsigned long long mask = __ballot(has);
    const int located = __popcll(mask);
    if (has) {
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));  // joint order
        const int xi = bu_map_coord(x, p.w), yi = bu_map_coord(y, p.h);
        const float* __restrict__ t =
            p.tagging + ((((size_t)img * p.ktag + (p.tag_per_joint ? lane : 0)) * p.h + yi) * p.w + xi) * L;
#pragma unroll
        for (int l = 0; l < L; ++l) tags[pos][l] = t[l];
    }
    __syncthreads();
    const float total = bu_numpy_sum(vals, p.k, lane);
    if (lane == 0) {
        p.scores[slot] = total / (float)p.k;
        p.located[slot] = located;
    }
    if (located == 0) return;  // (grouping builds a person from at least one detection) no mean tag: the refinement skips it
    if (L == 1) {
        const float sum = bu_numpy_sum(&tags[0][0], located, lane);
        if (lane == 0) p.mean_tag[slot] = sum / (float)located;
    } else if (lane < L) {
        float sum = tags[0][lane];
        for (int i = 1; i < located; ++i) sum = sum + tags[i][lane];
        p.mean_tag[slot * L + lane] = sum / (float)located;
    }
}

template <int L>
__global__ __launch_bounds__(kBuRefineThreads) void bu_finish_refine_kernel(BuFinishParams p) {
    __shared__ float wave_v[kBuRefineThreads / kWave];
    __shared__ int wave_i[kBuRefineThreads / kWave];
    const int k = blockIdx.x, person = blockIdx.y, img = blockIdx.z;
    if (person >= bu_finish_count(p, img)) return;  // (every exit is uniform per workgroup)
    const size_t slot = (size_t)img * p.groups + person;
    float* joint = p.people + (slot * p.k + k) * (3 + L);
    if (!(joint[2] == 0.0f) || p.located[slot] == 0) return;  // a located joint stays; a person without any has no mean tag
    const int hw = p.h * p.w;
    const float* __restrict__ plane = p.raw + ((size_t)img * p.k + k) * hw;
    const float* __restrict__ tags = p.tagging + ((size_t)img * p.ktag + (p.tag_per_joint ? k : 0)) * (size_t)hw * L;
    float mean[L];
#pragma unroll
    for (int l = 0; l < L; ++l) mean[l] = p.mean_tag[slot * L + l];
    float found[3];
    if (bu_refine_argmax<L>(plane, tags, mean, p.h, p.w, wave_v, wave_i, found) && found[2] > 0.0f) {
        joint[0] = found[0];
        joint[1] = found[1];
        joint[2] = found[2];
    }
}

// the grouping entry's limits (bottomup_match.hip): what people [N, K * M, K, 3 + L] can hold
static bool bu_finish_in_limits(int k, int m, int num_tags) { return k <= 64 && m <= kBuMaxM && num_tags <= kBuMaxTags && k * m <= 1024; }

static int bu_tiles_x(int w) { return (w + kBuTileW - 1) / kBuTileW; }
static int bu_tiles(int h, int w) { return bu_tiles_x(w) * ((h + kBuTileH - 1) / kBuTileH); }

}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_bottomup_workspace_bytes(int n, int k, int h, int w, int max_num) {
    if (n <= 0 || k <= 0 || h <= 0 || w <= 0 || max_num <= 0) return 0;
    return (size_t)n * k * bu_tiles(h, w) * max_num * sizeof(unsigned long long);
}

// Validates the arguments of a parse entry and fills the kernel parameters; tags_per_stage = 1, or 2 for the flip form, whose
// every tag stage also contributes the mirrored run's tags.
static int bu_parse_params(const mp_bottomup_stage* stages, int num_stages, const uint8_t* mask_dev, int mask_h, int mask_w, int n, int k,
                           int tag_per_joint, int nms_kernel, int max_num, float* heatmap_raw_dev, float* tagging_dev,
                           void* workspace_dev, size_t workspace_bytes, int tags_per_stage, BuParseParams& p) {
    if (!stages || !mask_dev || !heatmap_raw_dev || !tagging_dev) return MP_ERR_NULL;
    if (num_stages < 1 || num_stages > kBuMaxStages || n <= 0 || k <= 0 || mask_h <= 0 || mask_w <= 0) return MP_ERR_SHAPE;
    if (nms_kernel != 1 && nms_kernel != 3 && nms_kernel != 5 && nms_kernel != 7) return MP_ERR_UNSUPPORTED;
    if (max_num < 1 || max_num > kBuMaxM) return MP_ERR_UNSUPPORTED;
    const mp_bottomup_stage& full = stages[num_stages - 1];
    p.h = full.h;
    p.w = full.w;
    if (p.h <= 0 || p.w <= 0 || (size_t)p.h * p.w > 0x7fffffffu || max_num > p.h * p.w) return MP_ERR_SHAPE;
    p.ktag = tag_per_joint ? k : 1;
    int slot = 0;
    for (int i = 0; i < num_stages; ++i) {
        const mp_bottomup_stage& s = stages[i];
        if (!s.data_dev) return MP_ERR_NULL;
        if (s.h <= 0 || s.w <= 0 || s.c < k) return MP_ERR_SHAPE;
        if (s.has_tags && s.c - k != p.ktag) return MP_ERR_SHAPE;
        p.st[i] = BuStage{s.data_dev, s.c, s.h, s.w, s.has_tags ? slot : -1, (float)s.h / (float)p.h, (float)s.w / (float)p.w};
        slot += s.has_tags ? 1 : 0;
    }
    if (slot == 0 || slot * tags_per_stage > kBuMaxTags) return MP_ERR_UNSUPPORTED;
    const size_t need = mp_bottomup_workspace_bytes(n, k, p.h, p.w, max_num);
    if (!workspace_dev || workspace_bytes < need) return MP_ERR_WORKSPACE;
    p.ns = num_stages;
    p.mask = mask_dev;
    p.mh = mask_h;
    p.mw = mask_w;
    p.msy = (float)mask_h / (float)p.h;
    p.msx = (float)mask_w / (float)p.w;
    p.n = n;
    p.k = k;
    p.tag_per_joint = tag_per_joint ? 1 : 0;
    p.num_tags = slot * tags_per_stage;
    p.r = nms_kernel / 2;
    p.m = max_num;
    p.tiles_x = bu_tiles_x(p.w);
    p.tiles = bu_tiles(p.h, p.w);
    p.raw = heatmap_raw_dev;
    p.tagging = tagging_dev;
    p.slab = reinterpret_cast<unsigned long long*>(workspace_dev);
    if (n > 65535 || k > 65535) return MP_ERR_SHAPE;
    return MP_OK;
}

int mp_bottomup_parse_nms_topk(const mp_bottomup_stage* stages, int num_stages, const uint8_t* mask_dev, int mask_h, int mask_w,
                               int n, int k, int tag_per_joint, int nms_kernel, int max_num, float* heatmap_raw_dev,
                               float* tagging_dev, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream) {
    BuParseParams p{};
    const int rc = bu_parse_params(stages, num_stages, mask_dev, mask_h, mask_w, n, k, tag_per_joint, nms_kernel, max_num,
                                   heatmap_raw_dev, tagging_dev, workspace_dev, workspace_bytes, 1, p);
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(bu_parse_kernel, dim3((unsigned)p.tiles, (unsigned)k, (unsigned)n), dim3(kBuThreads), 0, as_stream(stream), p);
    return check_launch();
}

int mp_bottomup_parse_nms_topk_flip(const mp_bottomup_stage* stages, const mp_bottomup_stage* flipped_stages,
                                    const int32_t* flip_index_host, int num_stages, const uint8_t* mask_dev, int mask_h, int mask_w,
                                    int n, int k, int tag_per_joint, int nms_kernel, int max_num, float* heatmap_raw_dev,
                                    float* tagging_dev, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream) {
    if (!stages || !flipped_stages || !flip_index_host) return MP_ERR_NULL;
    if (k <= 0) return MP_ERR_SHAPE;
    if (!tag_per_joint || k > kBuFlipMaxJoints) return MP_ERR_UNSUPPORTED;
    BuFlip fl{};
    for (int j = 0; j < k; ++j) {  // the kernel indexes the mirrored stages with these: none may leave [0, k)
        if (flip_index_host[j] < 0 || flip_index_host[j] >= k) return MP_ERR_SHAPE;
        fl.index[j] = flip_index_host[j];
    }
    BuParseParams p{};
    const int rc = bu_parse_params(stages, num_stages, mask_dev, mask_h, mask_w, n, k, tag_per_joint, nms_kernel, max_num,
                                   heatmap_raw_dev, tagging_dev, workspace_dev, workspace_bytes, 2, p);
    if (rc != MP_OK) return rc;
    for (int i = 0; i < num_stages; ++i) {
        const mp_bottomup_stage& s = stages[i];
        const mp_bottomup_stage& f = flipped_stages[i];
        if (!f.data_dev) return MP_ERR_NULL;
        if (f.c != s.c || f.h != s.h || f.w != s.w || (f.has_tags != 0) != (s.has_tags != 0)) return MP_ERR_SHAPE;
        fl.data[i] = f.data_dev;
    }
    hipLaunchKernelGGL(bu_parse_flip_kernel, dim3((unsigned)p.tiles, (unsigned)k, (unsigned)n), dim3(kBuThreads), 0, as_stream(stream),
                       p, fl);
    return check_launch();
}

int mp_bottomup_parse_nms_topk_multi(const mp_bottomup_run* runs_host, int num_runs, int base_run, const int32_t* flip_index_host,
                                     int num_stages, const uint8_t* mask_dev, int mask_h, int mask_w, int n, int k,
                                     int tag_per_joint, int nms_kernel, int max_num, float* heatmap_raw_dev, float* tagging_dev,
                                     void* workspace_dev, size_t workspace_bytes, mp_stream_t stream) {
    if (!runs_host) return MP_ERR_NULL;
    if (num_runs < 1 || num_runs > kBuMaxRuns || base_run < 0 || base_run >= num_runs) return MP_ERR_SHAPE;
    const bool flip = runs_host[0].flipped != nullptr;
    for (int r = 0; r < num_runs; ++r) {
        if (!runs_host[r].stages) return MP_ERR_NULL;
        if ((runs_host[r].flipped != nullptr) != flip) return MP_ERR_SHAPE;  // the flip test covers every run or none
    }
    if (flip != (flip_index_host != nullptr)) return MP_ERR_NULL;
    BuFlip fl{};
    if (flip) {
        if (k <= 0) return MP_ERR_SHAPE;
        if (!tag_per_joint || k > kBuFlipMaxJoints) return MP_ERR_UNSUPPORTED;
        for (int j = 0; j < k; ++j) {  // the kernel indexes the mirrored stages with these: none may leave [0, k)
            if (flip_index_host[j] < 0 || flip_index_host[j] >= k) return MP_ERR_SHAPE;
            fl.index[j] = flip_index_host[j];
        }
    }
    const mp_bottomup_stage* base = runs_host[base_run].stages;
    BuParseParams p{};
    const int rc = bu_parse_params(base, num_stages, mask_dev, mask_h, mask_w, n, k, tag_per_joint, nms_kernel, max_num,
                                   heatmap_raw_dev, tagging_dev, workspace_dev, workspace_bytes, flip ? 2 : 1, p);
    if (rc != MP_OK) return rc;
    BuRuns rs{};
    rs.num_runs = num_runs;
    rs.base = base_run;
    for (int r = 0; r < num_runs; ++r)
        for (int i = 0; i < num_stages; ++i) {
            const mp_bottomup_stage& s = runs_host[r].stages[i];
            if (!s.data_dev) return MP_ERR_NULL;
            if (s.h <= 0 || s.w <= 0 || (size_t)s.h * s.w > 0x7fffffffu) return MP_ERR_SHAPE;
            if (s.c != base[i].c || (s.has_tags != 0) != (base[i].has_tags != 0)) return MP_ERR_SHAPE;
            rs.st[r][i] = BuStage{s.data_dev, s.c, s.h, s.w, -1, (float)s.h / (float)p.h, (float)s.w / (float)p.w};
            if (!flip) continue;
            const mp_bottomup_stage& f = runs_host[r].flipped[i];
            if (!f.data_dev) return MP_ERR_NULL;
            if (f.c != s.c || f.h != s.h || f.w != s.w || (f.has_tags != 0) != (s.has_tags != 0)) return MP_ERR_SHAPE;
            rs.flipped[r][i] = f.data_dev;
            if (r == base_run) fl.data[i] = f.data_dev;
        }
    const dim3 grid((unsigned)p.tiles, (unsigned)k, (unsigned)n);
    if (flip)
        hipLaunchKernelGGL(bu_parse_multi_kernel<true>, grid, dim3(kBuThreads), 0, as_stream(stream), p, fl, rs);
    else
        hipLaunchKernelGGL(bu_parse_multi_kernel<false>, grid, dim3(kBuThreads), 0, as_stream(stream), p, fl, rs);
    return check_launch();
}

int mp_resize_bilinear_nchw(const float* in_dev, float* out_dev, int planes, int ih, int iw, int oh, int ow, mp_stream_t stream) {
    if (!in_dev || !out_dev) return MP_ERR_NULL;
    if (planes <= 0 || ih <= 0 || iw <= 0 || oh <= 0 || ow <= 0) return MP_ERR_SHAPE;
    if ((size_t)ih * iw > 0x7fffffffu || (size_t)oh * ow > 0x7fffffffu) return MP_ERR_SHAPE;
    const float sy = (float)ih / (float)oh, sx = (float)iw / (float)ow;
    const bool wide = ow % 4 == 0 && (uintptr_t)out_dev % 16 == 0;
    const size_t total = (size_t)planes * oh * (wide ? ow / 4 : ow);
    size_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (wide)
        hipLaunchKernelGGL(resize_bilinear_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), in_dev, out_dev, total, ih,
                           iw, oh, ow, sy, sx);
    else
        hipLaunchKernelGGL(resize_bilinear_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), in_dev, out_dev, total, ih,
                           iw, oh, ow, sy, sx);
    return check_launch();
}

int mp_bottomup_gather(const float* heatmap_raw_dev, const float* tagging_dev, const void* workspace_dev, size_t workspace_bytes,
                       int n, int k, int h, int w, int tag_per_joint, int num_tags, int max_num, int shift_coordinate,
                       float* val_k_dev, float* ind_k_dev, float* tag_k_dev, mp_stream_t stream) {
    if (!heatmap_raw_dev || !tagging_dev || !val_k_dev || !ind_k_dev || !tag_k_dev) return MP_ERR_NULL;
    if (n <= 0 || k <= 0 || h <= 0 || w <= 0 || (size_t)h * w > 0x7fffffffu) return MP_ERR_SHAPE;
    if (max_num < 1 || max_num > kBuMaxM || num_tags < 1 || num_tags > kBuMaxTags) return MP_ERR_UNSUPPORTED;
    if (max_num > h * w || n > 65535 || k > 65535) return MP_ERR_SHAPE;
    const size_t need = mp_bottomup_workspace_bytes(n, k, h, w, max_num);
    if (!workspace_dev || workspace_bytes < need) return MP_ERR_WORKSPACE;
    BuGatherParams p{};
    p.raw = heatmap_raw_dev;
    p.tagging = tagging_dev;
    p.slab = reinterpret_cast<const unsigned long long*>(workspace_dev);
    p.n = n;
    p.k = k;
    p.h = h;
    p.w = w;
    p.ktag = tag_per_joint ? k : 1;
    p.tag_per_joint = tag_per_joint ? 1 : 0;
    p.num_tags = num_tags;
    p.m = max_num;
    p.tiles = bu_tiles(h, w);
    p.shift = shift_coordinate ? 1 : 0;
    p.val_k = val_k_dev;
    p.ind_k = ind_k_dev;
    p.tag_k = tag_k_dev;
    hipLaunchKernelGGL(bu_gather_kernel, dim3((unsigned)k, (unsigned)n), dim3(kBuMergeThreads), 0, as_stream(stream), p);
    return check_launch();
}

int mp_bottomup_refine_missing(const float* heatmap_raw_dev, const float* tagging_dev, const float* mean_tag_dev,
                               const int* person_image_dev, int num_persons, int n, int k, int h, int w, int tag_per_joint,
                               int num_tags, float* found_dev, mp_stream_t stream) {
    if (num_persons == 0) return MP_OK;  // nobody to refine: no launch
    if (!heatmap_raw_dev || !tagging_dev || !mean_tag_dev || !person_image_dev || !found_dev) return MP_ERR_NULL;
    if (num_persons < 0 || n <= 0 || k <= 0 || h <= 0 || w <= 0 || (size_t)h * w > 0x7fffffffu) return MP_ERR_SHAPE;
    if (num_tags < 1 || num_tags > kBuMaxTags) return MP_ERR_UNSUPPORTED;
    if (num_persons > 65535) return MP_ERR_SHAPE;
    BuRefineParams p{};
    p.raw = heatmap_raw_dev;
    p.tagging = tagging_dev;
    p.mean_tag = mean_tag_dev;
    p.person_img = person_image_dev;
    p.n = n;
    p.k = k;
    p.h = h;
    p.w = w;
    p.ktag = tag_per_joint ? k : 1;
    p.tag_per_joint = tag_per_joint ? 1 : 0;
    p.num_tags = num_tags;
    p.found = found_dev;
    const dim3 grid((unsigned)k, (unsigned)num_persons), block(kBuRefineThreads);
    switch (num_tags) {
        case 1: hipLaunchKernelGGL(bu_refine_kernel<1>, grid, block, 0, as_stream(stream), p); break;
        case 2: hipLaunchKernelGGL(bu_refine_kernel<2>, grid, block, 0, as_stream(stream), p); break;
        case 3: hipLaunchKernelGGL(bu_refine_kernel<3>, grid, block, 0, as_stream(stream), p); break;
        default: hipLaunchKernelGGL(bu_refine_kernel<4>, grid, block, 0, as_stream(stream), p); break;
    }
    return check_launch();
}

size_t mp_bottomup_finish_workspace_bytes(int n, int k, int m, int num_tags) {
    if (n <= 0 || k <= 0 || m <= 0 || num_tags <= 0 || !bu_finish_in_limits(k, m, num_tags)) return 0;
    return (size_t)n * k * m * (num_tags + 1) * sizeof(float);  // the mean tags, then the located-joint counts
}

int mp_bottomup_finish_people(float* people_dev, const int* counts_dev, const int* status_dev, const float* heatmap_raw_dev,
                              const float* tagging_dev, int n, int k, int m, int h, int w, int tag_per_joint, int num_tags, int refine,
                              float* scores_dev, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream) {
    if (n == 0) return MP_OK;  // no image: no launch
    if (!people_dev || !counts_dev || !status_dev || !heatmap_raw_dev || !tagging_dev || !scores_dev) return MP_ERR_NULL;
    if (n < 0 || n > 65535 || k <= 0 || m <= 0 || h <= 0 || w <= 0 || num_tags <= 0 || (size_t)h * w > 0x7fffffffu) return MP_ERR_SHAPE;
    if (!bu_finish_in_limits(k, m, num_tags)) return MP_ERR_UNSUPPORTED;
    const size_t need = mp_bottomup_finish_workspace_bytes(n, k, m, num_tags);
    if (!workspace_dev || workspace_bytes < need) return MP_ERR_WORKSPACE;
    BuFinishParams p{};
    p.people = people_dev;
    p.counts = counts_dev;
    p.status = status_dev;
    p.raw = heatmap_raw_dev;
    p.tagging = tagging_dev;
    p.k = k;
    p.groups = k * m;
    p.h = h;
    p.w = w;
    p.ktag = tag_per_joint ? k : 1;
    p.tag_per_joint = tag_per_joint ? 1 : 0;
    p.scores = scores_dev;
    p.mean_tag = reinterpret_cast<float*>(workspace_dev);
    p.located = reinterpret_cast<int*>(p.mean_tag + (size_t)n * p.groups * num_tags);
    const dim3 persons((unsigned)p.groups, (unsigned)n), pairs((unsigned)k, (unsigned)p.groups, (unsigned)n);
    switch (num_tags) {
        case 1: hipLaunchKernelGGL(bu_finish_score_kernel<1>, persons, dim3(kWave), 0, as_stream(stream), p); break;
        case 2: hipLaunchKernelGGL(bu_finish_score_kernel<2>, persons, dim3(kWave), 0, as_stream(stream), p); break;
        case 3: hipLaunchKernelGGL(bu_finish_score_kernel<3>, persons, dim3(kWave), 0, as_stream(stream), p); break;
        default: hipLaunchKernelGGL(bu_finish_score_kernel<4>, persons, dim3(kWave), 0, as_stream(stream), p); break;
    }
    const int rc = check_launch();
    if (rc != MP_OK || !refine) return rc;
    switch (num_tags) {
        case 1: hipLaunchKernelGGL(bu_finish_refine_kernel<1>, pairs, dim3(kBuRefineThreads), 0, as_stream(stream), p); break;
        case 2: hipLaunchKernelGGL(bu_finish_refine_kernel<2>, pairs, dim3(kBuRefineThreads), 0, as_stream(stream), p); break;
        case 3: hipLaunchKernelGGL(bu_finish_refine_kernel<3>, pairs, dim3(kBuRefineThreads), 0, as_stream(stream), p); break;
        default: hipLaunchKernelGGL(bu_finish_refine_kernel<4>, pairs, dim3(kBuRefineThreads), 0, as_stream(stream), p); break;
    }
    return check_launch();
}

int mp_concat_channels(const void* a_dev, int ca, const void* b_dev, int cb, void* out_dev, int n, int h, int w, int c8,
                       mp_stream_t stream) {
    if (!a_dev || !b_dev || !out_dev) return MP_ERR_NULL;
    if (n <= 0 || ca <= 0 || cb <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    if (c8 && ca % 8 != 0) return MP_ERR_UNSUPPORTED;  // the second part must start on an 8-channel block
    const size_t hw = (size_t)h * w;
    // bytes per image of each part: fp32 NCHW planes, or whole [H][W][8] fp16 blocks (the pad channels of b's last block are zero)
    const size_t ab = c8 ? (size_t)(ca / 8) * hw * 16 : (size_t)ca * hw * 4;
    const size_t bb = c8 ? (size_t)((cb + 7) / 8) * hw * 16 : (size_t)cb * hw * 4;
    const bool wide = ab % 16 == 0 && bb % 16 == 0 && ((uintptr_t)a_dev | (uintptr_t)b_dev | (uintptr_t)out_dev) % 16 == 0;
    const size_t unit = wide ? 16 : 4;
    const size_t total = (size_t)n * (ab + bb) / unit;
    size_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (wide)
        hipLaunchKernelGGL(concat_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const uint4*)a_dev, ab / 16,
                           (const uint4*)b_dev, bb / 16, (uint4*)out_dev, total);
    else
        hipLaunchKernelGGL(concat_kernel<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const uint32_t*)a_dev,
                           ab / 4, (const uint32_t*)b_dev, bb / 4, (uint32_t*)out_dev, total);
    return check_launch();
}

int mp_col_slice(const void* in_dev, void* out_dev, int rows, int w_in, int start, int w_out, int c8, mp_stream_t stream) {
    if (!in_dev || !out_dev) return MP_ERR_NULL;
    if (rows <= 0 || w_in <= 0 || w_out <= 0 || start < 0 || start + w_out > w_in) return MP_ERR_SHAPE;
    const size_t total = (size_t)rows * w_out;
    size_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    if (c8)
        hipLaunchKernelGGL(col_slice_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const uint4*)in_dev, w_in,
                           start, (uint4*)out_dev, w_out, total);
    else
        hipLaunchKernelGGL(col_slice_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const float*)in_dev, w_in,
                           start, (float*)out_dev, w_out, total);
    return check_launch();
}

}  // extern "C"
