// Bottom-up training masks on the device (reference: mindpose/data/dataset/coco_bottomup.py:146-189 _get_encoded_mask, a start-up
// pass over the whole training set through pycocotools.mask.decode and cv2.erode; here per batch, two launches).
//   launch 1, row_clearance_kernel: one workgroup per image row.  Every pixel finds, in each region of its image, the run that holds
//     its column-major index x * H + y by binary search over the region's prefix sums - an odd run is ones - so the raster is a
//     GATHER: no scatter, no memset pass, no atomics.  The row's invalid flags meet in LDS as one 64-bit ballot word per 64 pixels;
//     clear(y, x) = min(255, distance to the nearest set bit) then comes from count-leading / trailing-zeros over at most five
//     words each way, and leaves as one byte per pixel (one dword per four where the row allows it).
//   launch 2, erode_kernel: a pixel is valid in stage i iff clear(y + d, x) > half_width_i[|d|] for every in-image row y + d - the
//     erosion by a disc given as per-row half widths, rows outside the image valid (cv2.erode's default border).  Every stage reads the
//     same clearance plane, a stage only the rows inside its own radius, compared two pixels at a time; every output byte is written once.  An image without regions never
//     reads the workspace: its planes are ones.
// All of it is integer arithmetic on the tables, so no result depends on the thread mapping.
#include "common.h"

namespace mp {
namespace {

constexpr int kMaskMaxStages = 8;     // radii and half widths travel in the kernel arguments
constexpr int kMaskMaxRadius = 127;   // a half width must stay below the saturated clearance
constexpr int kMaskMaxExtent = 16384; // 256 ballot words of LDS per row; H * W stays far inside uint32
constexpr int kMaskFar = 255;

struct MaskParams {
    const uint32_t* prefix;
    const int* region_ptr;
    const int* image_tab;       // [n][4]: H, W, first region, number of regions
    const long long* offsets;   // [n][2]: out, workspace
    uint8_t* out;
    uint8_t* clear;
    int s, rmax;
    int radius[kMaskMaxStages];
    uint8_t hw[kMaskMaxStages][kMaskMaxRadius + 1];
};

// true when index idx lies in a run of ones of the region whose inclusive prefix sums are p[0 .. m): the first j with p[j] > idx is
// the run (p[m - 1] = H * W > idx, checked on the host), odd runs are ones.  Most pixels of an image lie before a region's first
// ones or behind its last: those two runs are answered from one load each, without the search.
__device__ __forceinline__ bool region_covers(const uint32_t* __restrict__ p, int m, uint32_t idx) {
    if (idx < p[0]) return false;
    if (m >= 2 && idx >= p[m - 2]) return ((m - 1) & 1) != 0;
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p[mid] > idx) hi = mid; else lo = mid + 1;
    }
    return (lo & 1) != 0;
}

// distance from pixel x to the nearest set bit of the row's words, saturated
__device__ __forceinline__ int clearance(const unsigned long long* words, int nwords, int x) {
    const int w = x >> 6, b = x & 63;
    int best = kMaskFar;
    unsigned long long m = words[w] & (~0ull >> (63 - b));  // bits 0 .. b
    if (m) best = b - (63 - __clzll((long long)m));
    else
        for (int k = 1; k <= 4 && w - k >= 0; ++k) {
            m = words[w - k];
            if (m) { best = b + 64 * k - (63 - __clzll((long long)m)); break; }
        }
    m = words[w] & (~0ull << b);  // bits b .. 63
    int right = kMaskFar;
    if (m) right = (__ffsll((unsigned long long)m) - 1) - b;
    else
        for (int k = 1; k <= 4 && w + k < nwords; ++k) {
            m = words[w + k];
            if (m) { right = 64 * k + (__ffsll((unsigned long long)m) - 1) - b; break; }
        }
    best = right < best ? right : best;
    return best > kMaskFar ? kMaskFar : best;
}

// four adjacent pixels leave by one dword: the row width and both base addresses of the image must allow it
__device__ __forceinline__ bool wide_image(const MaskParams& p, int W, long long out_off, long long clear_off) {
    return (W & 3) == 0 && ((uintptr_t)(p.out + out_off) & 3) == 0 && ((uintptr_t)(p.clear + clear_off) & 3) == 0;
}

__global__ __launch_bounds__(256) void row_clearance_kernel(MaskParams p) {
    const int n = blockIdx.y, y = blockIdx.x;
    const int H = p.image_tab[4 * n], W = p.image_tab[4 * n + 1], r0 = p.image_tab[4 * n + 2], nr = p.image_tab[4 * n + 3];
    if (y >= H || nr == 0) return;  // uniform over the workgroup
    __shared__ unsigned long long words[kMaskMaxExtent / 64];
    const int nwords = (W + 63) >> 6;
    for (int x0 = 0; x0 < W; x0 += 256) {  // every wave of the workgroup takes part in every ballot
        const int x = x0 + (int)threadIdx.x;
        bool invalid = false;
        if (x < W) {
            const uint32_t idx = (uint32_t)x * (uint32_t)H + (uint32_t)y;
            for (int r = r0; r < r0 + nr && !invalid; ++r) {
                const int a = p.region_ptr[r];
                invalid = region_covers(p.prefix + a, p.region_ptr[r + 1] - a, idx);
            }
        }
        const unsigned long long bits = __ballot(invalid);
        const int word = (x0 >> 6) + ((int)threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0 && word < nwords) words[word] = bits;
    }
    __syncthreads();
    const long long out_off = p.offsets[2 * n], clear_off = p.offsets[2 * n + 1];
    uint8_t* __restrict__ row = p.clear + clear_off + (size_t)y * W;
    if (wide_image(p, W, out_off, clear_off)) {
        for (int g = threadIdx.x; g < (W >> 2); g += 256) {
            const int x = g * 4;
            *reinterpret_cast<uchar4*>(row + x) = make_uchar4((uint8_t)clearance(words, nwords, x), (uint8_t)clearance(words, nwords, x + 1),
                                                              (uint8_t)clearance(words, nwords, x + 2), (uint8_t)clearance(words, nwords, x + 3));
        }
    } else {
        for (int x = threadIdx.x; x < W; x += 256) row[x] = (uint8_t)clearance(words, nwords, x);
    }
}

// VEC adjacent pixels of one row, stage after stage.  The clearance bytes of a row ride two registers as 16-bit lanes (pixels 0 and
// 2 in `even`, 1 and 3 in `odd`), so one subtraction compares two pixels with a half width: (0x8000 + c) - (h + 1) keeps bit 15 of
// its lane iff c > h, and no lane borrows from its neighbour (c <= 255, h + 1 <= 128).  A stage's pixels stay valid while the AND
// over its rows keeps that bit.  The rows are read kMaskRowBatch at a time, all loads issued before the first compare; a row
// outside the image or beyond the stage's radius reads as "far", and the table holds 0 there, so neither clears a bit.
// `terms` is the workgroup's LDS copy of the discs: terms[i][d] = (half_width_i[d] + 1) in both lanes, 0 beyond the radius.
constexpr int kMaskRowBatch = 8;
constexpr int kMaskTermRow = kMaskMaxRadius + 1 + kMaskRowBatch;  // a batch may run up to kMaskRowBatch - 1 rows past the radius

template <int VEC>
__device__ __forceinline__ void erode_group(const MaskParams& p, const uint32_t (*terms)[kMaskTermRow], const uint8_t* __restrict__ clear,
                                            uint8_t* __restrict__ out, int H, int W, bool has_regions, int y, int x) {
    constexpr uint32_t kTop = 0x80008000u;
    for (int i = 0; i < p.s; ++i) {
        const int r = p.radius[i];
        uint32_t even = kTop, odd = kTop;
        for (int d0 = -r; d0 <= r && has_regions; d0 += kMaskRowBatch) {
            uint32_t c[kMaskRowBatch];
#pragma unroll
            for (int j = 0; j < kMaskRowBatch; ++j) {
                const int yy = y + d0 + j;
                c[j] = 0xFFFFFFFFu;
                if (d0 + j <= r && yy >= 0 && yy < H) {
                    if constexpr (VEC == 4) c[j] = *reinterpret_cast<const uint32_t*>(clear + (size_t)yy * W + x);
                    else c[j] = 0xFFFFFF00u | clear[(size_t)yy * W + x];
                }
            }
#pragma unroll
            for (int j = 0; j < kMaskRowBatch; ++j) {
                const uint32_t h1 = terms[i][d0 + j < 0 ? -(d0 + j) : d0 + j];  // one address for the whole wave
                even &= ((c[j] & 0x00FF00FFu) | kTop) - h1;
                odd &= (((c[j] >> 8) & 0x00FF00FFu) | kTop) - h1;
            }
        }
        uint8_t* o = out + ((size_t)i * H + y) * W + x;
        const uint32_t bytes = ((even >> 15) & 0x00010001u) | (((odd >> 15) & 0x00010001u) << 8);  // pixels 0 .. 3 as bytes 0 .. 3
        if constexpr (VEC == 4) *reinterpret_cast<uint32_t*>(o) = bytes;
        else o[0] = (uint8_t)(bytes & 1u);
    }
}

// a workgroup owns 16 rows x 16 thread-groups (64 or 16 pixels wide): the 16 + 2 rmax clearance rows it reads stay in the L1
__global__ __launch_bounds__(256) void erode_kernel(MaskParams p) {
    const int n = blockIdx.z;
    const int H = p.image_tab[4 * n], W = p.image_tab[4 * n + 1], nr = p.image_tab[4 * n + 3];
    if ((int)blockIdx.y * 16 >= H) return;  // uniform over the workgroup
    __shared__ uint32_t terms[kMaskMaxStages][kMaskTermRow];
    for (int t = threadIdx.x; t < p.s * kMaskTermRow; t += 256) {
        const int i = t / kMaskTermRow, d = t - i * kMaskTermRow;
        terms[i][d] = d <= p.radius[i] ? ((uint32_t)p.hw[i][d] + 1u) * 0x00010001u : 0u;
    }
    __syncthreads();
    const int y = blockIdx.y * 16 + ((int)threadIdx.x >> 4), g = blockIdx.x * 16 + ((int)threadIdx.x & 15);
    if (y >= H) return;
    const long long out_off = p.offsets[2 * n], clear_off = p.offsets[2 * n + 1];
    if (wide_image(p, W, out_off, clear_off)) {
        if (g * 4 < W) erode_group<4>(p, terms, p.clear + clear_off, p.out + out_off, H, W, nr != 0, y, g * 4);
    } else {
        if (g < W) erode_group<1>(p, terms, p.clear + clear_off, p.out + out_off, H, W, nr != 0, y, g);
    }
}

}  // namespace
}  // namespace mp

extern "C" int mp_bottomup_train_masks(const uint32_t* prefix_host, const int* region_ptr_host, const int* image_tab_host,
                                       const long long* offsets_host, const uint32_t* prefix_dev, const int* region_ptr_dev,
                                       const int* image_tab_dev, const long long* offsets_dev, const int* radii_host,
                                       const uint8_t* half_widths_host, uint8_t* out, size_t out_bytes, uint8_t* workspace,
                                       size_t workspace_bytes, int n, int s, mp_stream_t stream) {
    using namespace mp;
    if (!prefix_host || !region_ptr_host || !image_tab_host || !offsets_host || !prefix_dev || !region_ptr_dev || !image_tab_dev ||
        !offsets_dev || !radii_host || !half_widths_host || !out || !workspace)
        return MP_ERR_NULL;
    if (s < 1 || s > kMaskMaxStages) return MP_ERR_UNSUPPORTED;
    MaskParams p{};
    for (int i = 0; i < s; ++i) {
        const int r = radii_host[i];
        if (r < 0 || r > kMaskMaxRadius) return MP_ERR_UNSUPPORTED;
        p.radius[i] = r;
        p.rmax = r > p.rmax ? r : p.rmax;
        for (int d = 0; d <= r; ++d) {
            const int h = half_widths_host[i * (kMaskMaxRadius + 1) + d];
            if (h > kMaskMaxRadius) return MP_ERR_UNSUPPORTED;
            p.hw[i][d] = (uint8_t)h;
        }
    }
    if (n <= 0 || n > 65535) return MP_ERR_SHAPE;
    int hmax = 0, wmax = 0, next_region = 0;
    bool all_wide = true;  // wide_image() of every image: the kernels decide per image, the grid is sized by the narrowest form
    for (int j = 0; j < n; ++j) {
        const int H = image_tab_host[4 * j], W = image_tab_host[4 * j + 1], r0 = image_tab_host[4 * j + 2], nr = image_tab_host[4 * j + 3];
        if (H <= 0 || W <= 0 || H > kMaskMaxExtent || W > kMaskMaxExtent) return MP_ERR_SHAPE;
        if (nr < 0 || r0 != next_region) return MP_ERR_SHAPE;  // the regions of the images follow one another
        const unsigned long long pixels = (unsigned long long)H * W;
        for (int r = r0; r < r0 + nr; ++r) {
            const int a = region_ptr_host[r], b = region_ptr_host[r + 1];
            if (a < 0 || b <= a || (r == 0 && a != 0)) return MP_ERR_SHAPE;
            for (int t = a + 1; t < b; ++t)
                if (prefix_host[t] < prefix_host[t - 1]) return MP_ERR_SHAPE;
            if (prefix_host[b - 1] != pixels) return MP_ERR_SHAPE;  // the counts do not sum to H * W
        }
        next_region = r0 + nr;
        const long long oo = offsets_host[2 * j], co = offsets_host[2 * j + 1];
        if (oo < 0 || co < 0 || (unsigned long long)oo + (unsigned long long)s * pixels > out_bytes ||
            (nr > 0 && (unsigned long long)co + pixels > workspace_bytes))  // an image without regions has no clearance plane
            return MP_ERR_SHAPE;
        hmax = H > hmax ? H : hmax;
        wmax = W > wmax ? W : wmax;
        all_wide = all_wide && W % 4 == 0 && ((uintptr_t)out + (uintptr_t)oo) % 4 == 0 && ((uintptr_t)workspace + (uintptr_t)co) % 4 == 0;
    }
    p.prefix = prefix_dev; p.region_ptr = region_ptr_dev; p.image_tab = image_tab_dev; p.offsets = offsets_dev;
    p.out = out; p.clear = workspace; p.s = s;
    if (next_region > 0) {
        hipLaunchKernelGGL(row_clearance_kernel, dim3((unsigned)hmax, (unsigned)n), dim3(256), 0, as_stream(stream), p);
        const int rc = check_launch();
        if (rc != MP_OK) return rc;
    }
    // a workgroup row is 64 pixels wide in the wide form, 16 in the scalar one; in a mixed batch a wide image leaves its surplus
    // workgroups at once
    const int group_w = all_wide ? 64 : 16;
    hipLaunchKernelGGL(erode_kernel, dim3((unsigned)((wmax + group_w - 1) / group_w), (unsigned)((hmax + 15) / 16), (unsigned)n), dim3(256), 0,
                       as_stream(stream), p);
    return check_launch();
}
