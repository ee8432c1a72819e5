// fp16-MFMA convolution family (amp level O2/O3 inference): declarations shared by conv_f16.hip and the launch plan.
//
// Activations live in HBM channel-blocked, [N][ceil(C/8)][H][W][8] halfs ("c8"): one pixel of one 8-channel block is a
// 16-byte element, which is exactly the per-lane operand of v_mfma_f32_16x16x32_f16 (8 consecutive k), so global ->
// LDS staging is plain 16-byte copies and every MFMA operand is ONE ds_read_b128 at any tap offset or stride.
// Padding channels of the last block are kept zero by every producer.
#pragma once
#include <type_traits>

#include "common.h"

namespace mp {

struct ConvF16Params {
    const void* x;       // c8 halfs
    const void* wp;      // packed weights [Cin_pad32/32][T][4][Cout_pad16][8] halfs
    const float* scale;  // [Cout_pad16] fp32 (zero beyond Cout)
    const float* shift;  // [Cout_pad16]
    const void* res1;    // c8 halfs, output geometry
    const void* res2;
    void* out;           // c8 halfs
    int N, C8in, H, W;
    int Cout, Cout_pad16, C8out;
    int Ho, Wo, pad_t, pad_l;
    int R, G, Rin, Wp, img_plane;
    int plane;       // LDS elements (16 B) per 8-channel plane: == 0 (mod 16) for stride 1, odd for stride 2
    int PK;          // planes per chunk (multiple of 4 = one MFMA k-step of 32 channels)
    int PKs;         // planes per chunk that are staged (PK, or C8in when the single chunk is zero padded)
    int n_chunks, n_ct, tiles_y, tiles_n;
    int ncols, upc;  // staged columns per row, staging units per plane (G * Rin * ncols)
    int in_buf;      // LDS elements per input buffer (PK * plane)
    int w_buf;       // LDS elements per weight buffer (PK * T * CT)
    int nbuf;
    int relu;
    int out_h, out_w, out_mul, off_y, off_x;  // output mapping: conv pixel (y, x) -> (y*out_mul + off_y, x*out_mul + off_x)
    unsigned magic_upc, magic_ncols, magic_rin, magic_rwo, magic_wo;
    int RWo, total_blocks;
    int phases;              // 4: MP_CONV_PHASES4 - blockIdx.y = phase 2 py + px (its output offset, its weight slice); else 1
    unsigned w_phase_bytes;  // bytes per weight slice
    // persistent multi-tile kernel only: a workgroup keeps its weight slice in LDS and walks tiles_per_wg pixel tiles
    int tiles_total, tiles_per_wg, n_groups;
    int ni_used, nw_used;  // staging slots (of the kernel's NI / NW) that carry data for this shape: the rest are skipped
    unsigned magic_rows;       // / (G * Rin)
    int step_rows, step_cols;  // 256 staging units = step_rows whole rows + step_cols columns (slot-to-slot stepping)
    // BatchNorm statistics from the epilogue (training; conv_f16_dev.h): 0 = off, 1 = forward sums of the output, 2 = backward sums
    // of the masked gradient (the stored tensor is then the masked gradient)
    int st_mode, st_nparts, st_relu;
    float* st_part;        // [C8out][st_nparts][8][2] fp32
    const void* st_z;      // mode 2: the BatchNorm's input (output geometry, c8 halfs)
    const void* st_y;      // mode 2, st_relu == 1: the BatchNorm's output (mask = y > 0)
    // BatchNorm apply on the INPUT operand (training, mode 1, weights-in-registers kernel): the tensor at x is the raw conv output z
    // of the layer below; the staged tile becomes act(z * pre_scale[c] + pre_shift[c]) in LDS (padding stays zero) and the tile's own
    // rows are also written to pre_out - the activation tensor the backward pass reads - so no separate apply pass runs
    const float* pre_scale;  // [PK * 8] (zeros behind Cin); null: off
    const float* pre_shift;
    void* pre_out;           // may be null
    int pre_relu;
};

struct ConvF16Launch {
    ConvF16Params p;
    int ks, stride, variant;
    size_t lds_bytes;
};

// ---- Tile geometry: the rules the four configure functions share (f16_configure / f16_configure_mt in conv_f16.hip,
// f16_configure_wreg, f16_configure_ws).  Each family keeps what is its own: the LDS budget search over rows and chunk size (one
// tile), the buffer count and tile runs (multi-tile), the shared zero column and the fast DMA form (weights in registers), the
// fewest-tiles-per-workgroup row choice (weight-stationary).
//
// Fields whose meaning depends on the family that fills them in (the kernels read the same block):
//
//   field        | one-tile / multi-tile              | weights in registers                | weight-stationary
//   -------------+------------------------------------+-------------------------------------+--------------------------------
//   Wp           | columns the taps reach (widened to | W + halo: one shared zero column    | W + 1
//                | the padded row when <= 2 wider)    |                                     |
//   plane        | G img_plane, rounded (see          | G img_plane + halo, rounded; fast   | img_plane + 1, rounded up to 64
//                | f16_geom_planes)                   | form: rounded up to 64              |
//   ncols        | staged columns per row             | W                                   | W
//   upc          | staging units per plane            | DMA pieces (64 elements) per plane, | DMA pieces per plane
//                | (G Rin ncols)                      | 0 = the slow staging form           |
//   magic_upc    | / upc                              | / plane                             | -
//   magic_ncols  | / ncols                            | / Wp                                | / Wp
//   magic_rin    | / Rin                              | / img_plane                         | 0
//   magic_rwo    | / RWo                              | / RWo                               | 0
//   magic_wo     | / Wo                               | / Wo                                | / W
//   magic_rows   | one-tile: / (G Rin); multi-tile: - | -                                   | / tiles_y
//   tiles_total  | multi-tile only                    | tiles_y tiles_n                     | tiles_y N
//   nbuf         | chunk buffers (1 or 2) / input     | 1                                   | 2 (the DMA ring)
//                | tile buffers (2, or 1)             |                                     |

// tensor extents, padding, activation and the output mapping, straight from the desc
inline void f16_geom_tensors(const mp_conv_desc& d, ConvF16Params& p) {
    p.N = d.n; p.H = d.h; p.W = d.w; p.Cout = d.cout;
    p.C8in = (d.cin + 7) / 8;
    p.Cout_pad16 = round_up(d.cout, 16);
    p.C8out = (d.cout + 7) / 8;
    p.Ho = d.conv_h; p.Wo = d.conv_w; p.pad_t = d.pad_top; p.pad_l = d.pad_left;
    p.relu = d.relu;
    p.out_h = d.out_h; p.out_w = d.out_w; p.out_mul = d.out_mul; p.off_y = d.out_off_y; p.off_x = d.out_off_x;
}
// 32-bit byte offsets over the whole tensors (the output's are sums of masked parts: kInv in conv_f16_dev.h).  The one-tile kernel
// rebases its input descriptor per tile and does not ask.
inline bool f16_geom_offsets_fit(const mp_conv_desc& d, const ConvF16Params& p) {
    return (long long)d.n * p.C8in * d.h * d.w * 16 < 0x7FFFFFF0LL && (long long)d.n * p.C8out * d.out_h * d.out_w * 16 < 0x60000000LL;
}
// a pixel tile of PT pixels holds R whole output rows of one image - or, when that is the whole image, G whole images
inline void f16_geom_fit(ConvF16Params& p, int R, int PT) {
    p.R = R;
    p.G = 1;
    if (R == p.Ho) {
        p.G = PT / (p.Ho * p.Wo);
        if (p.G > p.N) p.G = p.N;
        if (p.G < 1) p.G = 1;
    }
    p.RWo = p.R * p.Wo;
}
// The staged tile: Rin input rows of pitch Wp per image, G images per 8-channel plane and `tail` elements behind them (the zero slot
// of the DMA kernels).  Plane pitch in 16-byte elements: == 0 (mod 16) for stride 1, odd for stride 2 (the lanes of a wave then read
// every other element) - either way every ds_read_b128 is conflict-free.
inline void f16_geom_planes(ConvF16Params& p, int KS, int S, int Wp, int tail) {
    p.Rin = (p.R - 1) * S + KS;
    p.Wp = Wp;
    p.img_plane = p.Rin * p.Wp;
    p.plane = S == 1 ? round_up(p.G * p.img_plane + tail, 16) : ((p.G * p.img_plane + tail) | 1);
}
// the DMA kernels' staging by pieces: one image per tile, the plane pitch a whole number of 64-element pieces
inline void f16_geom_dma_pieces(ConvF16Params& p, int tail) {
    p.plane = round_up(p.img_plane + tail, 64);
    p.upc = p.plane / 64;
}
// cout slices of CT, row bands per image (one when a tile holds whole images), image groups
inline void f16_geom_tiles(ConvF16Params& p, int CT) {
    p.n_ct = (p.Cout_pad16 + CT - 1) / CT;
    p.tiles_y = (p.G > 1 || p.R >= p.Ho) ? 1 : (p.Ho + p.R - 1) / p.R;
    p.tiles_n = (p.N + p.G - 1) / p.G;
}
// Persistent kernels: workgroups per cout slice - all resident at once, or what the test knob says (long tile runs on small
// problems) - and the tile runs they walk.  False: a run of ONE tile amortises nothing, the one-tile kernels do that with less LDS.
inline int f16_geom_groups(int occ, int n_ct, const char* knob_name) {
    int groups = occ * 256 / n_ct;
    if (const char* e = knob(knob_name)) {
        const int v = atoi(e);
        if (v >= 1) groups = v;
    }
    return groups;
}
inline bool f16_geom_runs(ConvF16Params& p, int groups) {
    p.tiles_total = p.tiles_y * p.tiles_n;
    p.tiles_per_wg = (p.tiles_total + groups - 1) / groups;
    if (p.tiles_per_wg < 2) return false;
    p.n_groups = (p.tiles_total + p.tiles_per_wg - 1) / p.tiles_per_wg;
    p.total_blocks = p.n_ct * p.n_groups;
    return true;
}
// lane -> (image, row, column) of its output pixel
inline void f16_geom_pixel_magics(ConvF16Params& p) {
    p.magic_rwo = magic_of(p.RWo);
    p.magic_wo = magic_of(p.Wo);
}

// Tile variants.  The ids are ABI: the tuner's tables and persisted caches, tests/f16_matrix.py and
// tests/golden/bench_plan_picks.json hold them.  What each id IS stands in kF16Variants below, and nowhere else.
enum ConvF16Variant { F_CT32_PT192 = 0, F_CT64_PT192 = 1, F_CT48_PT192 = 2, F_CT64_PT96 = 3, F_CT32_PT96 = 4,
                      F_CT32_PT192_L = 5, F_CT64_PT192_L = 6, F_CT48_PT192_L = 7, F_CT64_PT96_L = 8, F_CT32_PT96_L = 9,
                      F_MT2_BASE = 10, F_MT1_BASE = 15,
                      F_CT16_PT192 = 20, F_CT16_PT192_L = 21, F_CT16_PT192_MT2 = 22, F_CT16_PT192_MT1 = 23, F_CT32_PT384 = 24,
                      // P<pixel tiles of 16>C<cout tiles of 16 per wave>_W<n>: n waves split the pixel tiles (4 / n split the couts)
                      F_WREG_P6C2 = 25, F_WREG_P3C2 = 26, F_WREG_P6C1 = 27, F_WREG_P6C3 = 28, F_WREG_P3C3 = 29, F_WREG_P3C4 = 30,
                      F_WREG_P6C2_W2 = 31, F_WREG_P6C3_W2 = 32, F_WREG_P3C2_W2 = 33, F_WREG_P6C2_W4 = 34, F_WREG_P6C3_W4 = 35,
                      F_WREG_P3C2_W4 = 36,
                      F_WS_BASE = 37, F_WS_COUNT = 8,
                      F_WREG_P7C3 = 45, F_WREG_P4C3 = 46, F_WREG_P5C4 = 47, F_COUNT = 48 };

// kernel families: one tile per workgroup (conv_f16.hip), persistent multi-tile with the weights resident in LDS and the input tiles
// double-buffered (conv_f16_mt.hip), weights in registers (conv_f16_wreg.hip), weight-stationary persistent (conv_f16_ws.hip)
enum F16Family { kF16Tile, kF16Mt, kF16Wreg, kF16Ws };

// One row per variant id.  A wave owns ps pixel tiles x cs cout tiles of 16; waves_p of the 4 waves split the pixels, 4 / waves_p the
// couts: the workgroup's tile is 16 cs (4 / waves_p) couts x 16 ps waves_p pixels.  occ = workgroups per CU the build is compiled for.
struct F16Variant {
    F16Family family;
    int ps, cs, waves_p, occ;
    bool light;      // one-tile kernel: small chunks / few staging registers, three workgroups per CU (<= 52 KiB LDS)
    bool one_chunk;  // one-tile kernel: the build without a chunk loop - launches with n_chunks == 1 only
    bool k3s1_only;  // weights in registers: built for the 3x3 stride-1 branch convs only
    int nq;          // weight-stationary: k-steps of 32 input channels, Cin in (32 (nq - 1), 32 nq]
};
constexpr F16Variant f16_tile_row(int ps, int cs, int waves_p, bool light = false, bool one_chunk = false) {
    return {kF16Tile, ps, cs, waves_p, light ? 3 : 2, light, one_chunk, false, 0};
}
constexpr F16Variant f16_mt_row(int cs, int waves_p, int occ) { return {kF16Mt, 3, cs, waves_p, occ, false, false, false, 0}; }
constexpr F16Variant f16_wreg_row(int ps, int cs, int waves_p, int occ, bool k3s1_only = false) {
    return {kF16Wreg, ps, cs, waves_p, occ, false, false, k3s1_only, 0};
}
constexpr F16Variant f16_ws_row(int nq, int cs, int waves_p, int ps, int occ) { return {kF16Ws, ps, cs, waves_p, occ, false, false, false, nq}; }
constexpr F16Variant kF16Variants[F_COUNT] = {
    // 0..4: the five cout x pixel tiles of the one-tile kernel, 5..9 their light builds
    f16_tile_row(3, 2, 4), f16_tile_row(3, 4, 4), f16_tile_row(3, 3, 4), f16_tile_row(3, 2, 2), f16_tile_row(3, 1, 2),
    f16_tile_row(3, 2, 4, true), f16_tile_row(3, 4, 4, true), f16_tile_row(3, 3, 4, true), f16_tile_row(3, 2, 2, true), f16_tile_row(3, 1, 2, true),
    // 10..14 / 15..19: the same tiles in the multi-tile kernel, compiled for two / one workgroup per CU
    f16_mt_row(2, 4, 2), f16_mt_row(4, 4, 2), f16_mt_row(3, 4, 2), f16_mt_row(2, 2, 2), f16_mt_row(1, 2, 2),
    f16_mt_row(2, 4, 1), f16_mt_row(4, 4, 1), f16_mt_row(3, 4, 1), f16_mt_row(2, 2, 1), f16_mt_row(1, 2, 1),
    // 20..23: 16 couts x 192 px (twice the workgroups: latency hiding for the large-K small-map layers): one-tile, light, multi-tile
    f16_tile_row(3, 1, 4), f16_tile_row(3, 1, 4, true), f16_mt_row(1, 4, 2), f16_mt_row(1, 4, 1),
    // 24: 32 couts x 384 px for the small-K layers: a workgroup's fixed set-up (a third of its life at K = 288) and its
    // weight loads are spread over twice the MFMA work
    f16_tile_row(6, 2, 4, false, true),
    // 25..36: weights in registers
    f16_wreg_row(6, 2, 1, 1), f16_wreg_row(3, 2, 1, 2), f16_wreg_row(6, 1, 1, 2), f16_wreg_row(6, 3, 1, 1), f16_wreg_row(3, 3, 1, 1),
    f16_wreg_row(3, 4, 1, 1), f16_wreg_row(6, 2, 2, 2), f16_wreg_row(6, 3, 2, 1), f16_wreg_row(3, 2, 2, 2), f16_wreg_row(6, 2, 4, 2),
    f16_wreg_row(6, 3, 4, 1), f16_wreg_row(3, 2, 4, 2),
    // 37..44: weight-stationary (the table that was conv_f16_ws.hip's kWsShapes)
    f16_ws_row(1, 2, 4, 3, 2),  // 32 channels: 32 couts x 192 px (training convs of the 32-channel branch; inference runs them as fused blocks)
    f16_ws_row(2, 3, 4, 5, 1),  // 48 (W48 branch 1): 48 couts x 320 px
    f16_ws_row(2, 4, 4, 3, 1),  // 64: 64 couts x 192 px
    f16_ws_row(2, 2, 4, 3, 1),  // 64: two cout slices of 32 x 192 px
    f16_ws_row(3, 2, 4, 5, 1),  // 96 (W48 branch 2): three cout slices of 32 x 320 px
    f16_ws_row(3, 3, 4, 3, 1),  // 96: two cout slices of 48 x 192 px
    f16_ws_row(4, 2, 2, 3, 1),  // 128: two cout slices of 64 x 96 px
    f16_ws_row(4, 2, 1, 6, 1),  // 128: 128 couts x 96 px
    // 45..47: weights-in-registers shapes whose pixel tile makes W48's deep layers ONE round of 256 workgroups: 112 px x 192 couts
    // (192 -> 192 @24x18, N = 64: 6 rows of 18 = 4 tiles per image x 64), 64 px x 192 couts (384 -> 384 @12x9: 7 rows of 9 = 2 tiles
    // per image x 64 x 2 cout slices), 80 px x 256 couts
    f16_wreg_row(7, 3, 1, 1, true), f16_wreg_row(4, 3, 1, 1, true), f16_wreg_row(5, 4, 1, 1, true),
};
constexpr const F16Variant& f16_variant(int v) { return kF16Variants[v]; }  // 0 <= v < F_COUNT (f16_build_launch refuses the rest)
inline bool f16_variant_wreg(int v) { return f16_variant(v).family == kF16Wreg; }
inline bool f16_variant_ws(int v) { return f16_variant(v).family == kF16Ws; }
inline bool f16_variant_mt(int v) { return f16_variant(v).family == kF16Mt; }
constexpr int f16_variant_ct(int v) { return 16 * f16_variant(v).cs * (4 / f16_variant(v).waves_p); }
constexpr int f16_variant_pt(int v) { return 16 * f16_variant(v).ps * f16_variant(v).waves_p; }

// Runs f(std::integral_constant<int, V>) for the id V == v of one family - the family's dispatch instantiates its kernels from the
// table's rows, over its own ids only; MP_ERR_UNSUPPORTED for an id of another family
template <F16Family FAM, int V = 0, class F>
int f16_dispatch_variant(int v, F&& f) {
    if constexpr (V == F_COUNT) {
        return MP_ERR_UNSUPPORTED;
    } else {
        if constexpr (kF16Variants[V].family == FAM) {
            if (v == V) return f(std::integral_constant<int, V>{});
        }
        return f16_dispatch_variant<FAM, V + 1>(v, f);
    }
}

// The training builds (epilogue statistics, conv_f16_dev.h) of the one-tile and multi-tile kernels exist for the kernel sizes a
// BatchNorm follows / a data gradient runs through - 1x1 and 3x3: forward sums at either stride, backward sums at stride 1 (data
// gradients are stride-1 launches) - and for the 2x2 phase convs of a stride-2 data gradient: backward sums only.
constexpr bool f16_has_stats_build(int ks, int s, int mode) {
    if (mode == 0) return true;
    if (ks == 1 || ks == 3) return mode == 1 || s == 1;
    return ks == 2 && s == 1 && mode == 2;
}
// launch(std::integral_constant<int, STATS>) for the build that serves p.st_mode
template <int KS, int S, class F>
int f16_dispatch_stats(int st_mode, F&& launch) {
    if (st_mode == 0) return launch(std::integral_constant<int, 0>{});
    if constexpr (f16_has_stats_build(KS, S, 1)) {
        if (st_mode == 1) return launch(std::integral_constant<int, 1>{});
    }
    if constexpr (f16_has_stats_build(KS, S, 2)) {
        if (st_mode == 2) return launch(std::integral_constant<int, 2>{});
    }
    return MP_ERR_UNSUPPORTED;
}

// fused BasicBlock of the 32-channel branch (basicblock_f16.hip)
struct BlockF16Params {
    const void* x;
    const void* w1;
    const void* w2;
    const float* scale1;
    const float* shift1;
    const float* scale2;
    const float* shift2;
    void* out;
    int N, H, W;
    int R, Wp, plane_in, plane_mid;  // LDS planes in 16-byte units (multiples of 16: conflict-free ds_read_b128)
    int M1, M2;                      // intermediate / output pixels of a tile
    int in_units;                    // staged 16-byte units of the input tile (4 planes x (R+4) rows x W)
    int tiles_y, tiles_total, tiles_per_wg, total_blocks, ni_used;
    unsigned magic_w, magic_rw;      // / W, / ((R+4) * W)   (second structure: / (W + 1), / plane_in)
    unsigned magic_wo;               // second structure: / W
    unsigned long long* dbg;         // diagnostic builds (-DMP_BLOCK_STAMPS=1) only: 16 x u64 per (workgroup, wave half)
};

// which kernel serves a fused block (mp_plan_entry_info reports the number)
enum BlockForm { kTile65 = 0, kTile53 = 1,      // first structure of the 32-channel block: the <6,5> / <5,3> pixel-tile builds
                 kV2Wave8 = 2, kV2Wave4 = 3,    // second structure, eight / four waves (the four-wave shape is not built any more)
                 kC64 = 4, kC128 = 5 };         // 64- / 128-channel block
struct BlockF16Launch {
    BlockF16Params p;
    BlockForm form;
    size_t lds_bytes;
};
int blockf16_build(const void* x, const void* w1, const float* scale1, const float* shift1, const void* w2, const float* scale2,
                   const float* shift2, void* out, int n, int c, int h, int w, int rows, BlockF16Launch& L);
int blockf16_launch(const BlockF16Launch& L, hipStream_t s);
inline int run(const BlockF16Launch& L, hipStream_t s) { return blockf16_launch(L, s); }
inline void describe(const BlockF16Launch& L, int64_t info[12]) {
    const int c = L.form == kC64 ? 64 : L.form == kC128 ? 128 : 32;  // cout tile / cin chunk = the block's width
    fill_info(info, {kBlockF16, 3, 1, L.form, L.p.total_blocks, (int64_t)L.lds_bytes, c, L.p.M2, c, 1, L.p.R});
}
// second structure (basicblock_f16_v2.hip): weights in registers, LDS-DMA bands, 512-thread workgroups (form kV2Wave8)
bool blockf16_v2_build(const void* x, const void* w1, const float* scale1, const float* shift1, const void* w2, const float* scale2,
                       const float* shift2, void* out, int n, int c, int h, int w, int rows, BlockF16Launch& L);
int blockf16_v2_launch(const BlockF16Launch& L, hipStream_t s);
// 64- / 128-channel block (basicblock_f16_c64.hip): one band per workgroup, cout tile per wave (forms kC64 / kC128)
bool blockf16_c64_build(const void* x, const void* w1, const float* scale1, const float* shift1, const void* w2, const float* scale2,
                        const float* shift2, void* out, int n, int c, int h, int w, int rows, BlockF16Launch& L);
int blockf16_c64_launch(const BlockF16Launch& L, hipStream_t s);

// two chained 1x1 convs of HRNet's stage 1 in one launch (pwchain_f16.hip): expand conv of Bottleneck i + reduce conv of i + 1
struct PwChainParams {
    const void* mid;   // [N][CM/8][HW] x 16 B: the 3x3 conv's output
    const void* res;   // [N][CE/8][HW]: the identity of the expand conv
    const void* w3;    // packed 1x1 weights CM -> CE
    const float* scale3;
    const float* shift3;
    const void* w1;    // packed 1x1 weights CE -> CR
    const float* scale1;
    const float* shift1;
    void* y;           // [N][CE/8][HW]
    void* z;           // [N][CR/8][HW]
    int N, HW, tiles_per_img, total_blocks, relu3, relu1;
    // down-sample form: the identity is conv1x1(x0; wd) * scale_d + shift_d (no ReLU), computed in the launch (res unused)
    const void* x0;    // [N][CM/8][HW]: the block's input
    const void* wd;    // packed 1x1 weights CM -> CE
    const float* scale_d;
    const float* shift_d;
};
struct PwChainLaunch {
    PwChainParams p;
    int cm, ce, cr, h, w;
    bool dual;  // both convs read `mid` (the first Bottleneck's down-sample + reduce convs): res == mid marks it
    bool ds;    // the identity is the block's down-sample conv of x0, computed in the launch
    size_t lds_bytes;
};
int pwchain_build(const void* mid, const void* res, const void* w3, const float* scale3, const float* shift3, int relu3, const void* w1,
                  const float* scale1, const float* shift1, int relu1, void* y, void* z, int n, int cm, int ce, int cr, int h, int w,
                  PwChainLaunch& L, const void* x0 = nullptr, const void* wd = nullptr, const float* scale_d = nullptr,
                  const float* shift_d = nullptr);
int pwchain_launch(const PwChainLaunch& L, hipStream_t s);
inline int run(const PwChainLaunch& L, hipStream_t s) { return pwchain_launch(L, s); }
inline void describe(const PwChainLaunch& L, int64_t info[12]) {
    fill_info(info, {kPwChainF16, 1, 1, L.dual ? 1 : L.ds ? 2 : 0, L.p.total_blocks, (int64_t)L.lds_bytes, L.ce, 64, L.cm, 1});
}

// first conv of the network straight from the fp32 NCHW image (stem_f16.hip): 3x3 stride 2 padding 1, 3 -> 64 channels
struct StemF16Params {
    const float* x;      // [N][3][H][W] fp32
    const float* w;      // [64][3][3][3] fp32
    const float* scale;  // [64]
    const float* shift;
    void* out;           // [N][8][H/2][W/2] x 16 B
    int N, H, W, Ho, Wo, pitch, tiles_y, total_blocks, relu;
    unsigned magic_upr;  // / (W / 4)
};
struct StemF16Launch {
    StemF16Params p;
    size_t lds_bytes;
};
int stemf16_build(const float* x, const float* w, const float* scale, const float* shift, int relu, void* out, int n, int h, int wd,
                  StemF16Launch& L);
int stemf16_launch(const StemF16Launch& L, hipStream_t s);
inline int run(const StemF16Launch& L, hipStream_t s) { return stemf16_launch(L, s); }
inline void describe(const StemF16Launch& L, int64_t info[12]) {  // 64 couts x 8 output rows per workgroup, one 3-channel chunk
    fill_info(info, {kStemF16, 3, 2, 0, L.p.total_blocks, (int64_t)L.lds_bytes, 64, 8 * L.p.Wo, 3, 1, 8});
}

int f16_build_launch(const mp_conv_desc* desc, int variant, const void* x, const void* w, const float* scale,
                     const float* shift, const void* res1, const void* res2, void* out, ConvF16Launch& L);
int f16_launch(const ConvF16Launch& L, hipStream_t s);
// partial-sum slots (per channel) a launch with epilogue statistics writes: one per pixel-tile workgroup / persistent workgroup
int f16_stats_parts(const ConvF16Launch& L);
int f16_mt_launch(const ConvF16Launch& L, hipStream_t s);
bool f16_configure_wreg(const mp_conv_desc& d, int variant, ConvF16Launch& L);
int f16_wreg_launch(const ConvF16Launch& L, hipStream_t s);
int f16_mt_ni(int occ);
bool f16_configure_ws(const mp_conv_desc& d, int variant, ConvF16Launch& L);
int f16_ws_launch(const ConvF16Launch& L, hipStream_t s);

inline int run(const ConvF16Launch& L, hipStream_t s) { return f16_launch(L, s); }
inline void describe(const ConvF16Launch& L, int64_t info[12]) {
    fill_info(info, {kConvF16, L.ks, L.stride, L.variant, L.p.total_blocks, (int64_t)L.lds_bytes, f16_variant_ct(L.variant),
                     f16_variant_pt(L.variant), L.p.PK * 8, L.p.G, L.p.R, f16_variant(L.variant).light ? 1 : 0});
}

}  // namespace mp
