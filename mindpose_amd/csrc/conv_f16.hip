// fp16-MFMA direct convolution (v_mfma_f32_16x16x32_f16, fp32 accumulate) over channel-blocked activations, plus the
// layout converters and the exchange-unit sum in that layout.  See conv_f16.h for the data layout.
//
//   implicit GEMM:  rows (MFMA A) = output channels, columns (MFMA B) = output pixels, K = Cin x KS x KS; one k-step =
//                   32 input channels = 4 channel-block planes, lane l feeding plane (l >> 4), pixel / cout (l & 15).
//   D layout:       lane holds couts 4*(l>>4) .. +3 of one pixel (l & 15): four halfs = one 8-byte store into the pixel's
//                   16-byte channel block; a wave's store instruction covers whole 256-byte runs.
//   LDS:            input tile [PK planes][G images][Rin rows][Wp cols] x 16 B with zero halo; plane stride == 0 mod 16
//                   elements (stride 1) or odd (stride 2) keeps every ds_read_b128 conflict-free; weight tile
//                   [PK/4][T][4][CT] x 16 B is a lane-linear image of the A operands.
//   pipeline:       as the fp32 kernel: chunk c+1 is fetched into registers (range-checked buffer loads) while chunk c
//                   computes, operand fragments are read one k-step ahead, one barrier per chunk.
//   epilogue:       fp32 scale/shift (folded BatchNorm or bias), up to two residual tensors, ReLU, one rounding to fp16.
#include <stdlib.h>

#include "conv_f16.h"
#include "conv_f16_dev.h"

namespace mp {

namespace {

// ONE_CHUNK: the build for layers whose whole K fits one chunk (the 32-channel layers): no chunk loop, so the staging
// registers are dead before the MFMA loop and a wave can own six pixel tiles instead of three
// STATS: the training build whose epilogue also produces the partial BatchNorm sums of conv_f16_dev.h (p.st_mode 1 / 2)
// The kernel body as a device function of (parameters, workgroup index, phase index); conv_f16_kernel below passes its own launch
// parameters and blockIdx.  (Round 5 put a grouped launch on top of it - several independent convs of one instantiation from a job
// table, bit-identical to the single launches - for the branches of an HRModule at small batch sizes; the one-crop amp-O2 forward
// got SLOWER with it, 1.06 -> 1.63 ms: DESIGN 7.  The kernel is gone again, the split stays.)
template <int KS, int S, int PS, int CS, int WAVES_P, int WAVES_C, int NI, int NW, int OCC, bool ONE_CHUNK = false, int STATS = 0>
__device__ __forceinline__ void conv_f16_body(const ConvF16Params& p, const int block_x, const int block_y) {
    static_assert(WAVES_P * WAVES_C == 4, "4 waves per workgroup");
    constexpr int T = KS * KS;
    constexpr int CT = 16 * CS * WAVES_C;
    extern __shared__ __attribute__((aligned(16))) u32x4 smem16[];
    u32x4* __restrict__ lds_in = smem16;                     // [nbuf][in_buf]
    u32x4* __restrict__ lds_w = smem16 + p.nbuf * p.in_buf;  // [nbuf][w_buf]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp_i = wave % WAVES_P, wc_i = wave / WAVES_P;
    const int lq = lane >> 4, lr = lane & 15;

    // XCD-aware tile id (blocks b, b+8, ... share an XCD): every XCD walks a contiguous run of tiles
    int b = xcd_contiguous(block_x, p.total_blocks);
    const int ct = b % p.n_ct;
    b /= p.n_ct;
    // pixel tile (of its phase, MP_CONV_PHASES4) = partial-sum slot of the epilogue statistics
    const int part_idx = (p.phases > 1 ? block_y * (p.tiles_y * p.tiles_n) : 0) + b;
    const int ty = b % p.tiles_y, tn = b / p.tiles_y;
    const int n0 = tn * p.G, y0 = ty * p.R;
    const int y_in0 = y0 * S - p.pad_t;
    const int HW = p.H * p.W;

    {
        const int n16 = (p.n_chunks > 1 ? p.nbuf : 1) * p.in_buf;  // a single-chunk launch only ever touches buffer 0
        const u32x4 zero = (u32x4){0u, 0u, 0u, 0u};
        for (int i = tid; i < n16; i += 256) lds_in[i] = zero;
    }

    // Staging tables.  A workgroup of the small-K layers lives ~12 k cycles, of which this integer set-up used to be a
    // quarter (in-kernel cycle stamps): only the slots the shape uses are filled, and slot i+1 is derived from slot i by
    // stepping 256 units forward (row / plane carries) instead of three magic-number divisions per slot.
    unsigned isrc[NI];
    int idst[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        isrc[i] = kOob;
        idst[i] = -1;
    }
    {
        const int rows = p.G * p.Rin;  // staged rows per channel-block plane
        unsigned pl = fastdiv((unsigned)tid, p.upc, p.magic_upc);
        const unsigned rem0 = tid - pl * p.upc;
        unsigned gr = fastdiv(rem0, p.ncols, p.magic_ncols);
        unsigned xu = rem0 - gr * p.ncols;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (i < p.ni_used && pl < (unsigned)p.PKs) {
                const unsigned g = p.G > 1 ? fastdiv(gr, p.Rin, p.magic_rin) : 0u;
                const unsigned r = gr - g * p.Rin;
                const int yin = y_in0 + (int)r;
                if (yin >= 0 && yin < p.H && n0 + (int)g < p.N) {
                    isrc[i] = ((g * p.C8in + pl) * HW + yin * p.W + xu) * 16u;
                    idst[i] = (int)((pl << 20) | (pl * p.plane + g * p.img_plane + r * p.Wp + p.pad_l + xu));
                }
            }
            xu += p.step_cols;  // 256 units further: 256 = step_rows * ncols + step_cols
            gr += p.step_rows;
            if (xu >= (unsigned)p.ncols) { xu -= p.ncols; ++gr; }
            if (gr >= (unsigned)rows) {  // plane carry (several planes at once on the small maps)
                const unsigned k = fastdiv(gr, rows, p.magic_rows);
                gr -= k * rows;
                pl += k;
            }
        }
    }

    int b_off[PS];  // pixel operand
    int pix_gyx[PS];  // the lane's pixel of tile ps as (image << 24 | row << 12 | col), -1 = padding lane: reused by the epilogue
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        const unsigned pl0 = (unsigned)((wp_i * PS + ps) * 16 + lr);
        const unsigned pl = pl0 < (unsigned)(p.G * p.RWo) ? pl0 : 0u;
        const unsigned g = fastdiv(pl, p.RWo, p.magic_rwo);
        const unsigned rem = pl - g * p.RWo;
        const unsigned y = fastdiv(rem, p.Wo, p.magic_wo);
        const unsigned xx = rem - y * p.Wo;
        b_off[ps] = lq * p.plane + g * p.img_plane + (y * S) * p.Wp + xx * S;
        pix_gyx[ps] = pl0 < (unsigned)(p.G * p.RWo) ? (int)((g << 24) | (y << 12) | xx) : -1;
    }
    int a_off[CS];  // weight operand
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) a_off[cs] = lq * CT + wc_i * CS * 16 + f16_a_row<CS>(cs, lr);

    f32x4 acc[PS][CS];
#pragma unroll
    for (int ps = 0; ps < PS; ++ps)
#pragma unroll
        for (int cs = 0; cs < CS; ++cs) acc[ps][cs] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int n_img = min(p.G, p.N - n0);
    const char* xg = reinterpret_cast<const char*>(p.x) + (size_t)n0 * p.C8in * HW * 16;
    const __amdgpu_buffer_rsrc_t rs_x = make_rsrc(xg, (size_t)n_img * p.C8in * HW * 16);
    const int w_units = p.PK * T * CT;  // 16-B elements of one weight chunk of this cout tile
    const __amdgpu_buffer_rsrc_t rs_w =
        make_rsrc(reinterpret_cast<const char*>(p.wp) + (p.phases > 1 ? (size_t)block_y * p.w_phase_bytes : (size_t)0),
                  (size_t)p.n_chunks * p.PK * T * p.Cout_pad16 * 16);
    unsigned wsrc[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        wsrc[i] = kOob;
        if (i >= p.nw_used) continue;
        const int u = tid + 256 * i;
        const int row = u / CT, c = u - row * CT;
        if (u < w_units && ct * CT + c < p.Cout_pad16) wsrc[i] = (unsigned)(row * p.Cout_pad16 + ct * CT + c) * 16u;
    }

    u32x4 vin[NI], vw[NW];
    auto stage_load = [&](int ch) {
        const int c0 = ch * p.PK;
        const unsigned xo = (unsigned)c0 * HW * 16u;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (i >= p.ni_used) break;  // uniform: slots beyond this shape's unit count issue nothing
            unsigned off = isrc[i] + xo;
            if (idst[i] >= 0 && c0 + (idst[i] >> 20) >= p.C8in) off = kOob;  // zero planes beyond the real channels
            vin[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0);
        }
        const unsigned wo = (unsigned)ch * p.PK * T * p.Cout_pad16 * 16u;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if (i >= p.nw_used) break;
            vw[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, wsrc[i] == kOob ? kOob : wsrc[i] + wo, 0, 0);
        }
    };
    auto stage_store = [&](int buf) {
        u32x4* __restrict__ din = lds_in + buf * p.in_buf;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (i >= p.ni_used) break;
            if (idst[i] >= 0) din[idst[i] & 0xFFFFF] = vin[i];
        }
        u32x4* __restrict__ dw = lds_w + buf * p.w_buf;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            if (i >= p.nw_used) break;
            const int u = tid + 256 * i;
            if (u < w_units) dw[u] = vw[i];
        }
    };

    stage_load(0);
    __syncthreads();  // zero fill complete before the first copy lands
    stage_store(0);
    __syncthreads();

    const int nq = p.PK >> 2;
    auto compute = [&](int buf) {
        const u32x4* __restrict__ lin = lds_in + buf * p.in_buf;
        const u32x4* __restrict__ lw = lds_w + buf * p.w_buf;
        u32x4 bv[PS], av[CS];
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) bv[ps] = lin[b_off[ps]];
#pragma unroll
        for (int cs = 0; cs < CS; ++cs) av[cs] = lw[a_off[cs]];
        for (int q = 0; q < nq; ++q) {
            const int in_q = q * 4 * p.plane;
            const int w_q = q * T * 4 * CT;
            const int qn = min(q + 1, nq - 1);  // the final prefetch re-reads a valid k-step (discarded)
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int tn = (t + 1 < T) ? t + 1 : 0;
                const int in_off = ((t + 1 < T) ? in_q : qn * 4 * p.plane) + (tn / KS) * p.Wp + (tn % KS);
                const int w_off = ((t + 1 < T) ? w_q : qn * T * 4 * CT) + tn * 4 * CT;
                u32x4 bn[PS], an[CS];
#pragma unroll
                for (int cs = 0; cs < CS; ++cs) an[cs] = lw[a_off[cs] + w_off];  // weights first: the next step's first MFMA needs them
#pragma unroll
                for (int ps = 0; ps < PS; ++ps) bn[ps] = lin[b_off[ps] + in_off];
#pragma unroll
                for (int ps = 0; ps < PS; ++ps)
#pragma unroll
                    for (int cs = 0; cs < CS; ++cs)
                        acc[ps][cs] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, av[cs]),
                                                                              __builtin_bit_cast(f16x8, bv[ps]), acc[ps][cs], 0, 0, 0);
                {
                    constexpr int NR = PS + CS, NM = PS * CS, NPAIR = NR < NM ? NR : NM;
#pragma unroll
                    for (int i = 0; i < NPAIR; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // 1 DS read
                    }
                    if (NM > NPAIR) __builtin_amdgcn_sched_group_barrier(0x008, NM - NPAIR, 0);
                    if (NR > NPAIR) __builtin_amdgcn_sched_group_barrier(0x100, NR - NPAIR, 0);
                }
#pragma unroll
                for (int ps = 0; ps < PS; ++ps) bv[ps] = bn[ps];
#pragma unroll
                for (int cs = 0; cs < CS; ++cs) av[cs] = an[cs];
            }
        }
    };
    // all chunks but the last: fetch chunk c+1 into registers while chunk c computes
    if constexpr (!ONE_CHUNK) {
        for (int ch = 0; ch + 1 < p.n_chunks; ++ch) {
            const int buf = ch & 1;
            stage_load(ch + 1);
            compute(buf);
            stage_store(buf ^ 1);
            __syncthreads();
        }
    }
    // ---- output addressing, lane = (pixel lr of tile ps) x (couts 4*lq .. +3 of tile cs) -> one 8-byte store; the
    //      residual tensors are fetched before the LAST chunk computes (the staging registers are free by then), so
    //      their latency hides under that chunk's MFMA phase
    const int plane_o = p.out_h * p.out_w;
    const size_t grp = (size_t)n0 * p.C8out * plane_o * 16;
    const size_t grp_bytes = (size_t)n_img * p.C8out * plane_o * 16;
    const __amdgpu_buffer_rsrc_t rs_o = make_rsrc(reinterpret_cast<char*>(p.out) + grp, grp_bytes);
    const int off_y = p.phases > 1 ? (int)(block_y >> 1) : p.off_y, off_x = p.phases > 1 ? (int)(block_y & 1) : p.off_x;
    unsigned pix_off[PS];
#pragma unroll
    for (int ps = 0; ps < PS; ++ps) {
        const unsigned g = (unsigned)pix_gyx[ps] >> 24, y = ((unsigned)pix_gyx[ps] >> 12) & 0xFFFu, xx = (unsigned)pix_gyx[ps] & 0xFFFu;
        const int yy = y0 + y;
        const bool ok = pix_gyx[ps] >= 0 && n0 + (int)g < p.N && yy < p.Ho;
        pix_off[ps] = ok ? (g * p.C8out * plane_o + (yy * p.out_mul + off_y) * p.out_w + xx * p.out_mul + off_x) * 16u : kInv;
    }
    f32x4 sc[CS], sh[CS];
    unsigned co_off[CS];
#pragma unroll
    for (int cs = 0; cs < CS; ++cs) {
        const int co = ct * CT + wc_i * CS * 16 + f16_d_cout<CS>(cs, lq);
        const bool ok = co < p.C8out * 8;
        const int cc = co < p.Cout_pad16 ? co : 0;
        sc[cs] = *reinterpret_cast<const f32x4*>(p.scale + cc);
        sh[cs] = *reinterpret_cast<const f32x4*>(p.shift + cc);
        co_off[cs] = ok ? (unsigned)(co >> 3) * plane_o * 16u + ((co >> 2) & 1) * 8u : kInv;
    }
    // cout tiles 2j, 2j+1 share a 16-byte channel block per pixel (conv_f16_dev.h): 16-byte residual loads and stores
    constexpr int NP = CS / 2, NS = CS - 2 * NP;
    u32x4 r1p[NP ? NP : 1][PS], r2p[NP ? NP : 1][PS];
    u32x2 r1s[PS], r2s[PS];
    if (p.res1) {
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(reinterpret_cast<const char*>(p.res1) + grp, grp_bytes);
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) r1p[j][ps] = __builtin_amdgcn_raw_buffer_load_b128(rs, co_off[2 * j] + pix_off[ps], 0, 0);
        if (NS) {
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) r1s[ps] = __builtin_amdgcn_raw_buffer_load_b64(rs, co_off[CS - 1] + pix_off[ps], 0, 0);
        }
    }
    if (p.res2) {
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(reinterpret_cast<const char*>(p.res2) + grp, grp_bytes);
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) r2p[j][ps] = __builtin_amdgcn_raw_buffer_load_b128(rs, co_off[2 * j] + pix_off[ps], 0, 0);
        if (NS) {
#pragma unroll
            for (int ps = 0; ps < PS; ++ps) r2s[ps] = __builtin_amdgcn_raw_buffer_load_b64(rs, co_off[CS - 1] + pix_off[ps], 0, 0);
        }
    }
    // epilogue statistics, backward mode: the BatchNorm's z (and y) at the output positions, fetched like the residuals
    f32x4 st_a[STATS ? CS : 1], st_b[STATS ? CS : 1];
    u32x4 zp[(STATS && NP) ? NP : 1][PS], yp[(STATS && NP) ? NP : 1][PS];
    u32x2 zs[PS], ys[PS];
    if constexpr (STATS) {
#pragma unroll
        for (int cs = 0; cs < CS; ++cs) {
            st_a[cs] = st_b[cs] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if constexpr (STATS == 2) {
            const __amdgpu_buffer_rsrc_t rz = make_rsrc(reinterpret_cast<const char*>(p.st_z) + grp, grp_bytes);
            const __amdgpu_buffer_rsrc_t ry = make_rsrc(reinterpret_cast<const char*>(p.st_y ? p.st_y : p.st_z) + grp, p.st_y ? grp_bytes : 0);
#pragma unroll
            for (int j = 0; j < NP; ++j)
#pragma unroll
                for (int ps = 0; ps < PS; ++ps) {
                    zp[j][ps] = __builtin_amdgcn_raw_buffer_load_b128(rz, co_off[2 * j] + pix_off[ps], 0, 0);
                    yp[j][ps] = __builtin_amdgcn_raw_buffer_load_b128(ry, co_off[2 * j] + pix_off[ps], 0, 0);
                }
            if (NS) {
#pragma unroll
                for (int ps = 0; ps < PS; ++ps) {
                    zs[ps] = __builtin_amdgcn_raw_buffer_load_b64(rz, co_off[CS - 1] + pix_off[ps], 0, 0);
                    ys[ps] = __builtin_amdgcn_raw_buffer_load_b64(ry, co_off[CS - 1] + pix_off[ps], 0, 0);
                }
            }
        }
    }
    compute(p.nbuf == 2 ? ((p.n_chunks - 1) & 1) : 0);

    // ---- epilogue: scale/shift, residuals (fetched before the MFMA loop), ReLU, one rounding, 16-byte stores per tile pair
    const bool has1 = p.res1 != nullptr, has2 = p.res2 != nullptr;
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) {
            const u32x4 a1 = has1 ? r1p[j][ps] : (u32x4){0u, 0u, 0u, 0u}, a2 = has2 ? r2p[j][ps] : (u32x4){0u, 0u, 0u, 0u};
            u32x2 lo = f16_pack4(f16_epi4(acc[ps][2 * j], sc[2 * j], sh[2 * j], has1, (u32x2){a1.x, a1.y}, has2, (u32x2){a2.x, a2.y}, p.relu));
            u32x2 hi = f16_pack4(f16_epi4(acc[ps][2 * j + 1], sc[2 * j + 1], sh[2 * j + 1], has1, (u32x2){a1.z, a1.w}, has2, (u32x2){a2.z, a2.w}, p.relu));
            if constexpr (STATS) {
                const bool valid = pix_off[ps] != kInv;
                if constexpr (STATS == 2) {
                    const u32x4 zq = zp[j][ps], yq = yp[j][ps];
                    f16_stats_acc<2>(lo, valid, st_a[2 * j], st_b[2 * j], (u32x2){zq.x, zq.y}, (u32x2){yq.x, yq.y}, p.st_relu);
                    f16_stats_acc<2>(hi, valid, st_a[2 * j + 1], st_b[2 * j + 1], (u32x2){zq.z, zq.w}, (u32x2){yq.z, yq.w}, p.st_relu);
                } else {
                    f16_stats_acc<1>(lo, valid, st_a[2 * j], st_b[2 * j], lo, lo, 0);
                    f16_stats_acc<1>(hi, valid, st_a[2 * j + 1], st_b[2 * j + 1], hi, hi, 0);
                }
            }
            __builtin_amdgcn_raw_buffer_store_b128((u32x4){lo.x, lo.y, hi.x, hi.y}, rs_o, co_off[2 * j] + pix_off[ps], 0, 0);
        }
    if (NS) {
#pragma unroll
        for (int ps = 0; ps < PS; ++ps) {
            u32x2 o = f16_pack4(f16_epi4(acc[ps][CS - 1], sc[CS - 1], sh[CS - 1], has1, has1 ? r1s[ps] : (u32x2){0u, 0u}, has2,
                                         has2 ? r2s[ps] : (u32x2){0u, 0u}, p.relu));
            if constexpr (STATS) {
                const bool valid = pix_off[ps] != kInv;
                if constexpr (STATS == 2) f16_stats_acc<2>(o, valid, st_a[CS - 1], st_b[CS - 1], zs[ps], ys[ps], p.st_relu);
                else f16_stats_acc<1>(o, valid, st_a[CS - 1], st_b[CS - 1], o, o, 0);
            }
            __builtin_amdgcn_raw_buffer_store_b64(o, rs_o, co_off[CS - 1] + pix_off[ps], 0, 0);
        }
    }
    if constexpr (STATS)
        f16_stats_flush<CS, WAVES_P, WAVES_C>(st_a, st_b, reinterpret_cast<float*>(smem16), p.st_part, p.st_nparts, part_idx, ct * CT,
                                              p.C8out, wp_i, wc_i, lq, lr);
}


template <int KS, int S, int PS, int CS, int WAVES_P, int WAVES_C, int NI, int NW, int OCC, bool ONE_CHUNK = false, int STATS = 0>
__global__ __launch_bounds__(256, OCC) void conv_f16_kernel(const ConvF16Params p) {
    conv_f16_body<KS, S, PS, CS, WAVES_P, WAVES_C, NI, NW, OCC, ONE_CHUNK, STATS>(p, (int)blockIdx.x, (int)blockIdx.y);
}

// regular: big chunks, two workgroups per CU; light: small chunks / few staging registers, three per CU (<= 52 KiB LDS)
constexpr int f16_ni(int ks, bool light) { return light ? 5 : 10; }
constexpr int f16_nw(int ks, bool light) { return light ? 5 : (ks == 3 ? 9 : 8); }  // ks 2 (deconv phases): 8
constexpr int f16_occ(bool light) { return light ? 3 : 2; }

// the kernel of variant V (a row of kF16Variants) for this kernel size, stride and statistics mode
template <int KS, int S, int V, int STATS>
int launch_f16_kernel(const ConvF16Params& p, size_t lds_bytes, hipStream_t s) {
    if (g_dry_launch) return MP_OK;  // mp_f16_conv_supported: the dispatch alone
    constexpr F16Variant v = kF16Variants[V];
    constexpr auto kern = conv_f16_kernel<KS, S, v.ps, v.cs, v.waves_p, 4 / v.waves_p, f16_ni(KS, v.light), f16_nw(KS, v.light),
                                          v.one_chunk ? 2 : f16_occ(v.light), v.one_chunk, STATS>;
    return launch_lds<kern>(dim3(p.total_blocks, p.phases > 1 ? p.phases : 1), dim3(256), lds_bytes, s, p);
}

template <int KS, int S>
int launch_f16_ks(const ConvF16Params& p, int variant, size_t lds_bytes, hipStream_t s) {
    return f16_dispatch_variant<kF16Tile>(variant, [&](auto v) {
        if (kF16Variants[v].one_chunk && p.n_chunks != 1) return (int)MP_ERR_UNSUPPORTED;
        return f16_dispatch_stats<KS, S>(p.st_mode, [&](auto stats) { return launch_f16_kernel<KS, S, v, stats>(p, lds_bytes, s); });
    });
}

const int kLdsMax = 150 * 1024;
const int kLdsBudget = 78 * 1024;  // two workgroups per CU

// The LDS-operand kernels (one-tile, multi-tile) stage only the columns the taps reach - widened to the whole padded row when that
// costs at most two columns - in units of 16 bytes: ncols per row, upc per plane.  False: no column of the input is reached.
bool f16_geom_lds_tile(ConvF16Params& p, int KS, int S) {
    int wp = (p.Wo - 1) * S + KS;
    if (wp < p.pad_l + p.W && p.pad_l + p.W - wp <= 2) wp = p.pad_l + p.W;
    f16_geom_planes(p, KS, S, wp, 0);
    p.ncols = p.W < p.Wp - p.pad_l ? p.W : p.Wp - p.pad_l;
    if (p.ncols < 1) return false;
    p.upc = p.G * p.Rin * p.ncols;
    return true;
}
// ... and what follows from the chosen tile: buffer sizes, tile counts, the staging and pixel magics, the staging slots in use
void f16_geom_lds_finish(ConvF16Params& p, int T, int CT) {
    p.in_buf = p.PK * p.plane;
    p.w_buf = p.PK * T * CT;
    f16_geom_tiles(p, CT);
    p.magic_upc = magic_of(p.upc);
    p.magic_ncols = magic_of(p.ncols);
    p.magic_rin = magic_of(p.Rin);
    f16_geom_pixel_magics(p);
    p.ni_used = (p.PKs * p.upc + 255) / 256;
}

// persistent multi-tile geometry: whole K in one "chunk", weights resident, two input buffers
bool f16_configure_mt(const mp_conv_desc& d, int variant, ConvF16Launch& L) {
    const int CT = f16_variant_ct(variant), PT = f16_variant_pt(variant);
    ConvF16Params& p = L.p;
    const int S = d.stride, KS = d.kh, T = KS * KS;
    if (!(KS == 3 || ((KS == 1 || KS == 2) && S == 1))) return false;
    const int occ = f16_variant(variant).occ;
    f16_geom_tensors(d, p);
    if (!f16_geom_offsets_fit(d, p)) return false;
    p.PK = round_up(d.cin, 32) / 8;
    p.PKs = p.C8in < p.PK ? p.C8in : p.PK;
    p.n_chunks = 1;
    if (p.Wo > PT) return false;
    const int ni = f16_mt_ni(occ);
    const long long budget = occ == 2 ? kLdsBudget : kLdsMax;
    int rows_fit = PT / p.Wo;
    if (rows_fit > p.Ho) rows_fit = p.Ho;
    bool found = false;
    // double-buffered input tiles first; the one-workgroup-per-CU build may fall back to ONE input buffer for large-K layers
    // (weights + one tile fill LDS): the next tile still flies into registers under the MFMA loop, only its LDS write waits
    for (int nbuf = 2; nbuf >= (occ == 1 ? 1 : 2) && !found; --nbuf)
    for (int R = rows_fit; R >= 1 && !found; --R) {
        p.nbuf = nbuf;
        f16_geom_fit(p, R, PT);
        if (!f16_geom_lds_tile(p, KS, S)) return false;
        if ((long long)p.PKs * p.upc > (long long)ni * 256) continue;
        const long long bytes = ((long long)p.PK * T * CT + (long long)nbuf * p.PK * p.plane) * 16;
        if (bytes > budget) continue;
        found = true;
    }
    if (!found) return false;
    f16_geom_lds_finish(p, T, CT);
    int max_groups = f16_geom_groups(occ, p.n_ct, "MP_F16_MT_GROUPS");
    if (max_groups < 1) max_groups = 1;
    if (!f16_geom_runs(p, max_groups)) return false;
    p.nw_used = 0;  // this kernel loads its weights once, outside the staging slots
    L.ks = KS; L.stride = S; L.variant = variant;
    L.lds_bytes = (size_t)(p.w_buf + p.nbuf * p.in_buf) * 16;
    return L.lds_bytes <= (size_t)kLdsMax;
}

bool f16_configure(const mp_conv_desc& d, int variant, ConvF16Launch& L) {
    if (f16_variant_ws(variant)) return f16_configure_ws(d, variant, L);
    if (f16_variant_wreg(variant)) return f16_configure_wreg(d, variant, L);
    if (f16_variant_mt(variant)) return f16_configure_mt(d, variant, L);
    const int CT = f16_variant_ct(variant), PT = f16_variant_pt(variant);
    ConvF16Params& p = L.p;
    const int S = d.stride, KS = d.kh, T = KS * KS;
    f16_geom_tensors(d, p);
    const int planes_total = round_up(d.cin, 32) / 8;
    if (p.Wo > PT) return false;
    const bool light = f16_variant(variant).light;
    const int ni = f16_ni(KS, light), nw = f16_nw(KS, light);
    int rows_fit = PT / p.Wo;
    if (rows_fit > p.Ho) rows_fit = p.Ho;
    bool found = false;
    for (int pass = 0; pass < 2 && !found; ++pass) {  // pass 0: two workgroups per CU, pass 1: whatever fits
        const long long budget = pass == 0 ? (light ? 52 * 1024 : kLdsBudget) : kLdsMax;
        if (pass == 1 && light) break;  // a light build that cannot run three per CU has no point
        for (int R = rows_fit; R >= 1 && !found; --R) {
            f16_geom_fit(p, R, PT);
            if (!f16_geom_lds_tile(p, KS, S)) return false;
            for (int pk = planes_total; pk >= 4; pk -= 4) {
                if (planes_total % pk) continue;
                const int n_chunks = planes_total / pk;
                const int pks = (n_chunks == 1 && p.C8in < pk) ? p.C8in : pk;
                if ((long long)pks * p.upc > (long long)ni * 256) continue;
                if ((long long)pk * T * CT > (long long)nw * 256) continue;
                const int nbuf = n_chunks > 1 ? 2 : 1;
                const long long bytes = (long long)nbuf * (pk * p.plane + pk * T * CT) * 16;
                if (bytes > budget) continue;
                p.PK = pk; p.PKs = pks; p.n_chunks = n_chunks; p.nbuf = nbuf;
                found = true;
                break;
            }
        }
    }
    if (!found) return false;
    if (f16_variant(variant).one_chunk && p.n_chunks != 1) return false;  // single-chunk build
    f16_geom_lds_finish(p, T, CT);
    p.total_blocks = p.n_ct * p.tiles_y * p.tiles_n;
    p.nw_used = (p.PK * T * CT + 255) / 256;
    p.step_rows = 256 / p.ncols;  // slot-to-slot stepping of the staging table: 256 units = step_rows rows + step_cols columns
    p.step_cols = 256 % p.ncols;
    p.magic_rows = magic_of((unsigned)(p.G * p.Rin));
    L.ks = KS; L.stride = S; L.variant = variant;
    L.lds_bytes = (size_t)p.nbuf * (p.in_buf + p.w_buf) * 16;
    return L.lds_bytes <= (size_t)kLdsMax;
}

int f16_validate(const mp_conv_desc* d) {
    if (!d) return MP_ERR_NULL;
    if (d->n <= 0 || d->cin <= 0 || d->h <= 0 || d->w <= 0 || d->cout <= 0) return MP_ERR_SHAPE;
    if (d->kh != d->kw || !(d->kh == 1 || d->kh == 2 || d->kh == 3)) return MP_ERR_UNSUPPORTED;
    if (!(d->stride == 1 || d->stride == 2) || (d->kh == 2 && d->stride != 1)) return MP_ERR_UNSUPPORTED;
    if (d->pad_top < 0 || d->pad_left < 0 || d->pad_top > d->kh || d->pad_left > d->kw) return MP_ERR_SHAPE;
    if (d->conv_h <= 0 || d->conv_w <= 0) return MP_ERR_SHAPE;
    // plain or strided-scatter output mapping (sub-pixel phases of the transposed convolution); replication (nearest
    // up-sampling) is not part of this kernel: the exchange unit has its own streaming kernel in this layout
    if (d->out_rep != 1 || d->out_mul < 1 || d->out_off_y < 0 || d->out_off_x < 0 || (d->flags & ~(MP_CONV_SHARES_CUS | MP_CONV_PHASES4)))
        return MP_ERR_UNSUPPORTED;
    const int ph = (d->flags & MP_CONV_PHASES4) ? 1 : 0;  // the four phases reach one pixel further than phase (0, 0)
    if (ph && (d->kh != 2 || d->stride != 1 || d->out_mul != 2 || d->out_off_y != 0 || d->out_off_x != 0)) return MP_ERR_UNSUPPORTED;
    if (d->out_h <= 0 || d->out_w <= 0) return MP_ERR_SHAPE;
    if ((d->conv_h - 1) * d->out_mul + d->out_off_y + ph >= d->out_h || (d->conv_w - 1) * d->out_mul + d->out_off_x + ph >= d->out_w)
        return MP_ERR_SHAPE;
    // every input row / column a tap reads must exist or be zero padding on the top / left only up to pad; the bottom /
    // right overhang is covered by the LDS halo, as in the fp32 kernel
    if ((long long)d->n * ((d->cout + 7) / 8) * d->out_h * d->out_w * 16 >= (1LL << 40)) return MP_ERR_UNSUPPORTED;
    return MP_OK;
}

// [Cout,Cin,kh,kw] fp32 -> [Cin_pad32/32][T][4][Cout_pad16][8] fp16 (round to nearest even), zero padded
// transposed = 1: the (py, px) 2x2 sub-pixel phase of a Conv2dTranspose(k=4, s=2, p=1) weight [Cin,Cout,4,4]
// source value of packed element (cout co, cin ci, tap t) - callers have checked co < cout && ci < cin
__device__ __forceinline__ float pack_f16_source(const float* __restrict__ w, int cout, int cin, int kh, int kw, int transposed,
                                                 int py, int px, int co, int ci, int t) {
    const int ty = t / kw, tx = t % kw;
    if (!transposed) return w[(((size_t)co * cin + ci) * kh + ty) * kw + tx];
    if (transposed == 2) {
        // data gradient of a stride-1 conv whose weight is [cin, cout, kh, kw] in forward terms (this packed conv's
        // cout = forward cin): roles swapped, taps mirrored
        return w[(((size_t)ci * cout + co) * kh + (kh - 1 - ty)) * kw + (kw - 1 - tx)];
    }
    if (transposed == 3) {
        // data gradient of a 3x3 stride-2 pad-1 conv, output parity phase (py, px), as a 2x2 conv over dy:
        // dx[2a+p] = sum_t dy[a+t] * w[k(p,t)],  k(0,0)=1, k(0,1)=none, k(1,0)=2, k(1,1)=0
        const int ky = py == 0 ? (ty == 0 ? 1 : -1) : (ty == 0 ? 2 : 0);
        const int kx = px == 0 ? (tx == 0 ? 1 : -1) : (tx == 0 ? 2 : 0);
        return (ky < 0 || kx < 0) ? 0.f : w[(((size_t)ci * cout + co) * 3 + ky) * 3 + kx];
    }
    if (transposed == 4) {
        // data gradient of the (py, px) sub-pixel phase of Conv2dTranspose(k=4, s=2, p=1): roles swapped (this packed
        // conv's cout = the transposed conv's cin) and the 2x2 phase taps mirrored; w is [cout, cin, 4, 4] in
        // this packed conv's terms
        const int my = 1 - ty, mx = 1 - tx;
        const int ky = py == 0 ? 3 - 2 * my : 2 - 2 * my;
        const int kx = px == 0 ? 3 - 2 * mx : 2 - 2 * mx;
        return w[(((size_t)co * cin + ci) * 4 + ky) * 4 + kx];
    }
    // out row 2m+py reads in row m-1+py+ty with kernel row 3-2*ty (py=0) or 2-2*ty (py=1); same along x
    const int ky = py == 0 ? 3 - 2 * ty : 2 - 2 * ty;
    const int kx = px == 0 ? 3 - 2 * tx : 2 - 2 * tx;
    return w[(((size_t)ci * cout + co) * 4 + ky) * 4 + kx];
}

__global__ __launch_bounds__(256) void pack_weight_f16_kernel(const float* __restrict__ w, _Float16* __restrict__ out,
                                                              int cout, int cin, int kh, int kw, int kq, int cout_pad16,
                                                              int transposed, int py, int px) {
    const int T = kh * kw;
    const size_t total = (size_t)kq * T * 4 * cout_pad16 * 8;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        size_t r = i >> 3;
        const int co = (int)(r % cout_pad16);
        r /= cout_pad16;
        const int g = (int)(r & 3);
        r >>= 2;
        const int t = (int)(r % T);
        const int q = (int)(r / T);
        const int ci = q * 32 + g * 8 + j;
        float v = 0.f;
        if (co < cout && ci < cin) v = pack_f16_source(w, cout, cin, kh, kw, transposed, py, px, co, ci, t);
        out[i] = (_Float16)v;
    }
}

// every weight of a training step in ONE launch: block b serves job j with first_block[j] <= b < first_block[j + 1] (binary
// search over the prefix table), a thread writes one 16-byte group of 8 input channels
__global__ __launch_bounds__(256) void pack_weight_f16_batch_kernel(const mp_f16_pack_job* __restrict__ jobs,
                                                                    const unsigned* __restrict__ first_block, int n_jobs) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first_block[mid] <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const mp_f16_pack_job jb = jobs[lo];
    const int T = jb.kh * jb.kw, cp = (jb.cout + 15) / 16 * 16, kq = (jb.cin + 31) / 32;
    // A thread takes one (cin group of 8, cout) pair and walks the T taps (the job owns units / 256 blocks = T times the threads
    // this needs: the rest leave at once).  A thread per packed 16-byte unit - taps across threads - read the fp32 master weights
    // through 8 dwords 4 T bytes apart, every line ~12 times per launch: 193 us of every training step for 171 MB.  Here the 8 T
    // source floats of a thread are ONE contiguous run (forward weights: 16-byte loads), or T-float runs that neighbouring lanes
    // continue (data-gradient weights: roles swapped) - every line is fetched once; the stores of a tap are 1 KB runs across lanes.
    const unsigned groups = (unsigned)kq * 4u * (unsigned)cp;
    const unsigned u = (blockIdx.x - first_block[lo]) * 256u + threadIdx.x;
    if (u >= groups) return;
    const int co = (int)(u % cp);
    const unsigned r = u / cp;
    const int g = (int)(r & 3), q = (int)(r >> 2);
    const int ci0 = q * 32 + g * 8;
    u32x4* __restrict__ out = reinterpret_cast<u32x4*>(jb.packed);
    const size_t t_stride = (size_t)4 * cp;  // units between consecutive taps of one (q, g, co)
    const size_t o0 = ((size_t)q * T * 4 + g) * cp + co;
    if (!jb.transposed && co < jb.cout && ci0 + 8 <= jb.cin && (T == 9 || T == 1) &&
        ((reinterpret_cast<uintptr_t>(jb.w) | ((size_t)jb.cin * T * 4)) & 15) == 0) {
        // forward weights [cout][cin][kh][kw]: the thread's 8 T floats are contiguous from (co cin + ci0) T
        const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(jb.w + ((size_t)co * jb.cin + ci0) * T);
        if (T == 9) {
            float v[72];
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                const f32x4 x = src[i];
                v[4 * i] = x[0]; v[4 * i + 1] = x[1]; v[4 * i + 2] = x[2]; v[4 * i + 3] = x[3];
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                f16x8 o;
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (_Float16)v[j * 9 + t];
                out[o0 + t * t_stride] = __builtin_bit_cast(u32x4, o);
            }
        } else {
            const f32x4 x0 = src[0], x1 = src[1];
            const f16x8 o = (f16x8){(_Float16)x0[0], (_Float16)x0[1], (_Float16)x0[2], (_Float16)x0[3],
                                    (_Float16)x1[0], (_Float16)x1[1], (_Float16)x1[2], (_Float16)x1[3]};
            out[o0] = __builtin_bit_cast(u32x4, o);
        }
        return;
    }
    for (int t = 0; t < T; ++t) {
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ci = ci0 + j;
            float v = 0.f;
            if (co < jb.cout && ci < jb.cin)
                v = pack_f16_source(jb.w, jb.cout, jb.cin, jb.kh, jb.kw, jb.transposed, jb.phase_y, jb.phase_x, co, ci, t);
            o[j] = (_Float16)v;
        }
        out[o0 + t * t_stride] = __builtin_bit_cast(u32x4, o);
    }
}

// NCHW fp32 -> c8 fp16: one thread per (n, block, pixel): 8 strided plane reads (coalesced across lanes), one 16-B store
__global__ __launch_bounds__(256) void to_c8_kernel(const float* __restrict__ x, u32x4* __restrict__ out, int n, int c, int hw) {
    const int c8 = (c + 7) >> 3;
    const size_t total = (size_t)n * c8 * hw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pix = (int)(i % hw);
        const size_t r = i / hw;
        const int blk = (int)(r % c8);
        const size_t img = r / c8;
        f16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ch = blk * 8 + j;
            v[j] = ch < c ? (_Float16)x[(img * c + ch) * hw + pix] : (_Float16)0.f;
        }
        out[i] = __builtin_bit_cast(u32x4, v);
    }
}

// c8 fp16 -> NCHW fp32
__global__ __launch_bounds__(256) void from_c8_kernel(const u32x4* __restrict__ x, float* __restrict__ out, int n, int c, int hw) {
    const int c8 = (c + 7) >> 3;
    const size_t total = (size_t)n * c8 * hw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int pix = (int)(i % hw);
        const size_t r = i / hw;
        const int blk = (int)(r % c8);
        const size_t img = r / c8;
        const f16x8 v = __builtin_bit_cast(f16x8, x[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ch = blk * 8 + j;
            if (ch < c) out[(img * c + ch) * hw + pix] = (float)v[j];
        }
    }
}

// exchange-unit sum in the c8 layout: out = act(((base + up(t1)) + up(t2)) + up(t3)), nearest up-sampling by s_i;
// fp32 sums in the reference's term order, one rounding to fp16
__global__ __launch_bounds__(256) void fuse_sum_f16_kernel(const u32x4* __restrict__ base, const u32x4* __restrict__ t1, int s1,
                                                           const u32x4* __restrict__ t2, int s2, const u32x4* __restrict__ t3,
                                                           int s3, u32x4* __restrict__ out, int planes, int h, int w, int relu) {
    const size_t total = (size_t)planes * h * w;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % w);
        const size_t r = i / w;
        const int y = (int)(r % h);
        const size_t pl = r / h;
        const f16x8 bv = __builtin_bit_cast(f16x8, base[i]);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)bv[j];
        auto add = [&](const u32x4* __restrict__ t, int s) {
            const int hs = h / s, ws = w / s;
            const f16x8 tv = __builtin_bit_cast(f16x8, t[(pl * hs + y / s) * ws + x / s]);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] += (float)tv[j];
        };
        add(t1, s1);
        if (t2) add(t2, s2);
        if (t3) add(t3, s3);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (_Float16)(relu ? fmaxf(v[j], 0.f) : v[j]);
        out[i] = __builtin_bit_cast(u32x4, o);
    }
}

// The same sum with 32-bit index arithmetic: divisions by w and h through reciprocal multiplication, the power-of-two scale
// factors of HRNet's exchange units (2, 4, 8: hrnet.py:296-312) as shifts.  The generic kernel above spends two 64-bit and eight
// 32-bit integer divisions per 16-byte element - more instruction time than its memory traffic takes on the large maps.
__global__ __launch_bounds__(256) void fuse_sum_f16_fast_kernel(const u32x4* __restrict__ base, const u32x4* __restrict__ t1, int sh1,
                                                                const u32x4* __restrict__ t2, int sh2, const u32x4* __restrict__ t3,
                                                                int sh3, u32x4* __restrict__ out, unsigned total, unsigned h, unsigned w,
                                                                unsigned magic_h, unsigned magic_w, int relu) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const unsigned r = fastdiv(i, w, magic_w), x = i - r * w;
        const unsigned pl = fastdiv(r, h, magic_h), y = r - pl * h;
        const u32x4 bq = base[i];
        const u32x4 q1 = t1[(pl * (h >> sh1) + (y >> sh1)) * (w >> sh1) + (x >> sh1)];
        u32x4 q2 = (u32x4){0u, 0u, 0u, 0u}, q3 = q2;
        if (t2) q2 = t2[(pl * (h >> sh2) + (y >> sh2)) * (w >> sh2) + (x >> sh2)];
        if (t3) q3 = t3[(pl * (h >> sh3) + (y >> sh3)) * (w >> sh3) + (x >> sh3)];
        const f16x8 bv = __builtin_bit_cast(f16x8, bq), v1 = __builtin_bit_cast(f16x8, q1), v2 = __builtin_bit_cast(f16x8, q2),
                    v3 = __builtin_bit_cast(f16x8, q3);
        f16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = (float)bv[j] + (float)v1[j];  // the reference's term order; absent terms add +0 (exact)
            if (t2) v += (float)v2[j];
            if (t3) v += (float)v3[j];
            o[j] = (_Float16)(relu ? fmaxf(v, 0.f) : v);
        }
        out[i] = __builtin_bit_cast(u32x4, o);
    }
}

int grid_for(size_t total) {
    size_t blocks = (total + 255) / 256;
    return (int)(blocks > 8192 ? 8192 : (blocks < 1 ? 1 : blocks));
}

}  // namespace

int f16_build_launch(const mp_conv_desc* desc, int variant, const void* x, const void* w, const float* scale,
                     const float* shift, const void* res1, const void* res2, void* out, ConvF16Launch& L) {
    int rc = f16_validate(desc);
    if (rc != MP_OK) return rc;
    if (!x || !w || !scale || !shift || !out) return MP_ERR_NULL;
    if (variant >= F_COUNT) return MP_ERR_UNSUPPORTED;
    // output offsets are 32-bit sums of masked parts (kInv in conv_f16_dev.h)
    if ((size_t)desc->n * ((desc->cout + 7) / 8) * desc->out_h * desc->out_w * 16 >= 0x60000000u) return MP_ERR_UNSUPPORTED;
    bool ok = false;
    const bool phases4 = (desc->flags & MP_CONV_PHASES4) != 0;
    if (phases4 && (res1 || res2)) return MP_ERR_UNSUPPORTED;
    if (variant >= 0) {
        if ((f16_variant_wreg(variant) || f16_variant_ws(variant)) && phases4) return MP_ERR_UNSUPPORTED;  // one-tile / multi-tile kernels only
        if (f16_variant_ws(variant) && res2) return MP_ERR_UNSUPPORTED;
        if (f16_variant_wreg(variant) && res2 && desc->stride != 2) return MP_ERR_UNSUPPORTED;  // second residual: stride-2 builds only
        ok = f16_configure(*desc, variant, L);
    } else {
        // heuristic: widest cout tile that divides the padded couts, 192-pixel tiles unless the grid would not fill the chip
        const int c16 = round_up(desc->cout, 16);
        int order[5], n = 0;
        if (c16 % 64 == 0) { order[n++] = F_CT64_PT192; order[n++] = F_CT64_PT96; order[n++] = F_CT32_PT192; order[n++] = F_CT32_PT96; }
        else if (c16 % 48 == 0) { order[n++] = F_CT48_PT192; order[n++] = F_CT64_PT96; order[n++] = F_CT32_PT192; }
        else { order[n++] = F_CT32_PT192; order[n++] = F_CT32_PT96; order[n++] = F_CT64_PT96; }
        double best = -1;
        for (int i = 0; i < n; ++i) {
            ConvF16Launch c{};
            if (!f16_configure(*desc, order[i], c)) continue;
            const double pix_eff = (double)(c.p.G * c.p.RWo) / f16_variant_pt(order[i]);
            const double co_eff = (double)desc->cout / (c.p.n_ct * f16_variant_ct(order[i]));
            const double waves = (double)c.p.total_blocks / 512.0;
            const double fill = waves >= 1.0 ? waves / (double)((long long)waves + ((waves - (long long)waves) > 1e-9 ? 1 : 0)) : waves;
            const double score = pix_eff * co_eff * fill;
            if (score > best * 1.02) { best = score; L = c; ok = true; }
        }
    }
    if (!ok) return MP_ERR_UNSUPPORTED;
    L.p.x = x; L.p.wp = w; L.p.scale = scale; L.p.shift = shift; L.p.res1 = res1; L.p.res2 = res2; L.p.out = out;
    L.p.phases = phases4 ? 4 : 1;
    L.p.w_phase_bytes = phases4 ? (unsigned)((size_t)round_up(desc->cin, 32) * 4 * round_up(desc->cout, 16) * 2) : 0u;
    return MP_OK;
}

int f16_stats_parts(const ConvF16Launch& L) {
    // tile / weights-in-registers kernels: one slot per pixel tile; persistent multi-tile kernel: one per workgroup run; per phase
    return ((f16_variant_mt(L.variant) || f16_variant_ws(L.variant)) ? L.p.n_groups : L.p.tiles_y * L.p.tiles_n) * (L.p.phases > 1 ? L.p.phases : 1);
}

int f16_launch(const ConvF16Launch& L, hipStream_t s) {
    if (f16_variant_ws(L.variant)) return f16_ws_launch(L, s);
    if (f16_variant_wreg(L.variant)) return f16_wreg_launch(L, s);
    if (f16_variant_mt(L.variant)) return f16_mt_launch(L, s);
    if (L.ks == 1) return L.stride == 1 ? launch_f16_ks<1, 1>(L.p, L.variant, L.lds_bytes, s) : launch_f16_ks<1, 2>(L.p, L.variant, L.lds_bytes, s);
    if (L.ks == 2) return launch_f16_ks<2, 1>(L.p, L.variant, L.lds_bytes, s);
    if (L.ks == 3) return L.stride == 1 ? launch_f16_ks<3, 1>(L.p, L.variant, L.lds_bytes, s) : launch_f16_ks<3, 2>(L.p, L.variant, L.lds_bytes, s);
    return MP_ERR_UNSUPPORTED;
}

}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_f16_packed_weight_bytes(int cout, int cin, int kh, int kw) {
    if (cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) return 0;
    return (size_t)round_up(cin, 32) * kh * kw * round_up(cout, 16) * 2;
}

size_t mp_f16_activation_bytes(int n, int c, int h, int w) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)n * ((c + 7) / 8) * h * w * 16;
}

int mp_f16_pack_weight(const float* w, void* packed, int cout, int cin, int kh, int kw, int transposed, int phase_y, int phase_x,
                       mp_stream_t stream) {
    if (!w || !packed) return MP_ERR_NULL;
    if (cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) return MP_ERR_SHAPE;
    if (transposed < 0 || transposed > 4) return MP_ERR_UNSUPPORTED;
    if ((transposed == 1 || transposed == 3 || transposed == 4) && (kh != 2 || kw != 2 || phase_y < 0 || phase_y > 1 || phase_x < 0 || phase_x > 1))
        return MP_ERR_UNSUPPORTED;
    const int kq = round_up(cin, 32) / 32, cp = round_up(cout, 16);
    const size_t total = (size_t)kq * kh * kw * 4 * cp * 8;
    hipLaunchKernelGGL(pack_weight_f16_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), w,
                       reinterpret_cast<_Float16*>(packed), cout, cin, kh, kw, kq, cp, transposed, phase_y, phase_x);
    return check_launch();
}

int mp_f16_pack_weight_batch(const mp_f16_pack_job* jobs_dev, const unsigned* first_block_dev, int n_jobs, unsigned total_blocks,
                             mp_stream_t stream) {
    if (n_jobs == 0) return MP_OK;
    if (!jobs_dev || !first_block_dev) return MP_ERR_NULL;
    if (n_jobs < 0 || total_blocks == 0) return MP_ERR_SHAPE;
    hipLaunchKernelGGL(pack_weight_f16_batch_kernel, dim3(total_blocks), dim3(256), 0, as_stream(stream), jobs_dev, first_block_dev,
                       n_jobs);
    return check_launch();
}

int mp_f16_to_c8(const float* x, void* out, int n, int c, int h, int w, mp_stream_t stream) {
    if (!x || !out) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    const size_t total = (size_t)n * ((c + 7) / 8) * h * w;
    hipLaunchKernelGGL(to_c8_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), x, reinterpret_cast<u32x4*>(out), n, c, h * w);
    return check_launch();
}

int mp_f16_from_c8(const void* x, float* out, int n, int c, int h, int w, mp_stream_t stream) {
    if (!x || !out) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    const size_t total = (size_t)n * ((c + 7) / 8) * h * w;
    hipLaunchKernelGGL(from_c8_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), reinterpret_cast<const u32x4*>(x), out, n, c, h * w);
    return check_launch();
}

int mp_f16_conv2d_fwd(const mp_conv_desc* desc, int variant, const void* x, const void* packed_w, const float* scale,
                      const float* shift, const void* res1, const void* res2, void* out, mp_stream_t stream) {
    ConvF16Launch L{};
    int rc = f16_build_launch(desc, variant, x, packed_w, scale, shift, res1, res2, out, L);
    if (rc != MP_OK) return rc;
    return f16_launch(L, as_stream(stream));
}

static bool f16_stats_shape_ok(const mp_conv_desc* d) {
    // 1x1 / 3x3 convs, and the merged phase launch of a stride-2 data gradient (backward sums)
    return (d->kh == 1 || d->kh == 3 || (d->kh == 2 && (d->flags & MP_CONV_PHASES4))) && d->out_rep == 1;
}

int mp_f16_conv_stats_parts(const mp_conv_desc* desc, int variant) {
    if (!desc || f16_validate(desc) != MP_OK || variant >= F_COUNT || !f16_stats_shape_ok(desc)) return 0;
    ConvF16Launch L{};
    // the launch geometry exactly as mp_f16_conv2d_fwd_stats builds it (variant < 0: the library's deterministic heuristic);
    // the pointers only travel into the parameter block
    const void* dummy = reinterpret_cast<const void*>(static_cast<uintptr_t>(16));
    if (f16_build_launch(desc, variant, dummy, dummy, reinterpret_cast<const float*>(dummy), reinterpret_cast<const float*>(dummy), nullptr,
                         nullptr, const_cast<void*>(dummy), L) != MP_OK)
        return 0;
    return f16_stats_parts(L);
}

int mp_f16_conv_pre_supported(const mp_conv_desc* desc, int variant) {
    if (!desc || variant < 0 || variant >= F_COUNT || f16_validate(desc) != MP_OK || !f16_stats_shape_ok(desc)) return 0;
    ConvF16Launch L{};
    const void* dummy = reinterpret_cast<const void*>(static_cast<uintptr_t>(16));
    if (f16_build_launch(desc, variant, dummy, dummy, reinterpret_cast<const float*>(dummy), reinterpret_cast<const float*>(dummy), nullptr,
                         nullptr, const_cast<void*>(dummy), L) != MP_OK)
        return 0;
    // the conditions of mp_f16_conv2d_fwd_stats for stats->pre_scale_dev
    return (f16_variant_wreg(L.variant) && L.ks == 3 && L.stride == 1 && L.p.upc > 0 && L.p.G == 1) ? 1 : 0;
}

// everything mp_f16_conv2d_fwd_stats checks and fills in before the launch (shared with the mp_f16_conv_supported query)
static int f16_prepare_stats(const mp_conv_desc* desc, int variant, const void* x, const void* packed_w, const float* scale, const float* shift,
                             const void* res1, void* out, const mp_f16_conv_stats* st, ConvF16Launch& L) {
    if (!st || !st->partials_dev) return MP_ERR_NULL;
    int rc = f16_build_launch(desc, variant, x, packed_w, scale, shift, res1, nullptr, out, L);
    if (rc != MP_OK) return rc;
    const bool phases4 = (desc->flags & MP_CONV_PHASES4) != 0;
    // ONE phase (py, px) = (out_off_y, out_off_x) of a stride-2 data gradient launched on its own (backward sums only): it fills its
    // quarter of the partials the merged MP_CONV_PHASES4 launch of the same variant would leave - slot  phase * (slots per phase) +
    // tile - so four such launches and the merged one hand the BatchNorm the same sums in the same order
    const bool one_phase = !phases4 && desc->kh == 2 && desc->stride == 1 && desc->out_mul == 2 && desc->out_rep == 1 &&
                           desc->out_off_y <= 1 && desc->out_off_x <= 1 && st->mode == 2;
    if (!f16_stats_shape_ok(desc) && !one_phase) return MP_ERR_UNSUPPORTED;
    if (st->mode != 1 && st->mode != 2) return MP_ERR_UNSUPPORTED;
    if (phases4 && st->mode != 2) return MP_ERR_UNSUPPORTED;
    if (one_phase && (f16_variant_wreg(L.variant) || f16_variant_ws(L.variant))) return MP_ERR_UNSUPPORTED;  // as the merged launch
    const int per_phase = f16_stats_parts(L);
    const int parts = one_phase ? 4 * per_phase : per_phase;
    if (st->partials_bytes < (size_t)L.p.C8out * parts * 16 * sizeof(float)) return MP_ERR_WORKSPACE;
    L.p.st_mode = st->mode;
    L.p.st_nparts = parts;
    L.p.st_part = st->partials_dev + (one_phase ? (size_t)(2 * desc->out_off_y + desc->out_off_x) * per_phase * 16 : (size_t)0);
    if (st->mode == 2) {
        if (!st->z_dev || (st->relu != 0 && !st->y_dev)) return MP_ERR_NULL;
        if (desc->stride != 1 || desc->out_mul != ((phases4 || one_phase) ? 2 : 1) ||
            (!one_phase && (desc->out_off_y != 0 || desc->out_off_x != 0)))
            return MP_ERR_UNSUPPORTED;
        L.p.st_relu = st->relu != 0 ? 1 : 0;
        L.p.st_z = st->z_dev;
        L.p.st_y = st->relu != 0 ? st->y_dev : nullptr;
    }
    if (st->pre_scale_dev || st->pre_shift_dev || st->pre_out_dev) {
        // BatchNorm apply on the input operand: the fast staging form of the weights-in-registers kernel (decoded pieces, one image
        // per tile), forward statistics mode
        if (!st->pre_scale_dev || !st->pre_shift_dev) return MP_ERR_NULL;
        if (st->mode != 1 || !f16_variant_wreg(L.variant) || L.ks != 3 || L.stride != 1 || L.p.upc <= 0 || L.p.G != 1) return MP_ERR_UNSUPPORTED;
        L.p.pre_scale = st->pre_scale_dev;
        L.p.pre_shift = st->pre_shift_dev;
        L.p.pre_out = st->pre_out_dev;
        L.p.pre_relu = st->pre_relu != 0 ? 1 : 0;
    }
    return MP_OK;
}

int mp_f16_conv2d_fwd_stats(const mp_conv_desc* desc, int variant, const void* x, const void* packed_w, const float* scale,
                            const float* shift, const void* res1, void* out, const mp_f16_conv_stats* st, mp_stream_t stream) {
    ConvF16Launch L{};
    const int rc = f16_prepare_stats(desc, variant, x, packed_w, scale, shift, res1, out, st, L);
    if (rc != MP_OK) return rc;
    return f16_launch(L, as_stream(stream));
}

// the launch exactly as the entry points build it, on placeholder pointers (nothing is dereferenced on the host), then the
// family's own dispatch with the leaf launch switched off: whatever the entry would answer, by construction
static const void* const kF16Dummy = reinterpret_cast<const void*>(static_cast<uintptr_t>(16));
static int f16_dry_build(const mp_conv_desc* desc, int variant, int n_res, int stats_mode, ConvF16Launch& L, int& dry_rc) {
    const void* dummy = kF16Dummy;
    const float* fdummy = reinterpret_cast<const float*>(dummy);
    int rc;
    if (stats_mode == 0) {
        rc = f16_build_launch(desc, variant, dummy, dummy, fdummy, fdummy, n_res >= 1 ? dummy : nullptr, n_res >= 2 ? dummy : nullptr,
                              const_cast<void*>(dummy), L);
    } else {
        mp_f16_conv_stats st{};
        st.mode = stats_mode;
        st.relu = 1;
        st.partials_dev = reinterpret_cast<float*>(const_cast<void*>(dummy));
        st.partials_bytes = ~(size_t)0;
        st.z_dev = dummy;
        st.y_dev = dummy;
        rc = f16_prepare_stats(desc, variant, dummy, dummy, fdummy, fdummy, n_res >= 1 ? dummy : nullptr, const_cast<void*>(dummy), &st, L);
    }
    dry_rc = rc;
    if (rc != MP_OK) return rc;
    g_dry_launch = true;
    dry_rc = f16_launch(L, nullptr);
    g_dry_launch = false;
    return rc;
}

static bool f16_query_args_ok(const mp_conv_desc* desc, int n_res, int stats_mode) {
    return desc && n_res >= 0 && n_res <= 2 && stats_mode >= 0 && stats_mode <= 2 && !(stats_mode != 0 && n_res > 1);
}

int mp_f16_conv_supported(const mp_conv_desc* desc, int variant, int n_res, int stats_mode) {
    if (!f16_query_args_ok(desc, n_res, stats_mode)) return 0;
    ConvF16Launch L{};
    int dry_rc;
    return f16_dry_build(desc, variant, n_res, stats_mode, L, dry_rc) == MP_OK && dry_rc == MP_OK ? 1 : 0;
}

int mp_f16_conv_launch_words(const mp_conv_desc* desc, int variant, int n_res, int stats_mode, int64_t* out, int cap) {
    if (!out) return MP_ERR_NULL;
    if (!f16_query_args_ok(desc, n_res, stats_mode)) return MP_ERR_SHAPE;
    ConvF16Launch L{};
    int dry_rc;
    const int rc = f16_dry_build(desc, variant, n_res, stats_mode, L, dry_rc);
    const ConvF16Params& p = L.p;
    const int64_t head[2] = {rc, dry_rc};
    const int64_t body[] = {
        L.ks, L.stride, L.variant, (int64_t)L.lds_bytes,
        // scalar fields in declaration order
        p.N, p.C8in, p.H, p.W, p.Cout, p.Cout_pad16, p.C8out, p.Ho, p.Wo, p.pad_t, p.pad_l, p.R, p.G, p.Rin, p.Wp, p.img_plane, p.plane,
        p.PK, p.PKs, p.n_chunks, p.n_ct, p.tiles_y, p.tiles_n, p.ncols, p.upc, p.in_buf, p.w_buf, p.nbuf, p.relu, p.out_h, p.out_w,
        p.out_mul, p.off_y, p.off_x, p.magic_upc, p.magic_ncols, p.magic_rin, p.magic_rwo, p.magic_wo, p.RWo, p.total_blocks, p.phases,
        p.w_phase_bytes, p.tiles_total, p.tiles_per_wg, p.n_groups, p.ni_used, p.nw_used, p.magic_rows, p.step_rows, p.step_cols,
        p.st_mode, p.st_nparts, p.st_relu, p.pre_relu,
        // pointer fields: null / set
        p.x != nullptr, p.wp != nullptr, p.scale != nullptr, p.shift != nullptr, p.res1 != nullptr, p.res2 != nullptr, p.out != nullptr,
        p.st_part != nullptr, p.st_z != nullptr, p.st_y != nullptr, p.pre_scale != nullptr, p.pre_shift != nullptr, p.pre_out != nullptr,
        // the partial-sum slot offset of a single-phase launch, in bytes
        p.st_part ? (int64_t)(reinterpret_cast<const char*>(p.st_part) - reinterpret_cast<const char*>(kF16Dummy)) : 0};
    // a refused build leaves the record half configured: only the two return codes are its answer
    const int n_body = rc == MP_OK ? (int)(sizeof(body) / sizeof(body[0])) : 0;
    if (cap < 2 + n_body) return MP_ERR_WORKSPACE;
    out[0] = head[0];
    out[1] = head[1];
    for (int i = 0; i < n_body; ++i) out[2 + i] = body[i];
    return 2 + n_body;
}

int mp_f16_fuse_upsample_sum(const void* base, const void* t1, int s1, const void* t2, int s2, const void* t3, int s3, void* out,
                             int n, int c, int h, int w, int relu, mp_stream_t stream) {
    if (!base || !t1 || !out) return MP_ERR_NULL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) return MP_ERR_SHAPE;
    const int ss[3] = {s1, t2 ? s2 : 1, t3 ? s3 : 1};
    for (int i = 0; i < 3; ++i)
        if (ss[i] < 1 || h % ss[i] || w % ss[i]) return MP_ERR_SHAPE;
    if (t3 && !t2) return MP_ERR_NULL;
    const int planes = n * ((c + 7) / 8);
    const size_t total = (size_t)planes * h * w;
    auto log2_of = [](int v) { int l = 0; while ((1 << l) < v) ++l; return (1 << l) == v ? l : -1; };
    const int l1 = log2_of(ss[0]), l2 = log2_of(ss[1]), l3 = log2_of(ss[2]);
    if (l1 >= 0 && l2 >= 0 && l3 >= 0 && (unsigned long long)total * (unsigned)(h > w ? h : w) < 0x100000000ULL) {
        hipLaunchKernelGGL(fuse_sum_f16_fast_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream),
                           reinterpret_cast<const u32x4*>(base), reinterpret_cast<const u32x4*>(t1), l1, reinterpret_cast<const u32x4*>(t2), l2,
                           reinterpret_cast<const u32x4*>(t3), l3, reinterpret_cast<u32x4*>(out), (unsigned)total, (unsigned)h, (unsigned)w,
                           magic_of((unsigned)h), magic_of((unsigned)w), relu);
        return check_launch();
    }
    hipLaunchKernelGGL(fuse_sum_f16_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const u32x4*>(base), reinterpret_cast<const u32x4*>(t1), s1,
                       reinterpret_cast<const u32x4*>(t2), s2, reinterpret_cast<const u32x4*>(t3), s3,
                       reinterpret_cast<u32x4*>(out), planes, h, w, relu);
    return check_launch();
}

}  // extern "C"
