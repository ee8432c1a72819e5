// Streaming 1x1 fp32 convolution (conv_pw_f32.hip): launch record shared with the conv API / plan replay (conv_api.hip).
#pragma once
#include "common.h"

namespace mp {

struct PwParams {
    const float* x;
    const float* wp;  // the direct kernel's packing of a 1x1 weight: [Cin/4][4][Cout_pad16]
    const float* scale;
    const float* shift;
    const float* res1;
    float* out;
    int N, Cin, Cout, Cout_pad16, HW;
    int tiles, tiles_per_wg;  // 64-pixel tiles in all / per persistent workgroup
    int relu;
};

struct PwLaunch {
    PwParams p;
    int kq, cbw;  // Cin / 4, cout blocks per wave: the instantiation
    int grid;
    size_t lds_bytes;
};

int pw_configure(const mp_conv_desc* d, PwLaunch& L);  // MP_OK / MP_ERR_UNSUPPORTED; pointers left null
int pw_launch(const PwLaunch& L, hipStream_t s);

constexpr int kPointwise = 8;  // forced-variant index of this kernel (behind the direct kernel's tile variants; never the library's own choice)

inline int run(const PwLaunch& L, hipStream_t s) { return pw_launch(L, s); }
inline void describe(const PwLaunch& L, int64_t info[12]) {
    fill_info(info, {kConv, 1, 1, kPointwise, L.grid, (int64_t)L.lds_bytes, L.p.Cout, 64, 64, L.cbw, L.p.tiles_per_wg, L.kq});
}

}  // namespace mp
