// Shared helpers of libmindpose_hip.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <initializer_list>

#include "../../include/mindpose_hip.h"

namespace mp {

extern thread_local int g_last_hip_error;
// set around a dispatch by the "would this launch be accepted" queries: the leaf launch functions return MP_OK without launching
extern thread_local bool g_dry_launch;

inline int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return MP_ERR_HIP;
    }
    return MP_OK;
}

inline hipStream_t as_stream(mp_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kWave = 64;

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: one of these per kernel instantiation
// (function-local static) remembers on which devices it has been raised, so a process that drives a second device sets it
// there too; fetch_or makes concurrent first launches from several host threads harmless (both set it, once each at worst).
struct AttrOnce {
    unsigned long long mask = 0;
    bool need() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return true;
        const unsigned long long bit = 1ull << (dev & 63);
        return (__atomic_fetch_or(&mask, bit, __ATOMIC_RELAXED) & bit) == 0;
    }
};

// Launch of a kernel that takes dynamic LDS: raises the kernel's limit to the 160 KB of a gfx950 workgroup on its first launch on
// each device (the error of a refused raise is dropped: the launch itself reports what it cannot have), launches, and returns
// check_launch().  One launcher per kernel instantiation - the kernel is the TEMPLATE argument: the dynamic-LDS attribute is a
// property of the instantiation, so the once-per-device flag must be too (a flag shared through the common function-pointer type,
// as a static in a generic lambda or in a function that takes the kernel as a value would be, reaches only the first kernel a
// process launches through it).
template <auto Kern, typename... Args>
int launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args&... args) {
    static AttrOnce once;
    if (once.need()) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipGetLastError();
    }
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, s, args...);
    return check_launch();
}

// XCD-aware workgroup id.  Workgroups are dealt round-robin over the 8 XCDs (blocks b, b+8, ... share an XCD and its L2): this maps
// block b of nb to the id it takes when every XCD walks one contiguous run of ids instead, so neighbouring ids share an L2.
__device__ __forceinline__ int xcd_contiguous(int b, int nb) {
    const int q8 = nb >> 3, r8 = nb & 7, xcd = b & 7, j = b >> 3;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + j;
}

// Raw buffer access: the hardware range check makes invalid lanes free - an offset >= num_records loads 0 /
// drops the store - so masked staging and epilogue traffic needs no branches (and no s_waitcnt between loads).
constexpr unsigned kOob = 0x80000000u;  // every descriptor spans < 2 GiB
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, size_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(bytes < 0x7FFFFFF0u ? bytes : 0x7FFFFFF0u), 0x00020000);
}

// Division by a launch-constant d: magic = magic_of(d) = floor(2^32 / d) + 1; exact while e * d < 2^32
inline unsigned magic_of(unsigned d) { return d <= 1 ? 0u : (unsigned)(0x100000000ULL / d) + 1u; }
__device__ __forceinline__ unsigned fastdiv(unsigned e, unsigned d, unsigned magic) { return d == 1 ? e : __umulhi(e, magic); }

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Experiment knobs (MP_* environment variables: tile counts, forced forms - used by tests/ and tools/ to reach code paths small
// problems would not take).  A production process never looks at them: whether they are honoured at all is decided ONCE per
// process by MINDPOSE_EXPERIMENT_KNOBS=1 (tests/conftest.py and the tools set it), so the configure functions - called per conv
// launch by the eager training path - cost no getenv() unless that switch is on.
inline bool knobs_on() {
    static const bool on = [] {
        const char* e = getenv("MINDPOSE_EXPERIMENT_KNOBS");
        return e != nullptr && atoi(e) != 0;
    }();
    return on;
}
inline const char* knob(const char* name) { return knobs_on() ? getenv(name) : nullptr; }

// A launch plan (conv_api.hip) holds one launch record per entry.  Every record type comes with two functions beside its
// declaration: run(record, stream) launches it, describe(record, info) writes the twelve values mp_plan_entry_info reports -
// info[0] is the record's kind below.  The numbers are ABI (tools and tests read them); the fp32 conv kernels all report kConv.
enum PlanKind { kConv = 0, kMaxPool = 1, kFuseSum = 2, kConvF16 = 3, kFuseSumF16 = 4, kToC8 = 5, kFromC8 = 6, kBarrier = 7, kBlockF16 = 8,
                kWinograd = 9, kPwChainF16 = 10, kStemF16 = 11, kStemF32 = 12, kPwChainF32 = 13, kConcat = 14, kColSlice = 15 };

// info[] of an entry: the given values in order, zeros behind them
inline void fill_info(int64_t info[12], std::initializer_list<int64_t> values) {
    int i = 0;
    for (int64_t v : values) info[i++] = v;
    for (; i < 12; ++i) info[i] = 0;
}

}  // namespace mp
