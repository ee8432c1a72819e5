// Online hard keypoint mining (OHKM) over the joint MSE: per sample only the topk joints with the largest weighted squared error
// contribute.  The selection depends on the step's own heat maps, so it is made on the device and the whole loss stays inside a
// captured training step: three forward launches, one backward launch, no atomics, no read-back.
//
//   S[n,k]   = sum_i ((pred_i - target_i)^2 * w[n,k])              fp32, the arithmetic of mse_row_kernel (pose_ops.hip)
//   sel[n,k] = rank(k) < topk,  rank(k) = #{j : S_j goes before S_k}
//              (a NaN before every number, then the larger value, then the lower joint index: a total order)
//   L        = (float)(sum_n sum_{k selected, ascending} (double)S[n,k] / (N * topk * HW))
//   dL/dpred = g * sel * w * 2 (pred - target) / (N * topk * HW);   rows that are not selected are written as zeros, unread
//
// Launches: ohkm_row_kernel (a workgroup per (n, k) row) -> ohkm_select_kernel (a workgroup per sample: ranks from LDS, writes
// sel and the sample's fp64 sum) -> ohkm_final_kernel (one workgroup: the N sample sums in a fixed order).  The selection needs every
// row sum of its sample and the loss needs every selection, which is what separates the three.
//
// fp contraction is OFF in this file, as in pose_ops.hip: a row sum is the same sequence of roundings as mse_row_kernel's.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace mp {
namespace {

constexpr int kOhkmThreads = 256;   // row, final and backward launches: four waves
constexpr int kOhkmMaxJoints = 1024;  // the select launch keeps a sample's row sums in LDS

__device__ __forceinline__ float ohkm_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One (n, k) row per workgroup.  The per-thread order, the wave butterfly and the four-wave sum are those of mse_row_kernel, so a
// row's sum depends on its hw values and its weight only: two bit-identical rows give bit-identical sums wherever they lie.
// vec: hw % 4 == 0 and 16-byte aligned bases (decided by the host).
__global__ __launch_bounds__(kOhkmThreads) void ohkm_row_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                const float* __restrict__ wgt, float* __restrict__ row_sum, int hw,
                                                                int vec) {
    const int row = blockIdx.x;
    const float wv = wgt ? wgt[row] : 1.f;
    const float* a = pred + (size_t)row * hw;
    const float* b = tgt + (size_t)row * hw;
    float acc = 0.f;
    if (vec) {
        const float4* a4 = reinterpret_cast<const float4*>(a);
        const float4* b4 = reinterpret_cast<const float4*>(b);
        for (int q = threadIdx.x; q < (hw >> 2); q += kOhkmThreads) {
            const float4 x = a4[q], y = b4[q];
            const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
            acc += (d0 * d0) * wv;
            acc += (d1 * d1) * wv;
            acc += (d2 * d2) * wv;
            acc += (d3 * d3) * wv;
        }
    } else {
        for (int i = threadIdx.x; i < hw; i += kOhkmThreads) {
            const float d = a[i] - b[i];
            acc += (d * d) * wv;
        }
    }
    acc = ohkm_wave_sum(acc);
    __shared__ float ws[kOhkmThreads / kWave];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) row_sum[row] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// does joint j (sum sj) go before joint k (sum sk)?  j != k
__device__ __forceinline__ bool ohkm_before(float sj, int j, float sk, int k) {
    const bool nj = sj != sj, nk = sk != sk;
    if (nj || nk) return nj && (!nk || j < k);
    return sj > sk || (sj == sk && j < k);  // -0.0 == +0.0: the index decides
}

// One sample per workgroup (one wave for k <= 64, four beyond).  Every thread ranks its joints against all k sums, read from LDS
// at a wave-uniform address (a broadcast); one lane then adds the selected sums in ascending joint order in fp64.
__global__ __launch_bounds__(kOhkmThreads) void ohkm_select_kernel(const float* __restrict__ row_sum, unsigned char* __restrict__ sel,
                                                                   double* __restrict__ sample_sum, int k, int topk) {
    __shared__ float s_sum[kOhkmMaxJoints];
    __shared__ unsigned char s_sel[kOhkmMaxJoints];
    const int n = blockIdx.x, tid = threadIdx.x, threads = blockDim.x;
    const float* s = row_sum + (size_t)n * k;
    for (int j = tid; j < k; j += threads) s_sum[j] = s[j];
    __syncthreads();
    for (int i = tid; i < k; i += threads) {
        const float si = s_sum[i];
        int rank = 0;
        for (int j = 0; j < k; ++j) rank += (j != i && ohkm_before(s_sum[j], j, si, i)) ? 1 : 0;
        const unsigned char on = rank < topk ? 1 : 0;
        s_sel[i] = on;
        sel[(size_t)n * k + i] = on;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int j = 0; j < k; ++j)
            if (s_sel[j]) acc += (double)s_sum[j];
        sample_sum[n] = acc;
    }
}

// One workgroup: the n sample sums, each thread its strided share in ascending order, then a fixed tree.
__global__ __launch_bounds__(kOhkmThreads) void ohkm_final_kernel(const double* __restrict__ sample_sum, float* __restrict__ loss, int n,
                                                                  double count) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kOhkmThreads) acc += sample_sum[i];
    __shared__ double sm[kOhkmThreads];
    sm[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kOhkmThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(sm[0] / count);
}

// One (n, k) row per workgroup.  A row that is not selected is zero-filled without a load from pred or target (the gradient buffer
// is uninitialised memory, and the row's maps may hold anything).
__global__ __launch_bounds__(kOhkmThreads) void ohkm_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                const float* __restrict__ wgt, const unsigned char* __restrict__ sel,
                                                                const float* __restrict__ gout, float* __restrict__ gpred, int hw,
                                                                float two_over_count, int vec) {
    const int row = blockIdx.x;
    float* o = gpred + (size_t)row * hw;
    if (!sel[row]) {  // uniform over the workgroup
        if (vec) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int q = threadIdx.x; q < (hw >> 2); q += kOhkmThreads) reinterpret_cast<float4*>(o)[q] = z;
        } else {
            for (int i = threadIdx.x; i < hw; i += kOhkmThreads) o[i] = 0.f;
        }
        return;
    }
    const float g = (gout ? gout[0] : 1.f) * two_over_count;
    const float c = wgt ? wgt[row] * g : g;
    const float* a = pred + (size_t)row * hw;
    const float* b = tgt + (size_t)row * hw;
    if (vec) {
        for (int q = threadIdx.x; q < (hw >> 2); q += kOhkmThreads) {
            const float4 x = reinterpret_cast<const float4*>(a)[q], y = reinterpret_cast<const float4*>(b)[q];
            float4 r;
            r.x = (x.x - y.x) * c;
            r.y = (x.y - y.y) * c;
            r.z = (x.z - y.z) * c;
            r.w = (x.w - y.w) * c;
            reinterpret_cast<float4*>(o)[q] = r;
        }
    } else {
        for (int i = threadIdx.x; i < hw; i += kOhkmThreads) o[i] = (a[i] - b[i]) * c;
    }
}

int ohkm_shape(int n, int k, int hw, int topk) {
    if (n <= 0 || k <= 0 || hw <= 0 || topk < 1 || topk > k || k > kOhkmMaxJoints) return MP_ERR_SHAPE;
    if ((long long)n * k > 0x7fffffffLL) return MP_ERR_SHAPE;  // a workgroup per row
    return MP_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_joints_ohkm_workspace_bytes(int n, int k) {
    if (n <= 0 || k <= 0) return 0;
    return ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
}

int mp_joints_ohkm_fwd(const float* pred, const float* target, const float* weight, float* loss, float* row_sum, unsigned char* sel,
                       void* workspace, size_t workspace_bytes, int n, int k, int hw, int topk, mp_stream_t stream) {
    if (!pred || !target || !loss || !row_sum || !sel) return MP_ERR_NULL;
    int rc = ohkm_shape(n, k, hw, topk);
    if (rc != MP_OK) return rc;
    if (!workspace || workspace_bytes < mp_joints_ohkm_workspace_bytes(n, k) || ((uintptr_t)workspace & 7u)) return MP_ERR_WORKSPACE;
    double* sample_sum = reinterpret_cast<double*>(workspace);
    const int vec = (hw & 3) == 0 && aligned16(pred) && aligned16(target);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(ohkm_row_kernel, dim3(n * k), dim3(kOhkmThreads), 0, s, pred, target, weight, row_sum, hw, vec);
    if ((rc = check_launch()) != MP_OK) return rc;
    hipLaunchKernelGGL(ohkm_select_kernel, dim3(n), dim3(k <= kWave ? kWave : kOhkmThreads), 0, s, (const float*)row_sum, sel, sample_sum,
                       k, topk);
    if ((rc = check_launch()) != MP_OK) return rc;
    hipLaunchKernelGGL(ohkm_final_kernel, dim3(1), dim3(kOhkmThreads), 0, s, (const double*)sample_sum, loss, n,
                       (double)n * (double)topk * (double)hw);
    return check_launch();
}

int mp_joints_ohkm_bwd(const float* pred, const float* target, const float* weight, const unsigned char* sel, const float* grad_out,
                       float* grad_pred, int n, int k, int hw, int topk, mp_stream_t stream) {
    if (!pred || !target || !sel || !grad_pred) return MP_ERR_NULL;
    const int rc = ohkm_shape(n, k, hw, topk);
    if (rc != MP_OK) return rc;
    const float c = (float)(2.0 / ((double)n * (double)topk * (double)hw));
    const int vec = (hw & 3) == 0 && aligned16(pred) && aligned16(target) && aligned16(grad_pred);
    hipLaunchKernelGGL(ohkm_bwd_kernel, dim3(n * k), dim3(kOhkmThreads), 0, as_stream(stream), pred, target, weight, sel, grad_out,
                       grad_pred, hw, c, vec);
    return check_launch();
}

}  // extern "C"
