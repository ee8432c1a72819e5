// The joint MSE (JointsMSELoss, mse.py:36-44) and the joint MSE with online hard keypoint mining (OHKM: per sample only the topk joints
// with the largest weighted squared error contribute; the reference has no counterpart) on one row pass and one backward pass.
//
//   S[n,k]   = sum_i ((pred_i - target_i)^2 * w[n,k])              fp32, joints_sq_row_kernel, a workgroup per (n, k) row
//   MSE:  L  = (float)(sum_rows (double)S * (1 / (N K HW)))        joints_mse_final_kernel, one workgroup, fixed order
//   OHKM: sel[n,k] = rank(k) < topk,  rank(k) = #{j : S_j goes before S_k}                         ohkm_select_kernel, a workgroup per sample
//              (a NaN before every number, then the larger value, then the lower joint index: a total order)
//         L  = (float)(sum_n sum_{k selected, ascending} (double)S[n,k] / (N * topk * HW))          ohkm_final_kernel, one workgroup
//   dL/dpred = g * sel * w * 2 (pred - target) / (N * (K | topk) * HW)   joints_bwd_kernel; sel absent = 1; rows that are not selected
//              are written as zeros, unread
// The OHKM selection depends on the step's own heat maps, so it is made on the device and the loss stays inside a captured training
// step: no atomics, no read-back.  The selection needs every row sum of its sample and the loss every selection: three launches.
//
// Both losses launch the SAME row kernel under the SAME host predicate (vec16): OHKM's row sums are the MSE's row partials bit for bit,
// for any bases.  fp contraction is OFF in this file: the sums are compared bit for bit with fp32 restatements.
#include "common.h"
#include "reduce.h"

#include <math.h>

#pragma clang fp contract(off)

namespace mp {
namespace {

constexpr int kLossThreads = 256;     // row, final and backward launches: four waves
constexpr int kOhkmMaxJoints = 1024;  // the select launch keeps a sample's row sums in LDS

// One (n, k) row per workgroup: w * d^2 accumulated per element in the thread's own ascending order, the wave butterfly, the
// four-wave sum.  A row's sum depends on its hw values and its weight only: two bit-identical rows give bit-identical sums wherever
// they lie.  vec: the 16-byte path (vec16 below, decided by the host).
__global__ __launch_bounds__(kLossThreads) void joints_sq_row_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
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
        for (int q = threadIdx.x; q < (hw >> 2); q += kLossThreads) {
            const float4 x = a4[q], y = b4[q];
            const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
            acc += (d0 * d0) * wv;
            acc += (d1 * d1) * wv;
            acc += (d2 * d2) * wv;
            acc += (d3 * d3) * wv;
        }
    } else {
        for (int i = threadIdx.x; i < hw; i += kLossThreads) {
            const float d = a[i] - b[i];
            acc += (d * d) * wv;
        }
    }
    __shared__ float ws[kLossThreads / kWave];
    acc = block_sum_lane0(wave_sum(acc), ws);
    if (threadIdx.x == 0) row_sum[row] = acc;
}

// One workgroup: the row partials in fp64, each thread its strided share in ascending order, then a fixed tree.
__global__ __launch_bounds__(kLossThreads) void joints_mse_final_kernel(const float* __restrict__ partial, float* __restrict__ loss, int rows,
                                                                        double inv_count) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < rows; i += blockDim.x) acc += (double)partial[i];
    __shared__ double sm[kLossThreads];
    block_tree_sum_256(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(sm[0] * inv_count);
}

// does joint j (sum sj) go before joint k (sum sk)?  j != k
__device__ __forceinline__ bool ohkm_before(float sj, int j, float sk, int k) {
    const bool nj = sj != sj, nk = sk != sk;
    if (nj || nk) return nj && (!nk || j < k);
    return sj > sk || (sj == sk && j < k);  // -0.0 == +0.0: the index decides
}

// One sample per workgroup (one wave for k <= 64, four beyond).  Every thread ranks its joints against all k sums, read from LDS
// at a wave-uniform address (a broadcast); one lane then adds the selected sums in ascending joint order in fp64.
__global__ __launch_bounds__(kLossThreads) void ohkm_select_kernel(const float* __restrict__ row_sum, unsigned char* __restrict__ sel,
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

// One workgroup: the n sample sums likewise.  A division where the MSE multiplies by a reciprocal: the two round differently.
__global__ __launch_bounds__(kLossThreads) void ohkm_final_kernel(const double* __restrict__ sample_sum, float* __restrict__ loss, int n,
                                                                  double count) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kLossThreads) acc += sample_sum[i];
    __shared__ double sm[kLossThreads];
    block_tree_sum_256(acc, sm);
    if (threadIdx.x == 0) loss[0] = (float)(sm[0] / count);
}

// One (n, k) row per workgroup.  sel == NULL: every row (the plain MSE).  A row that is not selected is zero-filled without a load
// from pred or target (the gradient buffer is uninitialised memory, and the row's maps may hold anything).
__global__ __launch_bounds__(kLossThreads) void joints_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                  const float* __restrict__ wgt, const unsigned char* __restrict__ sel,
                                                                  const float* __restrict__ gout, float* __restrict__ gpred, int hw,
                                                                  float two_over_count, int vec) {
    const int row = blockIdx.x;
    float* o = gpred + (size_t)row * hw;
    if (sel && !sel[row]) {  // uniform over the workgroup
        if (vec) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int q = threadIdx.x; q < (hw >> 2); q += kLossThreads) reinterpret_cast<float4*>(o)[q] = z;
        } else {
            for (int i = threadIdx.x; i < hw; i += kLossThreads) o[i] = 0.f;
        }
        return;
    }
    const float g = (gout ? gout[0] : 1.f) * two_over_count;
    const float c = wgt ? wgt[row] * g : g;
    const float* a = pred + (size_t)row * hw;
    const float* b = tgt + (size_t)row * hw;
    if (vec) {
        for (int q = threadIdx.x; q < (hw >> 2); q += kLossThreads) {
            const float4 x = reinterpret_cast<const float4*>(a)[q], y = reinterpret_cast<const float4*>(b)[q];
            float4 r;
            r.x = (x.x - y.x) * c;
            r.y = (x.y - y.y) * c;
            r.z = (x.z - y.z) * c;
            r.w = (x.w - y.w) * c;
            reinterpret_cast<float4*>(o)[q] = r;
        }
    } else {
        for (int i = threadIdx.x; i < hw; i += kLossThreads) o[i] = (a[i] - b[i]) * c;
    }
}

// The 16-byte path of a launch: whole float4s per row, and every base the launch touches on a 16-byte boundary (rows are hw floats
// apart, so aligned bases make every row aligned).  grad is NULL for a forward launch.
int vec16(int hw, const float* pred, const float* target, const float* grad) {
    return (hw & 3) == 0 && (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)grad) & 15u) == 0;
}

int launch_rows(const float* pred, const float* target, const float* weight, float* row_sum, int rows, int hw, hipStream_t s) {
    hipLaunchKernelGGL(joints_sq_row_kernel, dim3(rows), dim3(kLossThreads), 0, s, pred, target, weight, row_sum, hw,
                       vec16(hw, pred, target, nullptr));
    return check_launch();
}

int launch_bwd(const float* pred, const float* target, const float* weight, const unsigned char* sel, const float* grad_out,
               float* grad_pred, int rows, int hw, double count, hipStream_t s) {
    hipLaunchKernelGGL(joints_bwd_kernel, dim3(rows), dim3(kLossThreads), 0, s, pred, target, weight, sel, grad_out, grad_pred, hw,
                       (float)(2.0 / count), vec16(hw, pred, target, grad_pred));
    return check_launch();
}

int ohkm_shape(int n, int k, int hw, int topk) {
    if (n <= 0 || k <= 0 || hw <= 0 || topk < 1 || topk > k || k > kOhkmMaxJoints) return MP_ERR_SHAPE;
    if ((long long)n * k > 0x7fffffffLL) return MP_ERR_SHAPE;  // a workgroup per row
    return MP_OK;
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

size_t mp_joints_mse_workspace_bytes(int n, int k) {
    if (n <= 0 || k <= 0) return 0;
    return ((size_t)n * k * sizeof(float) + 255) & ~(size_t)255;
}

int mp_joints_mse_fwd(const float* pred, const float* target, const float* weight, float* loss, void* workspace,
                      size_t workspace_bytes, int n, int k, int hw, mp_stream_t stream) {
    if (!pred || !target || !loss) return MP_ERR_NULL;
    if (n <= 0 || k <= 0 || hw <= 0) return MP_ERR_SHAPE;
    if (!workspace || workspace_bytes < mp_joints_mse_workspace_bytes(n, k)) return MP_ERR_WORKSPACE;
    float* partial = reinterpret_cast<float*>(workspace);
    const int rows = n * k;
    hipStream_t s = as_stream(stream);
    int rc = launch_rows(pred, target, weight, partial, rows, hw, s);
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(joints_mse_final_kernel, dim3(1), dim3(kLossThreads), 0, s, (const float*)partial, loss, rows,
                       1.0 / ((double)rows * (double)hw));
    return check_launch();
}

int mp_joints_mse_bwd(const float* pred, const float* target, const float* weight, const float* grad_out,
                      float* grad_pred, int n, int k, int hw, mp_stream_t stream) {
    if (!pred || !target || !grad_pred) return MP_ERR_NULL;
    if (n <= 0 || k <= 0 || hw <= 0) return MP_ERR_SHAPE;
    return launch_bwd(pred, target, weight, nullptr, grad_out, grad_pred, n * k, hw, (double)n * k * (double)hw, as_stream(stream));
}

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
    hipStream_t s = as_stream(stream);
    if ((rc = launch_rows(pred, target, weight, row_sum, n * k, hw, s)) != MP_OK) return rc;
    hipLaunchKernelGGL(ohkm_select_kernel, dim3(n), dim3(k <= kWave ? kWave : kLossThreads), 0, s, (const float*)row_sum, sel, sample_sum,
                       k, topk);
    if ((rc = check_launch()) != MP_OK) return rc;
    hipLaunchKernelGGL(ohkm_final_kernel, dim3(1), dim3(kLossThreads), 0, s, (const double*)sample_sum, loss, n,
                       (double)n * (double)topk * (double)hw);
    return check_launch();
}

int mp_joints_ohkm_bwd(const float* pred, const float* target, const float* weight, const unsigned char* sel, const float* grad_out,
                       float* grad_pred, int n, int k, int hw, int topk, mp_stream_t stream) {
    if (!pred || !target || !sel || !grad_pred) return MP_ERR_NULL;
    const int rc = ohkm_shape(n, k, hw, topk);
    if (rc != MP_OK) return rc;
    return launch_bwd(pred, target, weight, sel, grad_out, grad_pred, n * k, hw, (double)n * (double)topk * (double)hw,
                      as_stream(stream));
}

}  // extern "C"
