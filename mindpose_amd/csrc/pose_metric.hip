// Training-time pose accuracy (PCK of the output heat maps against the target heat maps) as two launches that fit into a captured
// training step: mp_pose_pck_accuracy reads the maps the step already holds, accumulates in a device state block and is read back
// once per epoch (models/metrics.py).
//
// The metric is the accuracy() of the HRNet training code (lib/core/evaluate.py) restated from knowledge, quirks included: arg-max
// per map with numpy's first-index tie rule, (0, 0) where the maximum is not > 0 (a NaN anywhere makes numpy's max NaN, so also
// then), pairs with a target peak in the first two rows or columns dropped, x divided by H / 10 and y by W / 10.  The hit test is
// the inequality  100 * ((dx W)^2 + (dy H)^2) < thr^2 (H W)^2  in double.  ONE lane evaluates it, from the integer coordinates, in
// this order, so the result cannot depend on how the threads divide a map.  (dx W)^2, (dy H)^2, their sum (below 2^49) and (H W)^2
// are exact integers in double for maps up to 4096 x 4096; the products with 100 and thr^2 are exact too up to 1024 x 1024 at
// thr = 0.5 (below 2^48) and round once each, as IEEE double does anywhere, beyond that.
//
// fp contraction is OFF in this file: the per-step mean and the running sums are compared bit for bit with a float64 restatement.
#include "common.h"
#include "reduce.h"

#include <math.h>

#pragma clang fp contract(off)

namespace mp {
namespace {

constexpr int kPckThreads = 256;         // launch 1: one workgroup of four waves per (n, k) map pair
constexpr int kPckGridCap = 256 * 16;    // launch 1's grid; more pairs than this are walked by a grid-stride loop
constexpr int kPckBatch = 4;             // 16-byte loads per map requested before the first is looked at
constexpr int kPckUpdateThreads = 1024;  // launch 2: sixteen waves, one joint each at a time (17 joints: two dependent rounds of loads)
constexpr int kPckJointChunk = 256;      // launch 2: joints reduced per pass

// per-thread running arg-max; the indices a thread sees ascend, so a strict comparison keeps the first of equal values
struct ArgMax {
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    bool nan = false;
    __device__ __forceinline__ void take(float v, int i) {
        nan |= v != v;
        if (v > best) {
            best = v;
            bidx = i;
        }
    }
    __device__ __forceinline__ void take4(const float4& v, int i) {
        take(v.x, i);
        take(v.y, i + 1);
        take(v.z, i + 2);
        take(v.w, i + 3);
    }
};

// elements in front of the first 16-byte boundary of a 4-byte aligned map (at most 3, at most the map)
__device__ __forceinline__ int head_of(const float* p, int hw) {
    const int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    return head < hw ? head : hw;
}

// One (output, target) map pair per workgroup pass.  Each map is read once: a scalar head up to the first 16-byte boundary, 16-byte
// loads (kPckBatch quads of either map in flight per thread before the first is used), a scalar tail.  flags[pair] = valid | hit << 1.
__global__ __launch_bounds__(kPckThreads) void pose_pck_flags_kernel(const float* __restrict__ output, const float* __restrict__ target,
                                                                      int pairs, int h, int w, double rhs,
                                                                      unsigned char* __restrict__ flags) {
    __shared__ float s_best[2][kPckThreads / kWave];
    __shared__ int s_idx[2][kPckThreads / kWave];
    __shared__ int s_nan[2][kPckThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = h * w;
    for (int pair = blockIdx.x; pair < pairs; pair += gridDim.x) {
        const float* maps[2] = {output + (size_t)pair * hw, target + (size_t)pair * hw};
        ArgMax am[2];
        int head[2], nq[2];
        const float4* body[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            head[m] = head_of(maps[m], hw);
            nq[m] = (hw - head[m]) >> 2;
            body[m] = reinterpret_cast<const float4*>(maps[m] + head[m]);
            if (tid < head[m]) am[m].take(maps[m][tid], tid);
        }
        const int nq_max = nq[0] > nq[1] ? nq[0] : nq[1];
        for (int q0 = tid; q0 < nq_max; q0 += kPckThreads * kPckBatch) {
            // every load is issued (a quad index past the end is clamped to the last quad, whose result is then not looked at): a
            // load under a per-element condition would be branched around and waited for one by one
            float4 v[2][kPckBatch];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                if (nq[m] == 0) continue;  // uniform over the workgroup
#pragma unroll
                for (int j = 0; j < kPckBatch; ++j) {
                    const int q = q0 + kPckThreads * j;
                    v[m][j] = body[m][q < nq[m] ? q : nq[m] - 1];
                }
            }
#pragma unroll
            for (int j = 0; j < kPckBatch; ++j)
#pragma unroll
                for (int m = 0; m < 2; ++m)
                    if (q0 + kPckThreads * j < nq[m]) am[m].take4(v[m][j], head[m] + ((q0 + kPckThreads * j) << 2));
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int i = head[m] + (nq[m] << 2) + tid;  // at most 3 elements behind the last quad
            if (i < hw) am[m].take(maps[m][i], i);
        }
        // four waves -> one result per map
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float best = am[m].best;
            int bidx = am[m].bidx;
            wave_argmax(best, bidx);
            const int any_nan = __any(am[m].nan ? 1 : 0);
            if (lane == 0) {
                s_best[m][wave] = best;
                s_idx[m][wave] = bidx;
                s_nan[m][wave] = any_nan;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int x[2], y[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                float best = s_best[m][0];
                int bidx = s_idx[m][0], nan = s_nan[m][0];
#pragma unroll
                for (int wv = 1; wv < kPckThreads / kWave; ++wv) {
                    argmax_combine(best, bidx, s_best[m][wv], s_idx[m][wv]);
                    nan |= s_nan[m][wv];
                }
                const bool peak = nan == 0 && best > 0.f;  // numpy: max(...) > 0 is False for a NaN maximum
                y[m] = peak ? bidx / w : 0;
                x[m] = peak ? bidx - y[m] * w : 0;
            }
            const bool valid = x[1] > 1 && y[1] > 1;
            const double a = (double)(x[0] - x[1]) * (double)w, b = (double)(y[0] - y[1]) * (double)h;
            const bool hit = valid && 100.0 * (a * a + b * b) < rhs;
            flags[pair] = (unsigned char)((valid ? 1 : 0) | (hit ? 2 : 0));
        }
        __syncthreads();  // the LDS slots are rewritten by the next pair
    }
}

struct PckState {  // mp_pose_pck_state followed by hits[K], valid[K]
    long long steps, sum_cnt;
    double sum_acc_cnt, last_avg_acc;
    long long last_cnt, pad;
};

// A single workgroup: per-joint integer sums of the flags over n, then ONE lane forms acc_k, avg_acc and cnt in double (joint
// order) and advances the state block.
__global__ __launch_bounds__(kPckUpdateThreads) void pose_pck_update_kernel(const unsigned char* __restrict__ flags, int n, int k,
                                                                       PckState* __restrict__ st) {
    __shared__ int s_hits[kPckJointChunk], s_valid[kPckJointChunk];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long* hits = reinterpret_cast<long long*>(st + 1);
    long long* valid = hits + k;
    double sum = 0.0;   // thread 0 only
    long long cnt = 0;  // thread 0 only
    for (int k0 = 0; k0 < k; k0 += kPckJointChunk) {
        const int kc = k - k0 < kPckJointChunk ? k - k0 : kPckJointChunk;
        for (int j = wave; j < kc; j += kPckUpdateThreads / kWave) {
            int hsum = 0, vsum = 0;
            for (int i = lane; i < n; i += 64) {
                const int f = flags[(size_t)i * k + k0 + j];
                vsum += f & 1;
                hsum += (f >> 1) & 1;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {  // the two int sums advance together
                hsum += __shfl_xor(hsum, off, 64);
                vsum += __shfl_xor(vsum, off, 64);
            }
            if (lane == 0) {
                s_hits[j] = hsum;
                s_valid[j] = vsum;
            }
        }
        __syncthreads();
        if (tid < kc) {
            hits[k0 + tid] += s_hits[tid];
            valid[k0 + tid] += s_valid[tid];
        }
        if (tid == 0) {
            for (int j = 0; j < kc; ++j) {
                if (s_valid[j] > 0) {
                    sum += (double)s_hits[j] / (double)s_valid[j];
                    cnt += 1;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double avg = cnt > 0 ? sum / (double)cnt : 0.0;
        st->steps += 1;
        st->sum_cnt += cnt;
        st->sum_acc_cnt += avg * (double)cnt;
        st->last_avg_acc = avg;
        st->last_cnt = cnt;
    }
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

int mp_pose_pck_accuracy(const float* output, const float* target, int N, int K, int H, int W, double thr, unsigned char* flags,
                         void* state, mp_stream_t stream) {
    if (!output || !target || !flags || !state) return MP_ERR_NULL;
    if (N < 1 || K < 1 || H < 1 || W < 1 || !(thr > 0.0) || !(thr < INFINITY)) return MP_ERR_SHAPE;
    if (H > 4096 || W > 4096) return MP_ERR_UNSUPPORTED;  // beyond that (dx W)^2 + (dy H)^2 and (H W)^2 are no longer exact integers in double
    if ((long long)N * K > 0x7fffffffLL) return MP_ERR_SHAPE;
    if (((uintptr_t)output & 3u) || ((uintptr_t)target & 3u) || ((uintptr_t)state & 7u)) return MP_ERR_UNSUPPORTED;
    static_assert(sizeof(PckState) == sizeof(mp_pose_pck_state), "state block header");
    const int pairs = N * K;
    const double hw = (double)H * (double)W;
    const double rhs = thr * thr * (hw * hw);
    const int grid = pairs < kPckGridCap ? pairs : kPckGridCap;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(pose_pck_flags_kernel, dim3(grid), dim3(kPckThreads), 0, s, output, target, pairs, H, W, rhs, flags);
    int rc = check_launch();
    if (rc != MP_OK) return rc;
    hipLaunchKernelGGL(pose_pck_update_kernel, dim3(1), dim3(kPckUpdateThreads), 0, s, (const unsigned char*)flags, N, K,
                       reinterpret_cast<PckState*>(state));
    return check_launch();
}

}  // extern "C"
