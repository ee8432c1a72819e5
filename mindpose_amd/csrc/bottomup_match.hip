// Associative-embedding grouping on gfx950: match_by_tag (mindpose/utils/match.py:15-116 of the reference) for a batch of images in
// ONE launch, bit-equal to the host function of utils/match.py, which calls scipy.optimize.linear_sum_assignment once per joint.
//
//   bu_match_kernel<L>  one workgroup of ONE wave64 per image.  The joint loop and the rows of an assignment are serial by nature;
//                       the parallel axis is the columns (the person groups): the distance row, the scan for the minimum and the key
//                       lookup run with the columns strided over the 64 lanes and wave-level reductions (shuffles).  All solver
//                       state lives in LDS, per column; no cost matrix is stored - cost(i, j) is recomputed from the row's tag and
//                       the group's mean tag (L <= 4 subtractions and a square root).  Lanes synchronise by program order alone
//                       (one wave): wave_sync() is a compiler fence, not an s_barrier.  No atomics.
//
// With rounded costs the matrix is full of ties and another optimum is another answer, so the kernel restates scipy's solver, tie
// order included, and numpy's float32 reductions (tests/match_restated.py is the same specification in Python, held to scipy and
// numpy by tests/test_match_restated_cpu.py):
//   (a) rectangular LSAP by shortest augmenting paths in double, nr = n_new <= nc = max(n_new, n_groups) (never transposed); dummy
//       columns cost float32(1e10).  Per row: remaining[it] = nc - 1 - it; every scan evaluates, for it < num_remaining and
//       j = remaining[it], r = ((minVal + cost[i][j]) - u[i]) - v[j] and keeps the smaller of r and shortest[j] (path[j] = i); the
//       next column is, among the scan positions of minimum shortest, the LARGEST position whose column is unassigned, else the
//       SMALLEST position - the closed form of scipy's sequential `s < lowest || (s == lowest && row4col[j] == -1)`, which reduces
//       across lanes; the chosen position is removed by the swap remaining[it] = remaining[--num_remaining] (kept: it fixes later
//       scan positions).  Then u[cur] += minVal, u[i] += minVal - shortest[col4row[i]] for the other visited rows,
//       v[j] -= minVal - shortest[j] for the visited columns, and the augmentation along path from the sink.
//   (b) group mean = np.mean(np.stack(tags), axis=0) on float32 [n, L]: L >= 2 a sequential sum in list order; L == 1 numpy's pairwise
//       sum (n < 8 sequential from 0; else eight accumulators over whole blocks of eight, ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), the
//       tail added in order); then one float32 division by n.  n <= k <= 64: the n >= 128 recursion never occurs.
//   (c) value > vis_thr and dist < tag_thr are float32 comparisons (numpy 2: Python floats are weak scalars).
//   (d) dist = float32 sqrt(sum_l d_l * d_l), summed in l order, correctly rounded sqrt (no fast-math in this build); np.round =
//       rintf; the threshold test reads the unrounded dist.
//   (e) the dict: key = tags[r, 0] compared as a float (-0.0 == 0.0); an existing key KEEPS the person's other joints, overwrites this
//       joint's row and RESETS the tag list to [tag]; the candidate groups and their means are frozen at the start of a step.
//
// Memory ordering inside the wave.  LDS: one wave's DS instructions execute in order.  Global memory: every address of people and of
// the tag lists is written by the SAME lane each time it is written (element e of a person block by lane e % 64, tag l by lane l), so
// stores to one address keep program order; the tag lists are read by other lanes only in a later step, behind the step's
// workgroup-scope fence.  fp contraction is OFF, as in bottomup_ops.hip.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace mp {

// the decoder's limits (bottomup_ops.hip: kBuMaxM, kBuMaxTags) and the joints a by-value order carries
constexpr int kBuMaxM = 64;
constexpr int kBuMaxTags = 4;
constexpr int kBuMatchMaxJoints = 64;
constexpr int kBuMatchMaxGroups = 1024;  // k * m: every detection opens at most one group; the per-column LDS state is sized by it

struct BuMatchParams {
    const float* val;  // [N, K, M]
    const float* tag;  // [N, K, M, L]
    const float* ind;  // [N, K, M, 2]
    int k, m;
    float vis_thr, tag_thr;
    int ignore_too_much, rounded;
    float* people;     // [N, K * M, K, 3 + L]
    int* counts;       // [N]
    int* status;       // [N]
    float* lists;      // [N, K (slot), K * M (group), L]: slot-major, so that the lanes of a mean pass read neighbouring groups
    unsigned char order[kBuMatchMaxJoints];
};

// Orders the LDS / global accesses of the wave's lanes around it.  The workgroup is one wave: no s_barrier is needed or emitted.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ double uniform(double v) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ double wave_min(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, kWave);
        v = o < v ? o : v;
    }
    return uniform(v);
}

__device__ __forceinline__ int wave_max(int v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
    return uniform(v);
}

template <int L>
struct BuMatchState {
    double shortest[kBuMatchMaxGroups];
    double v[kBuMatchMaxGroups];
    double u[kBuMaxM];
    float mean[kBuMatchMaxGroups][L];
    float key[kBuMatchMaxGroups];
    float row_tag[kBuMaxM][L];
    short path[kBuMatchMaxGroups];
    short row4col[kBuMatchMaxGroups];
    short remaining[kBuMatchMaxGroups];
    short col4row[kBuMaxM];
    short row_det[kBuMaxM];  // row r of the step = detection row_det[r] of the joint
    unsigned char in_sc[kBuMatchMaxGroups];
    unsigned char count[kBuMatchMaxGroups];  // tags in the group's list
    unsigned char dirty[kBuMatchMaxGroups];  // the list changed since mean[] was computed
    unsigned char in_sr[kBuMaxM];
};

// float32 distance between row r's tag and the frozen mean of group c
template <int L>
__device__ __forceinline__ float tag_distance(const BuMatchState<L>& s, const float* t, int c) {
    float d = t[0] - s.mean[c][0];
    float sum = d * d;
#pragma unroll
    for (int l = 1; l < L; ++l) {
        d = t[l] - s.mean[c][l];
        sum = sum + d * d;
    }
    return sqrtf(sum);
}

// np.mean over the n listed tags of group c (rule (b)); a[i] is slot i of component l
template <int L>
__device__ __forceinline__ void group_mean(BuMatchState<L>& s, const float* lists, int groups, int c, int n) {
    const float* a = lists + (size_t)c * L;
    const size_t slot = (size_t)groups * L;
    if (L == 1 && n >= 8) {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j * slot];
        int i = 8;
        for (; i + 8 <= n; i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + a[(i + j) * slot];
        }
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res = res + a[i * slot];
        s.mean[c][0] = res / (float)n;
        return;
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
        float sum = L == 1 ? 0.0f + a[l] : a[l];
        for (int i = 1; i < n; ++i) sum = sum + a[i * slot + l];
        s.mean[c][l] = sum / (float)n;
    }
}

template <int L>
__global__ __launch_bounds__(kWave) void bu_match_kernel(BuMatchParams p) {
    __shared__ BuMatchState<L> s;
    constexpr int W = 3 + L;
    const int img = blockIdx.x, lane = threadIdx.x;
    const int K = p.k, M = p.m, groups = K * M;
    const float* __restrict__ val = p.val + (size_t)img * K * M;
    const float* __restrict__ tag = p.tag + (size_t)img * K * M * L;
    const float* __restrict__ ind = p.ind + (size_t)img * K * M * 2;
    float* people = p.people + (size_t)img * groups * K * W;
    float* lists = p.lists + (size_t)img * K * groups * L;

    // a NaN or infinite tag on a visible detection: scipy raises on such a matrix - the host function decides for this image
    bool bad = false;
    for (int i = lane; i < K * M; i += kWave) {
        if (val[i] > p.vis_thr) {
#pragma unroll
            for (int l = 0; l < L; ++l) bad |= !__builtin_isfinite(tag[(size_t)i * L + l]);
        }
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0) {
            p.counts[img] = 0;
            p.status[img] = 1;
        }
        return;
    }

    int num_groups = 0;  // wave-uniform, as every value that steers the control flow below

    // (e) row r of the step opens the group of its key, or takes over the group that holds the key; returns the new group count
    auto open_group = [&](int joint, int r, int open) -> int {
        const int det = uniform((int)s.row_det[r]);
        const float key = s.row_tag[r][0];
        int hit = -1;
        for (int c = lane; c < open; c += kWave)
            if (s.key[c] == key) hit = c;
        const int found = wave_max(hit);  // keys are distinct: at most one lane holds a hit
        const int c = found < 0 ? open : found;
        if (c >= groups) return open;  // (unreachable: every detection opens at most one group - but never write past the capacity)
        const size_t src = (size_t)joint * M + det;
        float* block = people + (size_t)c * K * W;
        if (c == open) {  // the whole [K, 3 + L] block: zeros, and the row at this joint (element e always by lane e % 64)
            for (int e = lane; e < K * W; e += kWave) {
                const int jj = e / W, x = e - jj * W;
                float value = 0.0f;
                if (jj == joint) value = x < 2 ? ind[src * 2 + x] : x == 2 ? val[src] : s.row_tag[r][x - 3];
                block[e] = value;
            }
        } else {
            const int x = (lane - joint * W) & (kWave - 1);  // the lane e % 64 of element e = joint * W + x
            if (x < W) block[joint * W + x] = x < 2 ? ind[src * 2 + x] : x == 2 ? val[src] : s.row_tag[r][x - 3];
        }
        if (lane < L) lists[(size_t)c * L + lane] = s.row_tag[r][lane];  // slot 0: the list is [tag]
        if (lane == 0) {
            s.key[c] = key;
            s.count[c] = 1;
            s.dirty[c] = 1;
        }
        wave_sync();
        return c == open ? open + 1 : open;
    };

    for (int step = 0; step < K; ++step) {
        const int joint = p.order[step];
        const bool visible = lane < M && val[joint * M + lane] > p.vis_thr;
        const unsigned long long vis_mask = __ballot(visible);
        const int n_new = __popcll(vis_mask);
        if (n_new == 0) continue;
        wave_sync();  // the previous step's readers of row_tag / row_det are done, its list stores are visible
        if (visible) {
            const int r = __popcll(vis_mask & ((1ull << lane) - 1ull));
            s.row_det[r] = (short)lane;
#pragma unroll
            for (int l = 0; l < L; ++l) s.row_tag[r][l] = tag[((size_t)joint * M + lane) * L + l];
        }
        wave_sync();

        if (step == 0 || num_groups == 0) {
            for (int r = 0; r < n_new; ++r) num_groups = open_group(joint, r, num_groups);
            continue;
        }

        const int n_groups = num_groups;  // frozen: groups opened in this step are no candidates
        if (p.ignore_too_much && n_groups == M) continue;
        for (int c = lane; c < n_groups; c += kWave) {
            if (s.dirty[c]) {
                group_mean<L>(s, lists, groups, c, (int)s.count[c]);
                s.dirty[c] = 0;
            }
        }

        // ---- (a) the assignment of the n_new rows to nc columns
        const int nr = n_new, nc = max(n_new, n_groups);
        for (int j = lane; j < nc; j += kWave) {
            s.v[j] = 0.0;
            s.row4col[j] = -1;
        }
        if (lane < nr) {
            s.u[lane] = 0.0;
            s.col4row[lane] = -1;
        }
        for (int cur = 0; cur < nr; ++cur) {
            for (int j = lane; j < nc; j += kWave) {
                s.shortest[j] = INFINITY;
                s.in_sc[j] = 0;
                s.remaining[j] = (short)(nc - 1 - j);
            }
            if (lane < nr) s.in_sr[lane] = 0;
            wave_sync();
            double min_val = 0.0;
            int i = cur, num_remaining = nc, sink = -1;
            while (sink < 0) {
                if (lane == 0) s.in_sr[i] = 1;
                const double ui = s.u[i];
                float t[L];
#pragma unroll
                for (int l = 0; l < L; ++l) t[l] = s.row_tag[i][l];
                double lane_min = INFINITY;
                int lane_code = -1;
                for (int it = lane; it < num_remaining; it += kWave) {
                    const int j = s.remaining[it];
                    double cost = 1e10;  // float32(1e10) exactly
                    if (j < n_groups) {
                        const float d = tag_distance<L>(s, t, j);
                        bad |= !__builtin_isfinite(d);
                        cost = (double)(p.rounded ? rintf(d) : d);
                    }
                    const double r = ((min_val + cost) - ui) - s.v[j];
                    double sp = s.shortest[j];
                    if (r < sp) {
                        s.path[j] = (short)i;
                        s.shortest[j] = r;
                        sp = r;
                    }
                    // unassigned columns above every assigned one and by ascending position, assigned ones by descending position
                    const int code = s.row4col[j] < 0 ? (0x40000000 | it) : (0x3fffffff - it);
                    if (sp < lane_min) {
                        lane_min = sp;
                        lane_code = code;
                    } else if (sp == lane_min) {
                        lane_code = max(lane_code, code);
                    }
                }
                const double lowest = wave_min(lane_min);
                const int code = wave_max(lane_min == lowest ? lane_code : -1);
                // an overflowed distance (finite tags too far apart for float32): not a matrix this kernel restates.  The image is
                // handed over with counts = 0; the person blocks its earlier steps wrote stay behind, for the caller to ignore
                // (code < 0: no column with a finite path cost - cannot happen with finite costs, and must not index anything)
                if (__ballot(bad) != 0ull || code < 0) {
                    if (lane == 0) {
                        p.counts[img] = 0;
                        p.status[img] = 2;
                    }
                    return;
                }
                const int index = (code & 0x40000000) ? (code & 0x3fffffff) : (0x3fffffff - code);
                min_val = lowest;
                const int j = uniform((int)s.remaining[index]);
                const int row = uniform((int)s.row4col[j]);
                --num_remaining;
                const short last = s.remaining[num_remaining];
                if (lane == 0) {
                    s.in_sc[j] = 1;
                    s.remaining[index] = last;
                }
                if (row < 0) sink = j;
                else i = row;
                wave_sync();
            }
            if (lane < nr && s.in_sr[lane]) {
                if (lane == cur) s.u[lane] += min_val;
                else s.u[lane] += min_val - s.shortest[s.col4row[lane]];  // (a visited row other than cur is assigned)
            }
            for (int j = lane; j < nc; j += kWave)
                if (s.in_sc[j]) s.v[j] -= min_val - s.shortest[j];
            wave_sync();
            for (int j = sink, hops = 0; j >= 0 && hops <= nr; ++hops) {  // augment: serial, the same on every lane; <= nr hops
                const int row = uniform((int)s.path[j]);
                const int next = uniform((int)s.col4row[row]);
                if (lane == 0) {
                    s.row4col[j] = (short)row;
                    s.col4row[row] = (short)j;
                }
                j = next;
                if (row == cur) break;
            }
            wave_sync();
        }

        // ---- the pairs in row order: join the matched group when the unrounded distance is below tag_thr, else open a group
        for (int r = 0; r < nr; ++r) {
            const int c = uniform((int)s.col4row[r]);
            bool join = false;
            if (c < n_groups) {
                float t[L];
#pragma unroll
                for (int l = 0; l < L; ++l) t[l] = s.row_tag[r][l];
                join = tag_distance<L>(s, t, c) < p.tag_thr;
            }
            if (__ballot(join) != 0ull) {  // (the same on every lane)
                const int det = uniform((int)s.row_det[r]);
                const size_t src = (size_t)joint * M + det;
                const int x = (lane - joint * W) & (kWave - 1);
                if (x < W) people[(size_t)c * K * W + joint * W + x] = x < 2 ? ind[src * 2 + x] : x == 2 ? val[src] : s.row_tag[r][x - 3];
                const int n = min(uniform((int)s.count[c]), K - 1);  // (at most one tag per step: n <= step)
                if (lane < L) lists[((size_t)n * groups + c) * L + lane] = s.row_tag[r][lane];
                if (lane == 0) {
                    s.count[c] = (unsigned char)(n + 1);
                    s.dirty[c] = 1;
                }
                wave_sync();
            } else {
                num_groups = open_group(joint, r, num_groups);
            }
        }
    }
    if (lane == 0) {
        p.counts[img] = num_groups;
        p.status[img] = 0;
    }
}

static bool bu_match_in_limits(int k, int m, int num_tags) {
    return k <= kBuMatchMaxJoints && m <= kBuMaxM && num_tags <= kBuMaxTags && k * m <= kBuMatchMaxGroups;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_bottomup_match_supported(int k, int m, int num_tags) {
    return k > 0 && m > 0 && num_tags > 0 && bu_match_in_limits(k, m, num_tags) ? 1 : 0;
}

size_t mp_bottomup_match_workspace_bytes(int n, int k, int m, int num_tags) {
    if (n <= 0 || k <= 0 || m <= 0 || num_tags <= 0 || !bu_match_in_limits(k, m, num_tags)) return 0;
    return (size_t)n * k * ((size_t)k * m) * num_tags * sizeof(float);
}

int mp_bottomup_match_by_tag(const float* val_k_dev, const float* tag_k_dev, const float* ind_k_dev, int n, int k, int m, int num_tags,
                             const int* joint_order_host, float vis_thr, float tag_thr, int ignore_too_much, int use_rounded_norm,
                             float* people_dev, int* counts_dev, int* status_dev, void* workspace_dev, size_t workspace_bytes,
                             mp_stream_t stream) {
    if (n == 0) return MP_OK;  // no image: no launch
    if (!val_k_dev || !tag_k_dev || !ind_k_dev || !joint_order_host || !people_dev || !counts_dev || !status_dev) return MP_ERR_NULL;
    if (n < 0 || k <= 0 || m <= 0 || num_tags <= 0) return MP_ERR_SHAPE;
    if (!bu_match_in_limits(k, m, num_tags)) return MP_ERR_UNSUPPORTED;
    BuMatchParams p{};
    bool seen[kBuMatchMaxJoints] = {};
    for (int j = 0; j < k; ++j) {  // the kernel indexes the inputs with these: a permutation of 0 .. k - 1
        const int o = joint_order_host[j];
        if (o < 0 || o >= k || seen[o]) return MP_ERR_SHAPE;
        seen[o] = true;
        p.order[j] = (unsigned char)o;
    }
    const size_t need = mp_bottomup_match_workspace_bytes(n, k, m, num_tags);
    if (!workspace_dev || workspace_bytes < need) return MP_ERR_WORKSPACE;
    p.val = val_k_dev;
    p.tag = tag_k_dev;
    p.ind = ind_k_dev;
    p.k = k;
    p.m = m;
    p.vis_thr = vis_thr;
    p.tag_thr = tag_thr;
    p.ignore_too_much = ignore_too_much ? 1 : 0;
    p.rounded = use_rounded_norm ? 1 : 0;
    p.people = people_dev;
    p.counts = counts_dev;
    p.status = status_dev;
    p.lists = reinterpret_cast<float*>(workspace_dev);
    const dim3 grid((unsigned)n), block(kWave);
    switch (num_tags) {
        case 1: hipLaunchKernelGGL(bu_match_kernel<1>, grid, block, 0, as_stream(stream), p); break;
        case 2: hipLaunchKernelGGL(bu_match_kernel<2>, grid, block, 0, as_stream(stream), p); break;
        case 3: hipLaunchKernelGGL(bu_match_kernel<3>, grid, block, 0, as_stream(stream), p); break;
        default: hipLaunchKernelGGL(bu_match_kernel<4>, grid, block, 0, as_stream(stream), p); break;
    }
    return check_launch();
}

}  // extern "C"
