// Data-parallel gradient exchange (SURVEY.md 8a row a17, 8b "mp_allreduce_grads"): the gradient mean over ranks on RCCL, in place
// on the flat fp32 gradient arena.  (The overflow check and the update that follow it are in step_end.hip.)
//
// Reference: tools/train.py:43-49 (data_parallel, gradients_mean=True: MindSpore all-reduces every gradient each step).
//
// RCCL is bound at run time (the copy the process already holds - PyTorch ships its own librccl - found with RTLD_NOLOAD; the
// system library only when none is loaded): the library has no link-time dependency on it and single-GPU users never load it.
#include <dlfcn.h>

#include "common.h"

namespace mp {
struct Id128 {  // ncclUniqueId: 128 opaque bytes passed BY VALUE to ncclCommInitRank
    char internal[128];
};
namespace {

// ---- RCCL, bound lazily ------------------------------------------------------------------------------------------------------
struct Rccl {
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, Id128, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommCount)(void*, int*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*ReduceScatter)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    bool ok = false;
};
Rccl& rccl() {
    static Rccl r = [] {
        Rccl t;
        void* h = nullptr;
        if (dlsym(RTLD_DEFAULT, "ncclAllReduce") == nullptr) {
            // PyTorch links its own librccl.so (SONAME librccl.so.1) and Python loads it RTLD_LOCAL, so the symbols are not in the
            // global scope: RTLD_NOLOAD hands out THAT copy by soname.  A second RCCL in the process (two sets of IPC state, two
            // proxy threads per communicator) is never created: only when no copy is loaded at all - a C caller without PyTorch -
            // the system library is loaded.
            h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
            if (h == nullptr) h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
            if (h == nullptr) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
            if (h == nullptr) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        }
        void* scope = h ? h : RTLD_DEFAULT;
        t.GetUniqueId = reinterpret_cast<decltype(t.GetUniqueId)>(dlsym(scope, "ncclGetUniqueId"));
        t.CommInitRank = reinterpret_cast<decltype(t.CommInitRank)>(dlsym(scope, "ncclCommInitRank"));
        t.CommDestroy = reinterpret_cast<decltype(t.CommDestroy)>(dlsym(scope, "ncclCommDestroy"));
        t.CommCount = reinterpret_cast<decltype(t.CommCount)>(dlsym(scope, "ncclCommCount"));
        t.AllReduce = reinterpret_cast<decltype(t.AllReduce)>(dlsym(scope, "ncclAllReduce"));
        t.ReduceScatter = reinterpret_cast<decltype(t.ReduceScatter)>(dlsym(scope, "ncclReduceScatter"));
        t.AllGather = reinterpret_cast<decltype(t.AllGather)>(dlsym(scope, "ncclAllGather"));
        t.GroupStart = reinterpret_cast<decltype(t.GroupStart)>(dlsym(scope, "ncclGroupStart"));
        t.GroupEnd = reinterpret_cast<decltype(t.GroupEnd)>(dlsym(scope, "ncclGroupEnd"));
        t.ok = t.GetUniqueId && t.CommInitRank && t.CommDestroy && t.AllReduce && t.ReduceScatter && t.AllGather && t.GroupStart &&
               t.GroupEnd;
        return t;
    }();
    return r;
}
constexpr int kNcclFloat = 7, kNcclSum = 0, kNcclAvg = 4;  // rccl.h: ncclFloat32 = 7, ncclSum = 0, ncclAvg = 4
thread_local int g_last_rccl_error = 0;
}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

int mp_comm_available(void) { return rccl().ok ? 1 : 0; }

int mp_comm_last_error(void) { return g_last_rccl_error; }

int mp_comm_get_unique_id(void* id128) {
    if (!id128) return MP_ERR_NULL;
    if (!rccl().ok) return MP_ERR_UNSUPPORTED;
    const int rc = rccl().GetUniqueId(id128);
    if (rc != 0) {
        g_last_rccl_error = rc;
        return MP_ERR_HIP;
    }
    return MP_OK;
}

int mp_comm_init_rank(void** comm_out, int nranks, const void* id128, int rank) {
    if (!comm_out || !id128) return MP_ERR_NULL;
    if (nranks <= 0 || rank < 0 || rank >= nranks) return MP_ERR_SHAPE;
    if (!rccl().ok) return MP_ERR_UNSUPPORTED;
    Id128 id;
    __builtin_memcpy(&id, id128, sizeof(id));
    void* comm = nullptr;
    const int rc = rccl().CommInitRank(&comm, nranks, id, rank);
    if (rc != 0) {
        g_last_rccl_error = rc;
        return MP_ERR_HIP;
    }
    *comm_out = comm;
    return MP_OK;
}

int mp_comm_destroy(void* comm) {
    if (!comm) return MP_ERR_NULL;
    if (!rccl().ok) return MP_ERR_UNSUPPORTED;
    const int rc = rccl().CommDestroy(comm);
    if (rc != 0) {
        g_last_rccl_error = rc;
        return MP_ERR_HIP;
    }
    return MP_OK;
}

int mp_comm_count(void* comm) {
    if (!comm || !rccl().ok || !rccl().CommCount) return -1;
    int n = -1;
    const int rc = rccl().CommCount(comm, &n);
    if (rc != 0) {
        g_last_rccl_error = rc;
        return -1;
    }
    return n;
}

int mp_allreduce_grads(void* comm, float* arena, size_t count, int average, mp_stream_t stream) {
    if (!comm || !arena) return MP_ERR_NULL;
    if (count == 0) return MP_OK;
    if (!rccl().ok) return MP_ERR_UNSUPPORTED;
    const int rc = rccl().AllReduce(arena, arena, count, kNcclFloat, average ? kNcclAvg : kNcclSum, comm, as_stream(stream));
    if (rc != 0) {
        g_last_rccl_error = rc;
        return MP_ERR_HIP;
    }
    return MP_OK;
}

int mp_reduce_scatter_allgather_grads(void* comm, float* arena, size_t count, int nranks, int rank, int average, mp_stream_t stream) {
    if (!comm || !arena) return MP_ERR_NULL;
    if (nranks <= 0 || rank < 0 || rank >= nranks) return MP_ERR_SHAPE;
    if (count == 0) return MP_OK;
    if (count % (size_t)nranks != 0) return MP_ERR_SHAPE;  // the caller pads the arena to a multiple of the world size
    if (!rccl().ok) return MP_ERR_UNSUPPORTED;
    const size_t shard = count / (size_t)nranks;
    hipStream_t s = as_stream(stream);
    int rc = rccl().ReduceScatter(arena, arena + (size_t)rank * shard, shard, kNcclFloat, average ? kNcclAvg : kNcclSum, comm, s);
    if (rc == 0) rc = rccl().AllGather(arena + (size_t)rank * shard, arena, shard, kNcclFloat, comm, s);
    if (rc != 0) {
        g_last_rccl_error = rc;
        return MP_ERR_HIP;
    }
    return MP_OK;
}

}  // extern "C"
