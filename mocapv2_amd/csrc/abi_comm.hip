// abi_comm.hip -- C-ABI host file: the RCCL binding and the one exchange of the path, an all-gather of centroid records.
#include <dlfcn.h>
#include "ctx.h"

// ---- RCCL, bound at run time -----------------------------------------------------------------------------------
// The path's one exchange is an ncclAllGather of centroid records.  librccl is looked up with dlopen
// when the first communicator call arrives: a process that already holds RCCL (PyTorch ships its own librccl.so.1)
// shares that copy, a plain C host gets /opt/rocm/lib's; single-GPU users never load it.
struct IdBytes { char internal[MOCAP_COMM_ID_BYTES]; }; // layout of ncclUniqueId (rccl.h: 128 opaque bytes, passed by value)
namespace {
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, IdBytes, int) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
}
static Rccl g_rccl;
static std::mutex g_rccl_mu;
static int load_rccl()
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return 0;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(MOCAP_E_UNSUPPORTED, "librccl.so.1 not found: %s", dlerror());
    Rccl r;
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.GetErrorString)
        return fail(MOCAP_E_UNSUPPORTED, "librccl lacks an expected symbol");
    r.lib = h;
    g_rccl = r;
    return 0;
}
#define RCCL_TRY(expr)                                                                                        \
    do {                                                                                                      \
        int r_ = (expr);                                                                                      \
        if (r_ != 0) return fail(MOCAP_E_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r_));             \
    } while (0)

extern "C" {

// ---- the exchange: one all-gather of centroid records (RCCL over xGMI) -------------------------------------------
int mocap_comm_unique_id(void* id_out)
{
    if (!id_out) return fail(MOCAP_E_INVALID, "null argument");
    TRY(load_rccl());
    RCCL_TRY(g_rccl.GetUniqueId(id_out));
    return MOCAP_OK;
}

int mocap_comm_available(void)
{
    return load_rccl();
}

int mocap_comm_init(mocap_ctx_t c, const void* id, int rank, int world)
{
    if (!c || !id) return fail(MOCAP_E_INVALID, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(MOCAP_E_INVALID, "rank %d of %d", rank, world);
    if (c->comm) return fail(MOCAP_E_STATE, "the context already has a communicator");
    TRY(load_rccl());
    if (set_device(c)) return MOCAP_E_HIP;
    auto sc = std::make_shared<SharedComm>();
    HIP_TRY(hipEventCreateWithFlags(&sc->last, hipEventDisableTiming));
    IdBytes idb;
    memcpy(idb.internal, id, sizeof(idb.internal));
    int r_ = g_rccl.CommInitRank(&sc->comm, world, idb, rank);
    if (r_ != 0) // (~SharedComm destroys the event: one owner)
        return fail(MOCAP_E_HIP, "ncclCommInitRank failed: %s", g_rccl.GetErrorString(r_));
    sc->rank = rank; sc->world = world; sc->device = c->device;
    sc->destroy_comm = [](void* comm) { return g_rccl.lib && g_rccl.CommDestroy(comm) == 0; };
    c->comm = sc;
    return MOCAP_OK;
}

int mocap_comm_share(mocap_ctx_t dst, mocap_ctx_t src)
{
    if (!dst || !src) return fail(MOCAP_E_INVALID, "null context");
    if (!src->comm) return fail(MOCAP_E_STATE, "the source context has no communicator");
    if (dst->comm) return fail(MOCAP_E_STATE, "the context already has a communicator");
    if (dst->device != src->device) return fail(MOCAP_E_INVALID, "contexts on different devices cannot share a communicator");
    dst->comm = src->comm;
    return MOCAP_OK;
}

int mocap_comm_destroy(mocap_ctx_t c)
{
    if (!c) return fail(MOCAP_E_INVALID, "null context");
    if (!c->comm) return MOCAP_OK;
    std::shared_ptr<SharedComm> sc = c->comm;
    c->comm.reset();
    if (sc.use_count() > 1) return MOCAP_OK; // other contexts of this rank still use it
    // the last user: destroyed here so that a failure can be reported (the destructor would do the same silently)
    (void)hipSetDevice(sc->device);
    if (sc->have_last) (void)hipEventSynchronize(sc->last);
    (void)hipEventDestroy(sc->last);
    sc->last = nullptr;
    void* comm = sc->comm;
    sc->comm = nullptr;
    if (comm && g_rccl.lib) RCCL_TRY(g_rccl.CommDestroy(comm));
    return MOCAP_OK;
}

int mocap_allgather_centroids(mocap_ctx_t c, const int32_t* local_records, int32_t* gathered, long ints_per_rank, void* stream)
{
    if (!c || !local_records || !gathered) return fail(MOCAP_E_INVALID, "null argument");
    if (ints_per_rank < 1) return fail(MOCAP_E_INVALID, "ints_per_rank = %ld", ints_per_rank);
    if (!c->comm) return fail(MOCAP_E_STATE, "mocap_comm_init / mocap_comm_share was not called for this context");
    if (set_device(c)) return MOCAP_E_HIP;
    SharedComm& sc = *c->comm;
    std::lock_guard<std::mutex> lk(sc.mu);
    if (sc.have_last) HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, sc.last, 0)); // after the communicator's previous all-gather
    RCCL_TRY(g_rccl.AllGather(local_records, gathered, (size_t)ints_per_rank, 2 /* ncclInt32 */, sc.comm, (hipStream_t)stream));
    HIP_TRY(hipEventRecord(sc.last, (hipStream_t)stream));
    sc.have_last = true;
    return MOCAP_OK;
}

} // extern "C"
