// abi_ctx.hip -- the C-ABI of libmocap_hip.so (declared in include/mocap_hip.h), first of six host files that hold argument checks
// and kernel launches and no compute: the error channel, the context's life cycle, its parameters, tuning switches, camera
// tables and profiling.
#include <stdarg.h>
#include "ctx.h"

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

struct TuneName { const char* name; int Tuning::*field; int lo, hi; };
static const TuneName kTuneNames[] = {
#define X(name, def, lo, hi) {#name, &Tuning::name, lo, hi},
#include "tuning.def"
#undef X
};
static bool tune_set(Tuning& t, const char* name, int v)
{
    for (const TuneName& n : kTuneNames)
        if (!strcmp(n.name, name)) {
            t.*(n.field) = v < n.lo ? n.lo : (v > n.hi ? n.hi : v);
            return true;
        }
    return false;
}
static Tuning tuning_from_env()
{
    Tuning t;
    for (const TuneName& n : kTuneNames) {
        char env[64] = "MOCAP_";
        size_t k = strlen(env);
        for (const char* p = n.name; *p && k + 1 < sizeof(env); p++) env[k++] = (char)((*p >= 'a' && *p <= 'z') ? *p - 32 : *p);
        env[k] = 0;
        const char* e = getenv(env);
        if (e && *e) tune_set(t, n.name, atoi(e));
    }
    { const char* e = getenv("MOCAP_WIDE_QUADS"); int r_ = 0, i_ = 0; // "remap,identity"
      if (e && sscanf(e, "%d,%d", &r_, &i_) == 2) { tune_set(t, "wide_quads_remap", r_); tune_set(t, "wide_quads_identity", i_); } }
    return t;
}

// ---- profiling -------------------------------------------------------------------------------------------------
void prof_begin(mocap_ctx* c, hipStream_t s, EvPair& p, bool& on)
{
    on = c->profiling;
    if (!on) return;
    if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) { on = false; return; }
    (void)hipEventRecord(p.a, s);
}
void prof_end(mocap_ctx* c, ProfSlot slot, hipStream_t s, EvPair& p, bool on)
{
    if (!on) return;
    (void)hipEventRecord(p.b, s);
    std::lock_guard<std::mutex> lk(c->mu);
    c->ev[slot].push_back(p);
}

extern "C" {

int mocap_abi_version(void) { return MOCAP_ABI_VERSION; }
const char* mocap_last_error(void) { return g_err.c_str(); }

int mocap_ctx_create(int device_id, int width, int height, int n_slots, mocap_ctx_t* out)
{
    if (!out || width < 1 || height < 1 || width > 32767 || height > 32767 || n_slots < 1 || n_slots > 64)
        return fail(MOCAP_E_INVALID, "mocap_ctx_create: bad geometry %dx%d slots=%d", width, height, n_slots);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(MOCAP_E_HIP, "mocap_ctx_create: no HIP device %d (%d visible)", device_id, ndev);
    HIP_TRY(hipSetDevice(device_id));
    std::unique_ptr<mocap_ctx, int (*)(mocap_ctx*)> c(new mocap_ctx(), mocap_ctx_destroy); // (destroyed by every early return)
    c->device = device_id; c->W = width; c->H = height; c->n_slots = n_slots; c->wpr = (width + 31) / 32;
    c->tune = tuning_from_env();
    c->base_sel = c->tune.base_sel;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) {
            c->box_grid = box_filter_blocks_per_cu() * prop.multiProcessorCount;
            c->n_cu = prop.multiProcessorCount;
            if (c->tune.box_blocks_per_cu >= 1) c->box_grid = c->tune.box_blocks_per_cu * prop.multiProcessorCount; // A/B switch
        }
    }
    c->slot_state.assign(n_slots, 0);
    c->slot_compact.assign(n_slots, 0);
    c->slot_wmax.assign(n_slots, 0);
    TRY(c->map_flags.reserve(n_slots + 64, true));
    TRY(c->n_items.reserve(256, true)); // item count + the 8 head words of the box kernel's runs
    TRY(c->probe_dev.reserve(PROBE_BYTES / sizeof(uint32_t)));
    TRY(c->probe_host.reserve(PROBE_BYTES / sizeof(uint32_t)));
    HIP_TRY(hipEventCreateWithFlags(&c->probe_ev, hipEventDisableTiming));
    // (the side stream of wide_fork is created on first use: every stream a process holds is dealt onto one of a few hardware
    // queues, and a stream nobody uses can end up sharing a queue with a batch's own stream)
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    TRY(c->cams.reserve(1, true));
    *out = c.release();
    return MOCAP_OK;
}

int mocap_ctx_destroy(mocap_ctx_t c)
{
    if (!c) return MOCAP_OK;
    (void)hipSetDevice(c->device);
    for (auto& v : c->ev) for (auto& p : v) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    (void)mocap_comm_destroy(c);
    if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    // before probe_host / probe_dev go away: an asynchronous copy into the pinned block may be in flight
    if (c->probe_ev) { (void)hipEventSynchronize(c->probe_ev); (void)hipEventDestroy(c->probe_ev); }
    delete c; // releases every buffer
    return MOCAP_OK;
}

int mocap_sync(mocap_ctx_t c, void* stream)
{
    if (!c) return fail(MOCAP_E_INVALID, "null context");
    if (set_device(c)) return MOCAP_E_HIP;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return MOCAP_OK;
}

int mocap_set_blob_params(mocap_ctx_t c, const mocap_blob_params* p)
{
    if (!c || !p) return fail(MOCAP_E_INVALID, "null argument");
    if (p->ksize != 5 || p->median != 5)
        return fail(MOCAP_E_UNSUPPORTED, "only the reference's 5x5 blur and 5x5 median are implemented (got %d, %d)", p->ksize, p->median);
    if (!(p->thresh == p->thresh)) return fail(MOCAP_E_INVALID, "thresh is NaN");
    c->prm = *p;
    return MOCAP_OK;
}

int mocap_set_tuning(mocap_ctx_t c, const char* name, int value)
{
    if (!c || !name) return fail(MOCAP_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!strcmp(name, "rows") || !strcmp(name, "box_blocks_per_cu") || !strcmp(name, "base_sel"))
        return fail(MOCAP_E_STATE, "tuning '%s' shapes the context's buffers: set MOCAP_%s in the environment before mocap_ctx_create", name, name);
    if (!tune_set(c->tune, name, value)) return fail(MOCAP_E_INVALID, "unknown tuning name '%s'", name);
    return MOCAP_OK;
}

int mocap_set_cameras(mocap_ctx_t c, int n, const double* K, const double* dist, const double* R, const double* t)
{
    if (!c || !K || !dist || !R || !t) return fail(MOCAP_E_INVALID, "null argument");
    if (n < 1 || n > 32) return fail(MOCAP_E_INVALID, "camera count %d not in 1..32", n);
    if (set_device(c)) return MOCAP_E_HIP;
    HIP_TRY(hipMemcpy(&c->cams->K[0][0], K, sizeof(double) * 9 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(&c->cams->dist[0][0], dist, sizeof(double) * 5 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(&c->cams->R[0][0], R, sizeof(double) * 9 * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(&c->cams->t[0][0], t, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
    c->n_cam = n;
    return MOCAP_OK;
}

int mocap_set_fundamentals(mocap_ctx_t c, int n, const double* F)
{
    if (!c || (n > 0 && !F)) return fail(MOCAP_E_INVALID, "null argument");
    if (n < 0 || n > 31) return fail(MOCAP_E_INVALID, "fundamental matrix count %d not in 0..31", n);
    if (set_device(c)) return MOCAP_E_HIP;
    if (n) HIP_TRY(hipMemcpy(&c->cams->F[0][0], F, sizeof(double) * 9 * n, hipMemcpyHostToDevice));
    c->n_F = n;
    return MOCAP_OK;
}

int mocap_profile_enable(mocap_ctx_t c, int on)
{
    if (!c) return fail(MOCAP_E_INVALID, "null context");
    c->profiling = on != 0;
    return MOCAP_OK;
}

int mocap_profile_read(mocap_ctx_t c, double ms[5], int cnt[5])
{
    if (!c || !ms || !cnt) return fail(MOCAP_E_INVALID, "null argument");
    if (set_device(c)) return MOCAP_E_HIP;
    for (int w = 0; w < PROF_SLOTS; w++) { ms[w] = 0; cnt[w] = 0; }
    std::lock_guard<std::mutex> lk(c->mu);
    for (int w = 0; w < PROF_SLOTS; w++) {
        for (auto& p : c->ev[w]) {
            HIP_TRY(hipEventSynchronize(p.b));
            float f = 0;
            HIP_TRY(hipEventElapsedTime(&f, p.a, p.b));
            ms[w] += f; cnt[w]++;
            (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b);
        }
        c->ev[w].clear();
    }
    return MOCAP_OK;
}

} // extern "C"
