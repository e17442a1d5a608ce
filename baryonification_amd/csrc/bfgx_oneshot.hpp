// The support code of the one-shot host entries (bfgx_baryonify_shell / _grid / _snapshot_records ...; bfgx_api.hip includes it where that section
// starts): what keeps a call safe on every return path, the plan caches, the test knobs and the phase timing.  Needs fail, alloc_fail, HIP_TRY,
// DevBuf / PoolBuf, validate_model and the three plan types (declared is enough for the grid and snapshot plans).
#pragma once
namespace {

std::atomic<long long> g_host_pinned_in_place{0}, g_host_staged{0}, g_host_pin_min_bytes{-1};      // HostSpan (bfgx_debug_host_spans)

// Every one-shot host entry leaves NOTHING in flight when it returns -- on success and on every error path: asynchronous copies read the
// caller's arrays (page-locked for the call, or pinned on the fly by the runtime) and write into the caller's result; a copy that is
// still running when the caller frees or reuses those arrays is a GPU memory fault at a host address.  Its streams are drained at scope exit whatever the return path --
// after the HostSpans have unregistered: OneShotCall (below) holds it as its FIRST member, so that it is destroyed last.
struct DrainOnExit {
    hipStream_t *s[4] = {nullptr, nullptr, nullptr, nullptr};
    bool null_stream = false;
    ~DrainOnExit()
    {
        for (hipStream_t *q : s) if (q && *q) (void)hipStreamSynchronize(*q);
        if (null_stream) (void)hipStreamSynchronize(nullptr);
    }
};

// a stream of the call's own, drained and destroyed at scope exit
struct CallStream {
    hipStream_t s = nullptr;
    ~CallStream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } }
};

// The halo columns of a box or grid catalog on the device: hcol[0 .. 3] = M, x, y, z (z: allocated, not filled, for ndim 2) of the nh halos of a host catalog, on stream st; at least one element each
int upload_halo_columns(hipStream_t st, const bfgx_grid_catalog *c, int32_t ndim, int64_t nh, DevBuf *hcol)
{
    const double *hsrc[4] = {c->M, c->x, c->y, ndim == 3 ? c->z : nullptr};
    for (int k = 0; k < 4; ++k) {
        if (hcol[k].alloc(sizeof(double) * (size_t)std::max<int64_t>(nh, 1))) return alloc_fail("catalog");
        // (a copy from pageable host memory has left the caller's array when hipMemcpyAsync returns)
        if (nh > 0 && hsrc[k]) HIP_TRY(hipMemcpyAsync(hcol[k].p, hsrc[k], sizeof(double) * (size_t)nh, hipMemcpyHostToDevice, st));
    }
    return BFGX_OK;
}

// A caller's host array as the source / destination of the ASYNCHRONOUS copies of a one-shot entry:
//  * already page-locked by the caller (bfgx_host_alloc): used as it is;
//  * >= 32 MiB -- beyond glibc's largest mmap threshold, i.e. a mapping of its own that shares no page with another object: page-locked in
//    place for the call (hipHostRegister);
//  * smaller: NEVER page-locked in place.  A small numpy array lives in the process heap next to other live objects; page-locking and
//    unlocking those pages call after call left a later, ordinary pageable copy from the same heap region reading through a mapping that
//    was gone (seen twice in round 4 as "Memory access fault by GPU ... on address <heap address>").  Small arrays take the entry's
//    synchronous route; `stage` (tests force the streamed route on small maps: BFGX_PIPE_CHUNKS) goes through a page-locked buffer of ours.
constexpr size_t kPinInPlaceMin = (size_t)32 << 20;
struct HostSpan {
    void *user = nullptr, *use = nullptr;
    size_t bytes = 0;
    bool registered = false, staged = false, is_out = false;
    hipStream_t *streams[3] = {nullptr, nullptr, nullptr};       // copies of the span may be in flight on these when an error returns early
    bool open(const void *q, size_t nb, bool out, bool stage)
    {
        user = (void *)q; bytes = nb; is_out = out;
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, q) == hipSuccess && at.type == hipMemoryTypeHost) { use = user; return true; }
        (void)hipGetLastError();
        if (nb >= kPinInPlaceMin) {
            if (hipHostRegister(user, nb, hipHostRegisterDefault) == hipSuccess) {
                registered = true; use = user;
                ++g_host_pinned_in_place;
                long long m = g_host_pin_min_bytes.load();
                while ((m < 0 || (long long)nb < m) && !g_host_pin_min_bytes.compare_exchange_weak(m, (long long)nb)) {}
                return true;
            }
            (void)hipGetLastError();
            return false;
        }
        if (!stage) return false;
        if (hipHostMalloc(&use, nb ? nb : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); use = nullptr; return false; }
        staged = true;
        ++g_host_staged;
        if (!out) std::memcpy(use, q, nb);
        return true;
    }
    void drain() const { for (hipStream_t *s : streams) if (s && *s) (void)hipStreamSynchronize(*s); }
    // success path, after the entry has drained its streams: a staged result reaches the caller's array
    void commit() { if (staged && is_out && use) { drain(); std::memcpy(user, use, bytes); } }
    ~HostSpan()
    {
        if (!registered && !staged) return;
        drain();                                             // never unlock / free a buffer a copy still uses
        if (registered) (void)hipHostUnregister(user);
        if (staged && use) (void)hipHostFree(use);
    }
};

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
    Timer() { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    ~Timer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void start(hipStream_t s) { (void)hipEventRecord(a, s); }
    double stop(hipStream_t s) { (void)hipEventRecord(b, s); (void)hipEventSynchronize(b); float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return ms; }
    double lap(hipStream_t s) { const double ms = stop(s); start(s); return ms; }      // the end of one phase is the start of the next
};

// ---- plan caches of the one-shot API: a process() call re-uses the plan (model on the device, tiling, binning workspace) and the
// device buffers of the previous call with the same model, geometry and device, so that a warm call performs no hipMalloc

// The key of a cached entry: two independent 64-bit hashes (an FNV-style basis and prime; another basis and odd multiplier) and the
// model table's value count.  A hit needs all three to agree, so that one 64-bit collision cannot hand a model another model's table.
struct CacheKey {
    uint64_t h[2] = {0xcbf29ce484222325ull, 0x2545f4914f6cdd1dull};
    int64_t values = 0;
    void add(const void *data, size_t bytes)
    {
        constexpr uint64_t m0 = 0x100000001b3ull, m1 = 0x9e3779b97f4a7c15ull;
        const unsigned char *c = (const unsigned char *)data;
        uint64_t a = h[0], b = h[1];
        size_t i = 0;
        for (; i + 8 <= bytes; i += 8) {
            uint64_t w;
            std::memcpy(&w, c + i, 8);
            a = (a ^ w) * m0; a ^= a >> 29;
            b = (b ^ w) * m1; b ^= b >> 29;
        }
        for (; i < bytes; ++i) { a = (a ^ c[i]) * m0; b = (b ^ c[i]) * m1; }
        h[0] = a; h[1] = b;
    }
    template <typename T> void add(const T &v) { add(&v, sizeof(v)); }
    bool operator==(const CacheKey &o) const { return h[0] == o.h[0] && h[1] == o.h[1] && values == o.values; }
};

// (device, model contents); the model has been validated: its table pointers are readable.  Each cache adds its geometry.
CacheKey model_key(int device, const bfgx_model *m)
{
    CacheKey k;
    k.add(device);
    const bfgx_table &t = m->table;
    k.add(t.ndim);
    k.add(t.n, sizeof(t.n));
    size_t nv = 1;
    for (int d = 0; d < t.ndim; ++d) { k.add(t.axis[d], sizeof(double) * (size_t)t.n[d]); nv *= (size_t)t.n[d]; }
    k.add(t.values, sizeof(double) * nv);
    k.add(&t.rdelta_sampling, sizeof(int32_t) * 2);
    k.add(t.eps_model);
    k.add(m->cosmo_runner); k.add(m->cosmo_model);
    k.add(m->massdef_runner.Delta); k.add(m->massdef_runner.rho_type);
    k.add(m->massdef_model.Delta); k.add(m->massdef_model.rho_type);
    k.add(m->eps_runner);
    k.values = (int64_t)nv;
    return k;
}

// A cached entry: its key, its plan and its streams and events.  The data travels up and down on streams of its own while the plan's
// stream computes; phase events (timed) for bfgx_stats; two pools of per-range events: a range has arrived (ev_up) / has been computed (ev_k).
template <typename Plan> struct CacheEntry {
    CacheKey key;
    uint64_t stamp = 0;
    int device = 0;
    Plan *plan = nullptr;
    hipStream_t up = nullptr, down = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> ev_up, ev_k;
    int create()
    {
        HIP_TRY(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
        for (auto &v : ev) HIP_TRY(hipEventCreate(&v));
        return BFGX_OK;
    }
    // at least nup events in ev_up and nk in ev_k
    int pools(int nup, int nk)
    {
        while ((int)ev_up.size() < nup || (int)ev_k.size() < nk) {
            std::vector<hipEvent_t> &pool = (int)ev_up.size() < nup ? ev_up : ev_k;
            hipEvent_t v;
            HIP_TRY(hipEventCreateWithFlags(&v, hipEventDisableTiming));
            pool.push_back(v);
        }
        return BFGX_OK;
    }
    ~CacheEntry()            // (the plan is destroyed by PlanCache::drop, before the entry's own buffers are freed)
    {
        if (up) (void)hipStreamDestroy(up);
        if (down) (void)hipStreamDestroy(down);
        for (auto &v : ev) if (v) (void)hipEventDestroy(v);
        for (auto &v : ev_up) (void)hipEventDestroy(v);
        for (auto &v : ev_k) (void)hipEventDestroy(v);
    }
};

void plan_destroy(bfgx_plan *p) { bfgx_plan_destroy(p); }
void plan_destroy(bfgx_grid_plan *p) { bfgx_grid_plan_destroy(p); }
void plan_destroy(bfgx_snapshot_plan *p) { bfgx_snapshot_plan_destroy(p); }

// A least-recently-used cache of at most kMax entries E (a CacheEntry<Plan> with the entry's own device buffers).  One call at a time
// holds mu; the shell, grid and snapshot entries each have a cache (and a mutex) of their own.
template <typename E, size_t kMax> struct PlanCache {
    std::mutex mu;
    std::vector<E *> v;
    uint64_t stamp = 0;

    static void drop(E *e)
    {
        (void)hipSetDevice(e->device);
        if (e->plan) plan_destroy(e->plan);
        delete e;
    }
    // the entry for key, with a plan for at least n halos (make(capacity, &plan) builds it) and its streams; setup(e) then readies the
    // entry's own buffers.  An entry whose set-up fails is removed.  mu is held by the caller.
    template <typename Make, typename Setup> int acquire(const CacheKey &key, int device, int64_t n, Make make, Setup setup, E **out)
    {
        auto it = std::find_if(v.begin(), v.end(), [&](E *c) { return c->key == key; });
        E *e = it != v.end() ? *it : nullptr;
        if (e && e->plan->max_halos < n) {                   // grew: rebuild the plan (its workspace scales with max_halos)
            (void)hipSetDevice(device);
            plan_destroy(e->plan);
            e->plan = nullptr;
        }
        if (!e) {
            if (v.size() >= kMax) {
                auto lru = std::min_element(v.begin(), v.end(), [](E *a, E *b) { return a->stamp < b->stamp; });
                drop(*lru);
                v.erase(lru);
            }
            e = new E();
            e->key = key; e->device = device;
            v.push_back(e);
        }
        int rc = BFGX_OK;
        if (!e->plan && (rc = make(std::max<int64_t>(n + n / 4, 1024), &e->plan))) e->plan = nullptr;
        if (!rc && hipSetDevice(device) != hipSuccess) rc = fail(BFGX_ERR_HIP, "hipSetDevice(%d) failed", device);
        if (!rc && !e->up) rc = e->create();
        if (!rc) rc = setup(e);
        if (rc) {
            v.erase(std::find(v.begin(), v.end(), e));
            drop(e);
            return rc;
        }
        e->stamp = ++stamp;
        *out = e;
        return BFGX_OK;
    }
    void clear()
    {
        std::lock_guard<std::mutex> lk(mu);
        for (E *e : v) drop(e);
        v.clear();
    }
};

// np.isclose(new_sum, old_sum): rtol 1e-5, atol 1e-8  (HealpixRunner.py:344-346)
int check_mass(double sum_in, double sum_out)
{
    if (!(std::fabs(sum_out - sum_in) <= 1e-8 + 1e-5 * std::fabs(sum_in)))
        return fail(BFGX_ERR_MASS, "ERROR in pixel regridding, sum(new_map) [%0.14e] != sum(oldmap) [%0.14e]", sum_out, sum_in);
    return BFGX_OK;
}

// the options of a one-shot entry; NULL: the defaults (each entry reads only its own fields)
bfgx_opts entry_opts(const bfgx_opts *opts)
{
    bfgx_opts o{};
    o.check_mass = 1; o.algo = 1; o.acc_offsets_f64 = BFGX_ACC_AUTO; o.acc_paint_f64 = 1;
    if (opts) o = *opts;
    return o;
}

// The two test knobs of the streamed routes, read once per call: BFGX_PIPE_CHUNKS sets the number of ranges (each entry clamps `chunks` to its
// own limits; small arrays then go through a page-locked staging buffer: HostSpan), BFGX_NO_PIPELINE sends every call down the one-pass route.
struct PipeKnobs { int chunks; bool stage; bool off; };
PipeKnobs pipe_knobs()
{
    const char *c = std::getenv("BFGX_PIPE_CHUNKS");
    return PipeKnobs{c ? std::atoi(c) : 0, c != nullptr, std::getenv("BFGX_NO_PIPELINE") != nullptr};
}

template <typename T> struct Restore { T &ref; T value; ~Restore() { ref = value; } };      // a plan field set back at scope exit, whatever the return path

// the bfgx_stats of a call (sums: NULL for the entries without a mass check).  No phase is negative: an elapsed time between events on
// two streams can come out slightly below zero, which means nothing.
void fill_stats(bfgx_stats *stats, const double *sums, int64_t n_pairs, double ms_h2d, double ms_kernels, double ms_d2h)
{
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats));
    if (sums) { stats->sum_in = sums[0]; stats->sum_out = sums[1]; }
    stats->ms_h2d = std::max(ms_h2d, 0.0); stats->ms_kernels = std::max(ms_kernels, 0.0); stats->ms_d2h = std::max(ms_d2h, 0.0);
    stats->n_pairs = n_pairs;
}

// The scope of one call of a one-shot entry, built from the plan's stream and the cached entry (its streams up / down and its four phase
// events) once the entry is acquired.  MEMBER ORDER IS THE SAFETY RULE: C++ destroys members in reverse, so the two HostSpans unregister /
// free (each after draining the streams itself) BEFORE `drain` synchronises the streams for the last time -- no entry can get it wrong.
struct OneShotCall {
    DrainOnExit drain;
    HostSpan in, out;
    hipEvent_t *ev = nullptr;
    bool ended = false;
    explicit OneShotCall(hipStream_t *plan_stream, hipStream_t *up = nullptr, hipStream_t *down = nullptr)
    {
        hipStream_t *s[3] = {plan_stream, up, down};
        for (int i = 0; i < 3; ++i) drain.s[i] = in.streams[i] = out.streams[i] = s[i];
        drain.null_stream = (*plan_stream == nullptr);
    }
    template <typename Plan> OneShotCall(hipStream_t *plan_stream, CacheEntry<Plan> *e) : OneShotCall(plan_stream, &e->up, &e->down) { ev = e->ev; }
    // page-locked views of the caller's arrays for the streamed route (false: pageable memory, take the one-pass route)
    bool open_in(const void *src, size_t bytes, bool stage) { return in.open(src, bytes, false, stage); }
    bool open_out(void *dst, size_t bytes, bool stage) { return out.open(dst, bytes, true, stage); }
    bool open(const void *src, size_t src_bytes, void *dst, size_t dst_bytes, bool stage) { return open_in(src, src_bytes, stage) && open_out(dst, dst_bytes, stage); }
    template <typename T> const T *src() const { return (const T *)in.use; }
    template <typename T> T *dst() const { return (T *)out.use; }
    void commit() { out.commit(); }                          // success path: a staged result reaches the caller's array
    // phase marks: 0 start, 1 the last byte has arrived, 2 the kernels are done, 3 (optional) the result has left
    int mark(int i, hipStream_t s) { ended = ended || i == 3; HIP_TRY(hipEventRecord(ev[i], s)); return BFGX_OK; }
    // the three phases between the marks (the last one ends when mark 3 is reached on its stream) and the rest of bfgx_stats
    int finish(bfgx_stats *stats, const double *sums, int64_t n_pairs)
    {
        float ms[3] = {0, 0, 0};
        if (ended) HIP_TRY(hipEventSynchronize(ev[3]));
        for (int i = 0; i < (ended ? 3 : 2); ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
        fill_stats(stats, sums, n_pairs, ms[0], ms[1], ms[2]);
        return BFGX_OK;
    }
};

}  // namespace
