// s2d_multi.hip -- several GPUs behind ONE handle: the extern "C" entry points (include/splat2d.h "s2d_multi_*"), on the
// caller's thread.  What the handle is made of and which unit holds what: s2d_multi.h.
#include "s2d_multi.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "s2d_multi_plan.h"

using namespace s2d::multi;

namespace {

// The s2d_multi_* calls select devices (hipSetDevice is per thread) from the CALLER's thread: put its device back on the
// way out, a caller that shares the thread with other HIP code (torch) does not expect it to have moved.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// `call` on every replica in turn, from the caller's thread (the workers are idle between commands).
template <typename Call>
int each_ctx(s2d_multi* m, const char* what, Call call)
{
    for (const Rank& R : m->ranks)
        if (int rc = call(R.ctx)) return mfail(m, rc, "%s on rank %d (device %d): %s", what, R.index, R.device, s2d_last_error(R.ctx));
    return S2D_OK;
}

// What the handle's scheme needs beside the contexts.
int set_up_scheme(s2d_multi* m)
{
    if (m->scheme == SCHEME_REPLICATED) return set_up_replicated(m);
    if (m->scheme == SCHEME_OWNERSHIP) return set_up_peer_access(m);
    return S2D_OK;
}

} // namespace

extern "C" {

int s2d_multi_create(const s2d_config* cfg, const int32_t* devices, int32_t n_devices, uint32_t flags, s2d_multi** out)
{
    if (!cfg || !out || !devices || n_devices < 1 || n_devices > 32 || cfg->struct_size != sizeof(s2d_config)) return S2D_E_INVALID;
    *out = nullptr;
    if (cfg->row_begin != 0 || cfg->row_end != 0 || cfg->stream != nullptr) return S2D_E_INVALID; // the handle cuts the slabs itself
    if (cfg->flags & S2D_CFG_REFERENCE_ORDER) return S2D_E_INVALID; // one device's validation mode: its chains run over all splats
    if (cfg->flags & S2D_CFG_COVERAGE) return S2D_E_INVALID;        // the coverage channel has no slab kernels (and no fused one)
    DeviceGuard guard;
    s2d_multi* m = new (std::nothrow) s2d_multi();
    if (!m) return S2D_E_NOMEM;
    *out = m; // handed out even on failure so that s2d_multi_last_error works; the caller destroys it
    m->world = n_devices;
    m->W = cfg->width;
    m->H = cfg->height;
    m->n = cfg->n_splats;
    m->mse_norm = (double)((long long)m->H * m->W * 3);
    m->share_gpu = (flags & S2D_MULTI_SHARE_GPU) != 0;
    m->scheme = (flags & S2D_MULTI_REPLICATED) ? SCHEME_REPLICATED : (n_devices > 1 ? SCHEME_OWNERSHIP : SCHEME_NONE);
    m->ranks = std::vector<Rank>((size_t)m->world);
    m->bounds.assign((size_t)m->world + 1, m->H);
    m->barrier.n = m->world;
    if (const char* e = getenv("S2D_MULTI_STALL_TIMEOUT_MS")) m->stall_ms = std::max(0, atoi(e));
    if ((m->H + 15) / 16 < m->world) return mfail(m, S2D_E_INVALID, "%d devices for %d tile rows", m->world, (m->H + 15) / 16);
    for (int r = 0; r < m->world; r++) {
        Rank& R = m->ranks[(size_t)r];
        R.index = r;
        R.device = devices[m->share_gpu ? 0 : r];
        s2d_config c = *cfg;
        c.device = R.device;
        s2d::slab_rows(m->H, r, m->world, &c.row_begin, &c.row_end);
        m->bounds[(size_t)r] = R.row_begin = c.row_begin;
        R.row_end = c.row_end;
        const int rc = s2d_create(&c, &R.ctx);
        if (rc != S2D_OK)
            return mfail(m, rc, "s2d_create for device %d, rows %d..%d: %s", c.device, c.row_begin, c.row_end,
                         R.ctx ? s2d_last_error(R.ctx) : "rejected configuration");
        if (hipSetDevice(R.device) != hipSuccess) return mfail(m, S2D_E_HIP, "hipSetDevice(%d)", R.device);
        for (Event& e : R.ev_prog)
            if (e.create(hipEventDisableTiming) != hipSuccess) return mfail(m, S2D_E_HIP, "hipEventCreate on device %d", R.device);
    }
    // Adam moves a parameter by at most lr * |m^| / sqrt(v^) <= 2.35 * lr per step for beta = (0.9, 0.99); pos.y moves by
    // that and reach = 3 * max(sx, sy) + 2 by three times that: the margin must outlast one refresh interval
    const float lr = cfg->training_rate > 0.0f ? cfg->training_rate : 0.05f;
    m->margin = std::max(8.0f, 1.1f * 2.35f * 4.0f * lr * (float)m->interval);
    if (int rc = set_up_scheme(m)) return rc;
    start_workers(m);
    return S2D_OK;
}

void s2d_multi_destroy(s2d_multi* m)
{
    if (!m) return;
    DeviceGuard guard;
    if (m->health == Health::Abandoned) {
        // some worker sits inside a runtime call that never returned: it cannot be joined, and what it may still touch
        // -- the handle, its context, its device memory -- cannot be freed under it.  Abandon all of it.
        for (auto& t : m->workers) t.detach();
        return;
    }
    quit_workers(m); // every worker lets its rank's resources go (Rank::let_go)
    for (Rank& R : m->ranks) {
        if (m->workers.empty()) R.let_go(); // creation failed before any worker was started
        destroy_communicator(m, R);
    }
    for (Rank& R : m->ranks)
        if (R.ctx) s2d_destroy(R.ctx);
    delete m;
}

const char* s2d_multi_last_error(const s2d_multi* m) { return m ? m->err : "null handle"; }

int s2d_multi_device_count(const s2d_multi* m) { return m ? m->world : 0; }

int s2d_multi_set_stall_timeout(s2d_multi* m, int32_t milliseconds)
{
    if (!m || milliseconds < 0) return S2D_E_INVALID;
    m->stall_ms = milliseconds;
    return S2D_OK;
}

int s2d_multi_device_info(s2d_multi* m, int32_t rank, int32_t* device, int32_t* row_begin, int32_t* row_end, char* pci_bus_id,
                          int32_t pci_capacity, char* name, int32_t name_capacity)
{
    if (!m || rank < 0 || rank >= m->world) return S2D_E_INVALID;
    const Rank& R = m->ranks[(size_t)rank];
    if (device) *device = R.device;
    if (row_begin) *row_begin = R.row_begin;
    if (row_end) *row_end = R.row_end;
    if (pci_bus_id && pci_capacity > 0) {
        pci_bus_id[0] = 0;
        if (hipDeviceGetPCIBusId(pci_bus_id, pci_capacity, R.device) != hipSuccess) {
            (void)hipGetLastError();
            pci_bus_id[0] = 0;
        }
    }
    if (name && name_capacity > 0) {
        hipDeviceProp_t prop;
        name[0] = 0;
        if (hipGetDeviceProperties(&prop, R.device) == hipSuccess) snprintf(name, (size_t)name_capacity, "%s", prop.name);
        else (void)hipGetLastError();
    }
    return S2D_OK;
}

int s2d_test_multi_stall(s2d_multi* m, int32_t rank, int32_t iteration, int32_t milliseconds)
{
    if (!m) return S2D_E_INVALID;
    m->stall_rank = rank;
    m->stall_iter = iteration;
    m->stall_for_ms = milliseconds;
    return S2D_OK;
}

int s2d_multi_exchange_info(s2d_multi* m, int64_t* out4)
{
    if (!m || !out4) return S2D_E_INVALID;
    out4[0] = m->scheme;
    out4[1] = out4[2] = out4[3] = 0;
    if (m->scheme == SCHEME_OWNERSHIP && m->hold_valid)
        for (const Rank& R : m->ranks) {
            out4[1] += R.halo.total;
            out4[2] += R.halo.handed;
            out4[3] += (int64_t)R.halo.held.size();
        }
    else
        out4[3] = (int64_t)m->n * m->world;
    return S2D_OK;
}

int s2d_multi_set_target(s2d_multi* m, const float* rgba32f)
{
    if (!m || !rgba32f) return S2D_E_INVALID;
    DeviceGuard guard;
    return each_ctx(m, "s2d_set_target", [&](s2d_ctx* c) { return s2d_set_target(c, rgba32f); });
}

int s2d_multi_set_target_synthetic(s2d_multi* m)
{
    if (!m) return S2D_E_INVALID;
    DeviceGuard guard;
    return each_ctx(m, "s2d_set_target_synthetic", s2d_set_target_synthetic);
}

int s2d_multi_init_splats(s2d_multi* m)
{
    if (!m) return S2D_E_INVALID;
    DeviceGuard guard;
    if (int rc = each_ctx(m, "s2d_init_splats", s2d_init_splats)) return rc; // every replica: the same deterministic init(), main.cpp:280-305
    m->iterations = 0;
    state_set_afresh(m);
    m->hold_valid = false; // every replica is complete again: new hold sets at the next step
    return S2D_OK;
}

int s2d_multi_get_adam(s2d_multi* m, s2d_splat_adam* adams, float* beta1t, float* beta2t, int32_t* iterations)
{
    if (!m) return S2D_E_INVALID;
    DeviceGuard guard;
    s2d_ctx* first = m->ranks[0].ctx;
    if (m->scheme == SCHEME_OWNERSHIP && m->hold_valid && adams) {
        if (int rc = assemble_adam(m, adams)) return rc;
        adams = nullptr;
    }
    if (int rc = s2d_get_adam(first, adams, beta1t, beta2t, iterations)) return mfail(m, rc, "s2d_get_adam: %s", s2d_last_error(first));
    return S2D_OK;
}

int s2d_multi_set_splats(s2d_multi* m, const s2d_splat* splats)
{
    if (!m || (!splats && m->n)) return S2D_E_INVALID;
    DeviceGuard guard;
    if (m->scheme == SCHEME_OWNERSHIP && m->hold_valid) {
        // the replicas are about to hold everything again: complete their Adam state first (a rank has current
        // moments only for the splats it holds)
        std::vector<s2d_splat_adam> full((size_t)m->n);
        float b1 = 0.f, b2 = 0.f;
        int32_t it = 0;
        if (int rc = s2d_multi_get_adam(m, full.data(), &b1, &b2, &it)) return rc;
        if (int rc = each_ctx(m, "s2d_set_adam", [&](s2d_ctx* c) { return s2d_set_adam(c, full.data(), b1, b2, it); })) return rc;
    }
    if (int rc = each_ctx(m, "s2d_set_splats", [&](s2d_ctx* c) { return s2d_set_splats(c, splats); })) return rc;
    m->hold_valid = false;
    return S2D_OK;
}

int s2d_multi_get_splats(s2d_multi* m, s2d_splat* splats)
{
    if (!m || (!splats && m->n)) return S2D_E_INVALID;
    DeviceGuard guard;
    if (m->scheme == SCHEME_OWNERSHIP && m->hold_valid)
        return assemble_splats(m, splats);
    s2d_ctx* first = m->ranks[0].ctx;
    if (int rc = s2d_get_splats(first, splats)) return mfail(m, rc, "s2d_get_splats: %s", s2d_last_error(first));
    return S2D_OK; // the replicas are bit-identical: any one of them
}

int s2d_multi_set_adam(s2d_multi* m, const s2d_splat_adam* adams, float beta1t, float beta2t, int32_t iterations)
{
    if (!m || (!adams && m->n) || iterations < 0) return S2D_E_INVALID;
    DeviceGuard guard;
    // complete on every rank; hold sets unaffected
    if (int rc = each_ctx(m, "s2d_set_adam", [&](s2d_ctx* c) { return s2d_set_adam(c, adams, beta1t, beta2t, iterations); })) return rc;
    m->iterations = iterations;
    state_set_afresh(m); // every rank's counters are alike again (the caller sets the splats as well: include/splat2d.h)
    return S2D_OK;
}

int s2d_multi_step(s2d_multi* m, int32_t iters, uint32_t flags, double* mse_out)
{
    if (!m || iters < 0 || iters > (1 << 16)) return S2D_E_INVALID;
    if (int rc = refuse(m, Health::Usable)) return rc;
    DeviceGuard guard;
    if (int rc = ensure_hold(m)) return rc;
    run_command(m, CMD_STEP, iters, flags, m->iterations);
    if (int rc = first_failure(m, "s2d_multi_step")) {
        // Where the run stands now: a non-finite stop winds the counters of the rank that holds the splat back to the
        // failing iteration (s2d_sequence.hip judge_status); with slab ownership the other ranks did not see it and are ahead.
        // The earliest count is the iteration at which the reference abort()ed; the state is for inspection only, and
        // s2d_multi_set_adam (which sets every rank's counters alike) comes before any further step.
        int32_t earliest = INT32_MAX;
        for (const Rank& R : m->ranks) {
            int32_t it = 0;
            if (s2d_get_adam(R.ctx, nullptr, nullptr, nullptr, &it) == S2D_OK) earliest = std::min(earliest, it);
        }
        if (earliest != INT32_MAX) m->iterations = earliest;
        worsen(m, m->collective_lost.load() || m->timed_out.load() ? Health::Dead : Health::NeedsState);
        return rc;
    }
    m->iterations += iters;
    m->hold_age += iters;
    if (mse_out)
        for (int k = 0; k < iters; k++) {
            double sum = 0.0;
            for (const Rank& R : m->ranks) sum += R.sqerr[(size_t)k]; // slab order: a fixed order
            mse_out[k] = sum / m->mse_norm; // main.cpp:805
        }
    return S2D_OK;
}

int s2d_multi_forward(s2d_multi* m)
{
    if (!m) return S2D_E_INVALID;
    if (int rc = refuse(m, Health::NeedsState)) return rc;
    DeviceGuard guard;
    // slab ownership: after set_splats / init_splats the hold sets (and with them each context's list of the splats it
    // projects and rasterises) are stale until they are made afresh -- a splat that now reaches a rank's rows but was not
    // in its old set would be missing from that slab of the image
    if (int rc = ensure_hold(m)) return rc;
    run_command(m, CMD_FORWARD);
    return first_failure(m, "s2d_multi_forward");
}

int s2d_multi_get_image(s2d_multi* m, float* rgba32f)
{
    if (!m || !rgba32f) return S2D_E_INVALID;
    DeviceGuard guard;
    // every context holds (and returns) its own rows; together they tile the image
    const size_t row = (size_t)m->W * 4;
    for (const Rank& R : m->ranks)
        if (int rc = s2d_get_image_rows(R.ctx, rgba32f + row * (size_t)R.row_begin))
            return mfail(m, rc, "s2d_get_image_rows on rank %d: %s", R.index, s2d_last_error(R.ctx));
    return S2D_OK;
}

} // extern "C"
