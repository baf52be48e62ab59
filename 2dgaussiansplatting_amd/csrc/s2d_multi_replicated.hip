// s2d_multi_replicated.hip -- replicated state of the multi-device handle (S2D_MULTI_REPLICATED; s2d_multi.h): RCCL
// loaded at run time, one communicator per rank, the all-reduce of an iteration's gradients -- through RCCL, or through
// pinned host memory when the ranks share a GPU.
#include "s2d_multi.h"

#include <dlfcn.h>

namespace s2d {
namespace multi {

namespace {

bool load_rccl(Rccl* r, std::string* why)
{
    static std::mutex m;
    static Rccl cached;
    std::lock_guard<std::mutex> lk(m);
    if (!cached.lib) {
        // One RCCL per process, on the process's one HIP runtime: first an image that is already
        // mapped -- PyTorch's wheel bundles RCCL as torch/lib/librccl.so with SONAME librccl.so.1, and a process that has
        // imported torch must not get the system's copy beside it -- and only then a load by name (the system's librccl.so.1
        // needs libamdhip64.so.7, which binds to whichever runtime the process already has, by SONAME).
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            cached.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
            if (cached.lib) break;
        }
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            if (cached.lib) break;
            cached.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        }
        if (!cached.lib) {
            *why = std::string("cannot load librccl: ") + dlerror();
            return false;
        }
        cached.CommInitAll = (decltype(cached.CommInitAll))dlsym(cached.lib, "ncclCommInitAll");
        cached.CommDestroy = (decltype(cached.CommDestroy))dlsym(cached.lib, "ncclCommDestroy");
        cached.CommAbort = (decltype(cached.CommAbort))dlsym(cached.lib, "ncclCommAbort");
        cached.AllReduce = (decltype(cached.AllReduce))dlsym(cached.lib, "ncclAllReduce");
        cached.GetErrorString = (decltype(cached.GetErrorString))dlsym(cached.lib, "ncclGetErrorString");
        if (!cached.CommInitAll || !cached.CommDestroy || !cached.AllReduce || !cached.GetErrorString) {
            *why = "librccl lacks ncclCommInitAll / ncclAllReduce";
            cached.lib = nullptr;
            return false;
        }
    }
    *r = cached;
    return true;
}

// One communicator per rank, one rank per GPU.
int create_communicators(s2d_multi* m)
{
    std::string why;
    if (!load_rccl(&m->rccl, &why)) return mfail(m, S2D_E_HIP, "%s", why.c_str());
    std::vector<int> devs;
    for (const Rank& R : m->ranks) devs.push_back(R.device);
    std::vector<ncclComm_t> made((size_t)m->world, nullptr);
    const ncclResult_t nrc = m->rccl.CommInitAll(made.data(), m->world, devs.data());
    if (nrc != ncclSuccess)
        return mfail(m, S2D_E_HIP, "ncclCommInitAll over %d devices: %s (RCCL takes one rank per GPU; S2D_MULTI_SHARE_GPU rehearses "
                                   "on fewer)", m->world, m->rccl.GetErrorString(nrc));
    for (Rank& R : m->ranks) R.comm.store(made[(size_t)R.index]);
    return S2D_OK;
}

// The staging buffers of staged_all_reduce: every rank's pinned copy of its partial gradients.
int alloc_staging(s2d_multi* m)
{
    if (hipSetDevice(m->ranks[0].device) != hipSuccess) return mfail(m, S2D_E_HIP, "hipSetDevice(%d)", m->ranks[0].device);
    for (Rank& R : m->ranks)
        if (R.staging.alloc((size_t)m->n * 9 + 4, hipHostMallocDefault) != hipSuccess)
            return mfail(m, S2D_E_NOMEM, "host staging buffers for %d ranks", m->world);
    return S2D_OK;
}

// The sum RCCL would form, through host memory (S2D_MULTI_SHARE_GPU): every rank copies its partial gradients out,
// rank 0 adds them in rank order, every rank copies the sum back in.
int staged_all_reduce(s2d_multi* m, Rank& R, float* grads, size_t count)
{
    hipStream_t stream = R.stream();
    float* sum = m->ranks[0].staging;
    MHIP(R, hipMemcpyAsync(R.staging, grads, count * sizeof(float), hipMemcpyDeviceToHost, stream));
    if (int rc = drain_now(m, R, "copying its gradients out for the staged all-reduce")) return rc;
    if (int rc = meet_rank(m, R, "staged all-reduce (partials out)")) return rc;
    if (R.index == 0)
        for (int q = 1; q < m->world; q++) {
            const float* src = m->ranks[(size_t)q].staging;
            for (size_t k = 0; k < count; k++) sum[k] += src[k];
        }
    if (int rc = meet_rank(m, R, "staged all-reduce (sum formed)")) return rc;
    MHIP(R, hipMemcpyAsync(grads, sum, count * sizeof(float), hipMemcpyHostToDevice, stream));
    if (int rc = drain_now(m, R, "copying the summed gradients in")) return rc;
    return meet_rank(m, R, "staged all-reduce (sum read)"); // nobody overwrites its host copy before everybody has read the sum
}

} // namespace

int set_up_replicated(s2d_multi* m)
{
    if (!m->share_gpu) return create_communicators(m);
    return m->world > 1 ? alloc_staging(m) : S2D_OK;
}

// s2d_multi_destroy, with the workers gone: whoever empties a slot frees what it held (abort_collective).
void destroy_communicator(s2d_multi* m, Rank& R)
{
    if (const ncclComm_t c = R.comm.exchange(nullptr)) m->rccl.CommDestroy(c);
}

// The all-reduce of one iteration's gradients, between s2d_forward_backward and s2d_adam_step (a handle on one device
// goes through RCCL too: same code whatever N).
int all_reduce_grads(s2d_multi* m, Rank& R)
{
    float* grads = (float*)s2d_grads_device_ptr(R.ctx);
    const size_t count = (size_t)m->n * 9;
    if (m->share_gpu) return m->world > 1 ? staged_all_reduce(m, R, grads, count) : S2D_OK;
    if (m->comms_aborted.load()) { // a stop was published (the barrier breaks a moment later): not this rank's failure
        abort_collective(m, R);
        return kStopped;
    }
    const ncclComm_t comm = R.comm.load();
    if (!comm) return rank_fail(R, S2D_E_STATE, "no communicator");
    if (m->rccl.AllReduce(grads, grads, count, ncclFloat, ncclSum, comm, R.stream()) != ncclSuccess) return rank_fail(R, S2D_E_HIP, "ncclAllReduce failed");
    return S2D_OK;
}

} // namespace multi
} // namespace s2d
