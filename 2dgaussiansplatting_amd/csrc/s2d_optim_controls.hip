// s2d_optim_controls.hip -- the Adam launch under the optimiser controls (s2d_set_optim, s2d_set_frozen): the second
// instantiation of the step, a sibling of adam_kernel (s2d_optim.hip) over the same helpers (s2d_adam.h).
#include "s2d_adam.h"

namespace s2d {

// adam_kernel (s2d_optim.hip: read its comments first; the text below is that kernel's, with what follows added), with a
// rate per scalar -- the nine of this iteration, resolved by the host, uniform kernel arguments -- and `frozen` (n bytes by
// splat id, or nullptr), which names the splats the step does not exist for.  A frozen record is never live: its
// parameters, moments and dormant byte stay as they are, the finite guard does not see it, its words on a line shared with
// a live neighbour go back as they came, and only its gradient record is re-zeroed.
__global__ __launch_bounds__(256) void adam_controls_kernel(float* __restrict__ splats, float* __restrict__ adams,
                                                            float* __restrict__ grads, const uint32_t* __restrict__ held_ids,
                                                            const uint32_t* __restrict__ held_count, int n, Geometry g,
                                                            float beta1t, float beta2t, AdamRates lr, int mode, int iteration,
                                                            DeviceStatus* __restrict__ status, ProjRec* __restrict__ proj,
                                                            const TileRect* __restrict__ rects, int check_stamp,
                                                            int* __restrict__ host_stamp, uint8_t* __restrict__ dormant, SqerrJob sq,
                                                            int compact, int proj_current, const uint8_t* __restrict__ frozen)
{
    __shared__ __attribute__((aligned(16))) float buf[256 * 18];
    __shared__ uint32_t s_idbuf[256];
    __shared__ uint64_t s_live_words[4];
    if (!adam_prologue(status, iteration, sq)) return;
    // (asked for here, beside the word the prologue has just read, and not where it is used: behind the gradients)
    const int last_failed_check = __hip_atomic_load(&status->rebin_needed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int total = held_ids ? (int)min(*held_count, (uint32_t)n) : n;
    const int base = blockIdx.x * 256, cnt = min(256, total - base), t = threadIdx.x;
    if (cnt <= 0) return;
    const bool mine = t < cnt;
    const uint32_t* s_ids = nullptr;
    int i = base + t;
    if (held_ids) { // only the splats this rank holds, from their compact list
        if (mine) {
            i = (int)held_ids[base + t];
            s_idbuf[t] = (uint32_t)i;
        }
        s_ids = s_idbuf;
        __syncthreads();
    }
    // compact: record base + t of `splats` / `adams` IS splat ids[t]'s (the rank's held splats in a compact array of their
    // own: whole lines, like the all-splats case); the gradient records stay where the raster kernels' atomics put them
    const uint32_t* const s_ids_state = compact ? nullptr : s_ids;
    float v[9], mv[18], gr[9];
    const bool asleep = mine && dormant != nullptr && dormant[i] != 0; // (in flight together with the gradients)
    const bool frz = mine && frozen != nullptr && frozen[i] != 0; // (and so is the frozen byte)
    // gradients in
    const uint32_t grads_nonzero = grads_fill(buf, grads, s_ids, base, cnt);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; k++) gr[k] = mine ? buf[t * 9 + k] : 0.0f;
    // which records are INERT, and when none may be skipped (may_skip): adam_kernel
    const bool may_skip = proj == nullptr || (proj_current != 0 && last_failed_check != check_stamp - 1);
    bool live = false;
    if (mine && !frz) {
#pragma unroll
        for (int k = 0; k < 9; k++) live = live || (f32_bits(gr[k]) != 0u);
        if (!live) live = !may_skip || !asleep;
    }
    // A frozen record is moved only where its projection record is not known current: it then passes through unchanged
    // (`live` for the lines and the projection, no update), as an inert one does there.
    if (frz) live = proj != nullptr && !may_skip;
    const uint64_t wave_live = __ballot(live);
    if ((t & 63) == 0) s_live_words[t >> 6] = wave_live;
    if (!__syncthreads_or(live)) {
        // An all-inert block has all-+0 gradients and nothing to store -- but a block of FROZEN splats has real ones, which
        // the next backward pass would add to: they are re-zeroed before the block leaves.
        grads_rezero(grads, s_ids, base, cnt, grads_nonzero);
        return;
    }
    const int inert_records = cnt - (__popcll(s_live_words[0]) + __popcll(s_live_words[1]) + __popcll(s_live_words[2]) + __popcll(s_live_words[3]));
    const uint64_t* const s_live = __builtin_amdgcn_readfirstlane(inert_records) == 0 ? nullptr : s_live_words;
    // zeros out, over the words that are not +0 already
    grads_rezero(grads, s_ids, base, cnt, grads_nonzero);
    // parameters in.  Every thread keeps its record's words, whichever of them were loaded: the copy is overwritten by the
    // moments below, and an inert record's words on a line it shares with a live one have to go back with that line.
    lds_fill<9>(buf, splats, s_ids_state, s_live, base, cnt);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = mine ? buf[t * 9 + k] : 0.0f;
    __syncthreads();
    // moments in
    lds_fill<18>(buf, adams, s_ids_state, s_live, base, cnt);
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 18; k++) mv[k] = buf[t * 18 + k];
        if (!frz) adam_update_one(v, mv, gr, g.W, g.H, beta1t, beta2t, lr, mode, iteration, status);
        if (dormant && !frz) { // all eighteen moments +0: the next +0 gradient changes nothing
            uint32_t any = 0u;
#pragma unroll
            for (int k = 0; k < 18; k++) any |= f32_bits(mv[k]);
            dormant[i] = any == 0u ? 1 : 0;
        }
        // moments out (each thread rewrites only its own record of the block's copy; the opacity slot goes back
        // unchanged when the checkbox is off)
#pragma unroll
        for (int k = 0; k < 18; k++) buf[t * 18 + k] = mv[k];
    }
    __syncthreads();
    lds_drain<18>(adams, buf, s_ids_state, s_live, base, cnt);
    __syncthreads();
    // parameters out
    if (mine) {
#pragma unroll
        for (int k = 0; k < 9; k++) buf[t * 9 + k] = v[k];
    }
    __syncthreads();
    lds_drain<9>(splats, buf, s_ids_state, s_live, base, cnt);
    if (proj && live) project_updated(v, i, g, status, proj, rects, check_stamp, host_stamp);
}

hipError_t launch_adam_controls(const AdamArgs& a, hipStream_t stream)
{
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_controls_kernel, dim3((a.n + 255) / 256), dim3(256), 0, stream, a.splats, a.adams, a.grads,
                       a.held_ids, a.held_count, a.n, a.g, a.beta1t, a.beta2t, a.rates, a.mode, a.iteration, a.check.status,
                       a.proj, (const TileRect*)a.check.rects, a.check.stamp, a.check.host_stamp, a.dormant, a.sq,
                       (a.compact && a.held_ids) ? 1 : 0, a.proj_current ? 1 : 0, a.frozen);
    return hipGetLastError();
}

} // namespace s2d
