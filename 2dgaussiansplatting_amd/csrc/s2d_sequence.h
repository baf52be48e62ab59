// s2d_sequence.h -- what the entry-point units (s2d_api*.hip) call of the sequencing of one iteration (s2d_sequence.hip):
// the passes, the step loop, the status word, and the events that make derived state stale.
//
// What is current: three things are derived from the parameters, each from the one before -- the projection with its
// containment check, the tile lists, and the frames (image0 and the gradients); the target stands beside them.  Freshness
// keeps the five flags.  Whoever PRODUCES one of them says so with a setter, and all producers are in s2d_sequence.hip
// (rebuild_lists, queue_raster, queue_adam, backward_queued, target_replaced).  Everything else names an EVENT, one of
// the functions at the end of this file, which does all that the event asks for: the flags, SplatState::written(), the
// status word.  Outside s2d_sequence.hip nothing calls invalidate() or a production setter; the other units read the
// getters and call events.
#pragma once

#include <climits>

#include "../../include/splat2d.h"
#include "s2d_device.h"
#include "s2d_loss.h"
#include "s2d_owned.h"
#include "s2d_state.h"

// What an event reaches: Frames < Projection < Lists, a level with everything below it.
enum class Stale { Frames, Projection, Lists };

class S2D_LOCAL Freshness {
public:
    bool target() const { return target_; }         // imageRef holds a target
    bool forward() const { return forward_; }       // image0 holds the framebuffer of the CURRENT parameters
    bool backward() const { return backward_; }     // ... and the gradient buffer their gradients
    bool projection() const { return projection_; } // surface.proj() and d_status->rebin_needed describe the CURRENT parameters
    bool lists() const { return lists_; }           // the tile lists are the scene's, built from the held splats
    void invalidate(Stale reach)
    {
        forward_ = backward_ = false;
        if (reach >= Stale::Projection) projection_ = false;
        if (reach >= Stale::Lists) lists_ = false;
    }
    void target_set() { target_ = true; }
    void lists_in_the_making() { lists_ = false; } // (a build writes into the buffers the lists lie in from its first launch on)
    void lists_built(bool of_the_scene) { lists_ = of_the_scene; } // a range's lists are walked once and replaced by the next range's
    void projected() { projection_ = true; }
    void frame_stored(bool image0) { forward_ = image0, backward_ = false; } // a raster pass is queued
    void backward_queued() { backward_ = true; }

private:
    bool target_ = false, forward_ = false, backward_ = false, projection_ = false, lists_ = false;
};

constexpr s2d::DeviceStatus kFreshStatus{0, INT_MAX, 0, 0}; // rebin_needed 0 matches no check (sequence numbers start at 1)

// ---- passes (each queues on the context's stream; the context's device is current) -----------------------------------
// Room for `need` pairs in the training image's lists and scratch, or the context's error (s2d_create asks for the first).
S2D_LOCAL int ensure_pair_capacity(s2d_ctx* c, uint64_t need);
S2D_LOCAL int queue_forward(s2d_ctx* c);
// upstream != nullptr: the walk starts from that dL/d(image0) instead of image0 - imageRef, and no squared error is
// formed or queued.  density: the walk also accumulates the density statistics (parse_walk_flags() has admitted it).
S2D_LOCAL int queue_backward(s2d_ctx* c, bool need_opacity_grad, const float4* upstream = nullptr, bool density = false);
S2D_LOCAL int queue_forward_backward(s2d_ctx* c, bool need_opacity_grad, bool write_image);
S2D_LOCAL int queue_adam(s2d_ctx* c, uint32_t flags);
// A backward pass of the current iteration has been queued; `by`: what becomes of its squared error.
S2D_LOCAL int backward_queued(s2d_ctx* c, s2d::SqerrBy by);

// What the flags of a backward pass (S2D_BWD_*) or of a step (step: S2D_STEP_*) ask of the backward walk.
struct WalkFlags {
    bool need_opacity_grad = true;
    bool density = false;
};
S2D_LOCAL int parse_walk_flags(s2d_ctx* c, uint32_t flags, bool step, WalkFlags* out);

// s2d_step (loss == nullptr) and s2d_step_loss.  The loss passes of the latter are s2d_api_loss.hip's:
S2D_LOCAL int run_steps(s2d_ctx* c, int iters, uint32_t flags, const s2d_loss_config* loss, double* loss_out, double* mse_out);
S2D_LOCAL int queue_loss_backward(s2d_ctx* c, const s2d_loss_config* cfg, bool need_opacity_grad, bool density);
// The ring the context's loss passes write now (the four totals under a pixel-weight plane, the three without), and the terms
// of one entry of it (weighted_mse: the mean the total counts, which under a plane is not t.mse).
S2D_LOCAL const s2d::TermRing& current_ring(const s2d_ctx* c);
S2D_LOCAL s2d_loss_terms loss_terms_of(const s2d_ctx* c, int terms, const double* sums, const float* w,
                                       double* weighted_mse = nullptr);
// Under a pixel-weight plane (include/splat2d_weights.h; s2d_api_loss.hip): what the context refuses a plane for, and the backward
// pass of s2d_backward / s2d_step (the weighted loss pass with weights (1, 0, 0), then the walk).
S2D_LOCAL int weights_refused_by_context(s2d_ctx* c, const char* who);
S2D_LOCAL int queue_weighted_backward(s2d_ctx* c, bool need_opacity_grad, bool density);

S2D_LOCAL int queue_status_read(s2d_ctx* c); // -> h_status, valid once the stream has been synchronised
S2D_LOCAL int check_status(s2d_ctx* c);      // ... read, waited for and judged

// ---- events -----------------------------------------------------------------------------------------------------------
// ("Adam step queued" and "non-finite step judged" are queue_adam's and judge_status's own.)
S2D_LOCAL void target_replaced(s2d_ctx* c);                 // s2d_set_target, _synthetic
S2D_LOCAL void backdrop_replaced(s2d_ctx* c);               // s2d_set_backdrop, _device: set, replaced or removed
S2D_LOCAL void weights_replaced(s2d_ctx* c);                // s2d_set_pixel_weights, _device: set, replaced or removed
S2D_LOCAL int splats_replaced(s2d_ctx* c);                  // s2d_init_splats, s2d_set_splats
S2D_LOCAL int splats_replaced_from_device(s2d_ctx* c);      // s2d_set_splats_device
S2D_LOCAL int rows_replaced(s2d_ctx* c, int32_t what);      // S2D_ROWS_*: s2d_rows_scatter; s2d_relocate and the seeding write S2D_ROWS_SPLATS (with their moments)
S2D_LOCAL int moments_replaced(s2d_ctx* c);                 // s2d_set_adam
S2D_LOCAL void held_set_changed(s2d_ctx* c, bool had, bool has, bool added); // s2d_halo_commit
S2D_LOCAL void alive_set_changed(s2d_ctx* c);               // s2d_set_alive, s2d_prune, s2d_grow, s2d_init_splats over a set
