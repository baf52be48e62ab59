// splat2d_train.cpp -- headless C++ host loop on top of the C ABI (include/splat2d.h).
//
// Mirrors the shape of the reference's main() (/root/reference/main.cpp:236-856) without its window:
//   load imageRef (main.cpp:253-259)  ->  NSplat splats (:271-272)  ->  init() (:280-307)  ->
//   loop { forward (:414-546); backward (:548-712); Adam + constraints (:714-785); MSE (:796-805);
//          printf("%d itr, mse %.4f\n") (:807); iterations++ (:809) }
// The three passes run on the MI355X through s2d_step(); this file owns only what main() owns besides them:
// the image, the flags the GUI exposed ("Optimize opacity" :825, "Restart" :828-831) and the trace line.
// It is plain C++ (g++), links the library, and has no compute of its own.
//
//   splat2d_train --image tests/golden/squirrel_cls_mini_268x213.s2di --splats 1024 --iters 300
//   splat2d_train --synthetic 4096x4096 --splats 1000000 --iters 100 --quiet
//   splat2d_train --synthetic 4096x4096 --splats 1000000 --iters 100 --quiet --gpus 8
//
// --gpus N: the same loop, with every option, on a multi-device handle (s2d_multi_*): the image cut
// into N row slabs, one context per GPU, and between the backward pass and the Adam step either the holders of a
// boundary splat swap its gradient rows by peer-to-peer copies (slab ownership, default) or RCCL all-reduces all
// N x 9 gradients over xGMI (--exchange dense, north_star's scheme) -- all inside the library.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "image_io.h"
#include "overlay.h"
#include "splat2d.h"
#include "splat2d_backdrop.h"
#include "splat2d_weights.h"
#include "splat2d_coarse.h"

namespace {

struct Options {
    std::string image;          // .s2di fixture (raw RGB8, see tools/make_image_fixtures.py), binary .ppm or .png
    int syn_w = 0, syn_h = 0;   // --synthetic WxH
    int n_splats = 1024;        // NSplat, main.cpp:271
    int iters = 300;
    int batch = 1;              // iterations queued per s2d_step call (1 = print after every iteration, like the reference)
    bool optimize_opacity = false;
    int opacity_from = 0;       // iteration from which the flag is on (the GUI checkbox can be ticked mid-run)
    int restart_at = -1;        // press "Restart" before this iteration (main.cpp:828-831)
    bool quiet = false;
    std::string out_image;      // --out-image file.(png|ppm|s2di): image0 after the last iteration (main.cpp:794)
    // View of the final splats instead of image0 (include/splat2d.h "view rendering"; one context only): with any of the four
    // options --out-image is the RGBA8 view.  Defaults: the image's own size, origin 0,0, zoom 1, one sample, no filter; the
    // filter's default is PROVISIONAL: nothing is claimed about the picture it gives.
    bool have_view = false;
    int view_w = 0, view_h = 0;           // --out-size WxH (0: the image's)
    float view_x = 0.0f, view_y = 0.0f, view_zoom = 1.0f; // --out-view X,Y,ZOOM
    int view_samples = 1;                 // --out-samples S: 1, 2 or 4 per axis
    float view_filter = 0.0f;             // --out-filter F: variance of the low-pass in output pixels^2
    std::string overlay;        // --overlay file: image0 upscaled by overlay_scale with the splat debug drawing (main.cpp:441-485)
    int overlay_scale = 2;      // viewScale, main.cpp:822
    int overlay_stride = 1;     // draw every k-th splat
    std::string overlay_dump;   // --overlay-vertices file: the pr::PrimVertex list of main.cpp:447-476 as drawn (binary, see below)
    std::string convert_in, convert_out; // --convert in out: image conversion only (no GPU)
    std::string load_ckpt, save_ckpt; // the five objects of main.cpp:272-278: splats, splatAdams, beta1t, beta2t, iterations
    int device = 0;
    int rebin_interval = 0;
    float lr = 0.0f;            // --lr: trainingRate, main.cpp:715 (0 = the reference's 0.05)
    bool deterministic = false; // --deterministic: bitwise reproducible gradient sums (S2D_CFG_DETERMINISTIC)
    bool reference_order = false; // --reference-order: gradients, state and trace bytes-equal to the reference's (S2D_CFG_REFERENCE_ORDER)
    int stall_ms = -1;          // --stall-timeout-ms (multi-device handle): how long a rank may not answer before the step fails
    int gpus = 1;               // --gpus N: devices device .. device + N - 1, one row slab each, RCCL all-reduce of the gradients
    bool share_gpu = false;     // --share-gpu: all N ranks on --device (rehearsal on a box with fewer GPUs than ranks)
    // Density control (include/splat2d.h "density control"; one context only).  The defaults of the window, the fraction and
    // the weight are PROVISIONAL: nobody has measured them yet.
    int relocate_every = 0;          // --relocate-every K: s2d_relocate before iteration K, 2K, ... (0: never, the reference's loop)
    int relocate_window = 10;        // --relocate-window S: the last S iterations before each relocation gather the statistics
    float relocate_max_fraction = 0.05f; // --relocate-max-fraction f: at most f * splats moved per relocation
    float relocate_min_weight = 0.5f;    // --relocate-min-weight w: a splat whose sum of T * alpha per pass is below w is starved
    // Importance-sampled placement (include/splat2d.h "importance-sampled placement"; one context only).
    std::string seed_init;           // --seed-init edges|uniform: init() followed by s2d_seed_splats over all rows -- positions drawn
                                     // from the target's edge map (edges) or from that map under the full uniform share, floor 4095,
                                     // where no pixel is more than twice as likely as another (uniform); colours from the target
    // --reseed-every K: s2d_reseed before iteration K, 2K, ...: the starved splats are drawn again from the squared error map.
    // Shaped like the relocation options, and like theirs the defaults are PROVISIONAL until someone sweeps them (DESIGN.md
    // section 14): they are the one configuration that section measured.
    int reseed_every = 0;
    int reseed_window = 10;              // --reseed-window S: the last S iterations before each pass gather the statistics
    float reseed_max_fraction = 0.1f;    // --reseed-max-fraction f: at most f * splats written per pass
    float reseed_min_weight = 5.0f;      // --reseed-min-weight w: a splat whose sum of T * alpha per pass is below w is starved
    float reseed_scale = 3.0f;           // --reseed-scale x: sx = sy of the rows written (0: sqrt(W H / splats))
    // The alive set (include/splat2d.h "the alive set"; one context only): --splats is the capacity.  The defaults of the
    // count, the scale, the window and the weight are PROVISIONAL: nobody has measured them yet.
    int alive_from = -1;             // --alive-from K0: after init() / --seed-init only the LAST K0 rows are alive (-1: all)
    int grow_every = 0;              // --grow-every M: s2d_grow before iteration M, 2M, ... from the squared error map, while a row is dead
    int grow_count = 0;              // --grow-count C: rows brought to life per event
    float grow_scale = 3.0f;         // --grow-scale X: sx = sy of the rows written (0: sqrt(W H / splats))
    int prune_every = 0;             // --prune-every K: s2d_prune before iteration K, 2K, ...
    float prune_min_weight = 0.5f;   // --prune-min-weight W: an alive row whose sum of T * alpha per pass is below W dies
    int prune_window = 10;           // --prune-window S: the last S iterations before each pruning gather the statistics
    // --loss-weights M,L,D: train with L = sum of M * d^2 / 2 + L * |d| + D * (1 - SSIM) (include/splat2d.h "image losses"; one
    // context only) instead of the reference's squared error; the trace line gains ", loss %.6f"
    bool have_loss = false;
    s2d_loss_config loss{};
    // Optimiser controls (include/splat2d.h "optimiser controls"; one context only).  All defaults leave the plain launch.
    bool have_lr_groups = false;     // --lr-groups P,S,R,C,O: a rate per parameter group (pos, scale, rot, colour, opacity)
    float lr_groups[5] = {0, 0, 0, 0, 0};
    bool have_lr_ratio = false;      // --lr-final-ratio P,S,R,C,O: each rate decays log-linearly to rate * ratio (0 or 1: not) ...
    float lr_ratio[5] = {0, 0, 0, 0, 0};
    int lr_decay_iters = 0;          // --lr-decay-iters T: ... over the first T iterations (groups not named by --lr-groups: --lr)
    float rebin_margin = 0.0f;       // --rebin-margin PX: s2d_config.rebin_margin (0: the library's 2 pixels)
    bool freeze_unmoved = false;     // --freeze-unmoved: after each --reseed-every / --relocate-every event only the rows it wrote
                                     // are trained until the next event (s2d_set_frozen)
    // --coverage: a coverage context (S2D_CFG_COVERAGE).  The target is the file's colour premultiplied by its alpha with .w =
    // alpha (a file without alpha, or --synthetic: alpha 1); --out-image is written as an RGBA8 PNG with straight alpha, rgb / A
    // where A > 0, otherwise 0.  One context only, the squared error only, and nothing that needs the density statistics.
    bool coverage = false;
    // --coarse Z:K[,Z:K...]: coarse-to-fine (splat2d_coarse.h).  Stage s runs K_s iterations of s2d_step_view on the whole image
    // at zoom Z_s -- output ceil(W Z) x ceil(H Z), origin 0, the library's own resampled target -- and prints the view's MSE in
    // the reference's trace line; the stages cover iterations 0 .. sum K - 1 of the run (they count towards --iters, and a
    // checkpoint loaded inside a stage continues it), s2d_view_release follows the last, the rest runs at full size as ever.
    // --coarse-samples S: samples per axis of the views (1, 2 or 4).  One context, the squared error, and nothing that gathers
    // density statistics.  The schedule has no defaults worth the name: which zooms and how long is provisional.
    std::vector<std::pair<float, int>> coarse;
    bool coarse_malformed = false;
    int coarse_samples = 1;
    // --background R,G,B: a constant backdrop (splat2d_backdrop.h): the splats are drawn and trained over that colour, and
    // --out-image, --out-size and --out-view include it.  One context; a checkpoint does not carry it.
    bool have_background = false, background_malformed = false;
    float background[3] = {0, 0, 0};
    // --weight-image PATH [--weight-gain G]: a pixel-weight plane (splat2d_weights.h) from the first channel of an image of the
    // target's size: omega = channel / 255 (a mask), or with the gain omega = 1 + G * channel / 255 (an emphasis).  One context;
    // a checkpoint does not carry it.  The gain's form is provisional.
    std::string weight_image;
    bool have_weight_gain = false, weight_gain_malformed = false;
    float weight_gain = 0.0f;
    bool replicated = false;    // --exchange dense: replicated state + RCCL all-reduce of all gradients (default: slab ownership)
                                // (RCCL takes one rank per GPU): a rehearsal of the N-rank host logic on a box with fewer GPUs
};

// Checkpoint = the state main() keeps between frames (main.cpp:272-278), in the reference's own layouts.
struct CkptHeader {
    char magic[4];      // "S2DC"
    uint32_t n_splats, width, height;
    float beta1t, beta2t;
    int32_t iterations;
};

int usage()
{
    std::fprintf(stderr,
                 "usage: splat2d_train (--image file.s2di|.ppm|.png|.jpg | --synthetic WxH) [--splats N] [--iters K] [--batch B]\n"
                 "                     [--optimize-opacity [--opacity-from IT]] [--restart-at IT] [--out-image file.png|.ppm]\n"
                 "                     [--out-size WxH] [--out-view X,Y,ZOOM] [--out-samples S] [--out-filter F]\n"
                 "                     [--overlay file [--overlay-scale S] [--overlay-stride K] [--overlay-vertices file]]\n"
                 "       splat2d_train --convert in.(s2di|ppm|png|jpg) out.(s2di|ppm|png)\n"
                 "                     [--load-checkpoint file] [--save-checkpoint file]\n"
                 "                     [--lr RATE] [--deterministic] [--reference-order] [--device D] [--gpus N [--exchange halo|dense] [--share-gpu]\n"
                 "                     [--stall-timeout-ms MS]] [--rebin-interval R] [--quiet]\n"
                 "                     [--relocate-every K [--relocate-window S] [--relocate-max-fraction F] [--relocate-min-weight W]]\n"
                 "                     [--loss-weights M,L,D] [--seed-init edges|uniform]\n"
                 "                     [--reseed-every K [--reseed-window S] [--reseed-max-fraction F] [--reseed-min-weight W] [--reseed-scale X]]\n"
                 "                     [--lr-groups P,S,R,C,O [--lr-final-ratio P,S,R,C,O --lr-decay-iters T]] [--rebin-margin PX] [--freeze-unmoved]\n"
                 "                     [--alive-from K0] [--grow-every M --grow-count C [--grow-scale X]]\n"
                 "                     [--prune-every K [--prune-min-weight W] [--prune-window S]] [--coverage]\n"
                 "                     [--background R,G,B] [--weight-image file [--weight-gain G]]\n"
                 "  --loss-weights M,L,D: train with the sum over pixels and channels of M * d^2 / 2 + L * |d| + D * (1 - SSIM), e.g.\n"
                 "    0,0.8,0.2, instead of the reference's squared error (one GPU only); every line ends with the loss's mean.\n"
                 "  --relocate-every K: before iteration K, 2K, ... move the starved splats (summed T * alpha per pass below W) onto\n"
                 "    halves of the splats with the largest summed |dL/dpos|, from statistics of the S iterations before, at most\n"
                 "    F * splats at a time (one GPU only).  Defaults S = 10, F = 0.05, W = 0.5 are provisional: not measured yet.\n");
    std::fprintf(stderr,
                 "  --out-size WxH, --out-view X,Y,ZOOM, --out-samples S, --out-filter F: with any of them --out-image is a view of the\n"
                 "    final splats instead of image0: the window of the source plane whose top-left corner is X,Y at ZOOM output pixels\n"
                 "    per source pixel, W x H pixels, S x S samples per pixel (1, 2 or 4), a low-pass of variance F output pixels^2 on\n"
                 "    the footprints (one GPU only).  Defaults: the image's size, 0,0,1, S = 1, F = 0 (provisional).\n");
    std::fprintf(stderr,
                 "  --seed-init edges|uniform: after init(), draw every splat's position from the target's edge map (uniform: under\n"
                 "    the full uniform share) and take its colour from the target there (one GPU only).\n"
                 "  --reseed-every K: before iteration K, 2K, ... draw the starved splats (summed T * alpha per pass below W) again from\n"
                 "    the squared error map at scale X, from statistics of the S iterations before, at most F * splats at a time (one\n"
                 "    GPU only; not together with --relocate-every).  Defaults S = 10, F = 0.1, W = 5, X = 3 are provisional.\n");
    std::fprintf(stderr,
                 "  --lr-groups P,S,R,C,O: Adam rates of position, scale, rotation, colour and opacity instead of the one --lr, e.g.\n"
                 "    0.5,0.2,0.1,0.05,0.05; with --lr-final-ratio and --lr-decay-iters T each decays log-linearly to rate * ratio over\n"
                 "    the first T iterations (one GPU only).  --rebin-margin PX: the margin of the re-used tile lists (default 2 pixels).\n"
                 "  --freeze-unmoved: after each reseeding / relocation only the rows it wrote are trained until the next one.\n");
    std::fprintf(stderr,
                 "  --alive-from K0: --splats is the capacity; after init() (or --seed-init, which then seeds only those) the last K0\n"
                 "    rows are alive.  --grow-every M --grow-count C: before iteration M, 2M, ... bring the C dead rows of lowest index\n"
                 "    to life, drawn from the squared error map at scale X, until no row is dead.  --prune-every K: before iteration\n"
                 "    K, 2K, ... alive rows whose summed T * alpha per pass is below W die, from statistics of the S iterations before\n"
                 "    (not together with --relocate-every / --reseed-every).  One GPU only, not with --reference-order, and not with\n"
                 "    --save-checkpoint / --load-checkpoint: the checkpoint format does not carry the set.  Defaults X = 3, W = 0.5,\n"
                 "    S = 10 are provisional: not measured yet.\n");
    std::fprintf(stderr,
                 "  --coverage: fit the image's alpha as well (a cut-out, a sprite, a layer): the target is the file's colour times its\n"
                 "    alpha, with the alpha as a fourth channel; --out-image file.png is written as RGBA with straight alpha.  One GPU\n"
                 "    only; not with --loss-weights, --reference-order, --relocate-every, --reseed-every or --prune-every.\n");
    std::fprintf(stderr,
                 "  --coarse Z:K[,Z:K...] [--coarse-samples S]: coarse-to-fine, e.g. --coarse 0.25:100,0.5:100 --iters 500: the first K\n"
                 "    iterations train a view of the whole image at zoom Z (ceil(W Z) x ceil(H Z) pixels) against the target resampled to\n"
                 "    that size, then the next stage, then full size; the trace prints the view's MSE.  The stages count towards --iters.\n"
                 "    One GPU only; not with --coverage, --reference-order, --loss-weights or the options that gather density\n"
                 "    statistics (--relocate-every, --reseed-every, --prune-every, --grow-every).  The schedule is provisional.\n");
    std::fprintf(stderr,
                 "  --background R,G,B: draw and train the splats over that colour instead of black, e.g. 1,1,1 for a page or a chart on\n"
                 "    white; --out-image, --out-size and --out-view include it.  One GPU only; not with --coverage, --reference-order or\n"
                 "    --coarse.  A checkpoint does not carry the background: give the option again with --load-checkpoint.\n");
    std::fprintf(stderr,
                 "  --weight-image file [--weight-gain G]: weigh every pixel's loss by a plane taken from the first channel of an image\n"
                 "    of the target's size: channel / 255 (black = ignore the pixel, a mask), or with the gain 1 + G * channel / 255\n"
                 "    (white = G + 1 times as important; provisional).  Every line ends with the weighted loss's mean, wloss; mse stays\n"
                 "    the plain one.  One GPU only; not with --coverage or --coarse.  A checkpoint does not carry the weight plane: give\n"
                 "    the option again with --load-checkpoint.\n");
    return 2;
}

// "R,G,B" -> three finite values; false: malformed (a missing part, trailing characters, a value that is not finite).
bool parse_background(const char* text, float* rgb)
{
    const char* p = text;
    for (int k = 0; k < 3; k++) {
        char* end = nullptr;
        rgb[k] = std::strtof(p, &end);
        if (end == p || !std::isfinite(rgb[k]) || *end != (k < 2 ? ',' : '\0')) return false;
        p = end + 1;
    }
    return true;
}

// "Z:K[,Z:K...]" -> stages; false: malformed (an empty list, a missing part, trailing characters).
bool parse_coarse(const char* text, std::vector<std::pair<float, int>>* out)
{
    out->clear();
    const char* p = text;
    while (true) {
        char* end = nullptr;
        const float z = std::strtof(p, &end);
        if (end == p || *end != ':') return false;
        p = end + 1;
        const long k = std::strtol(p, &end, 10);
        if (end == p) return false;
        out->push_back({z, (int)k});
        if (*end == '\0') return true;
        if (*end != ',') return false;
        p = end + 1;
    }
}

// One context, or a multi-device handle, behind the same calls: what main() below talks to.
struct Session {
    s2d_ctx* ctx = nullptr;
    s2d_multi* multi = nullptr;
    bool is_multi = false;

    const char* last_error() const { return is_multi ? s2d_multi_last_error(multi) : s2d_last_error(ctx); }
    int create(const Options& o, int W, int H)
    {
        s2d_config cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.struct_size = sizeof(cfg);
        cfg.width = W;
        cfg.height = H;
        cfg.n_splats = o.n_splats; // int NSplat = 1024; main.cpp:271
        cfg.rebin_interval = o.rebin_interval;
        cfg.training_rate = o.lr;
        cfg.rebin_margin = o.rebin_margin;
        if (o.deterministic) cfg.flags |= S2D_CFG_DETERMINISTIC;
        if (o.reference_order) cfg.flags |= S2D_CFG_REFERENCE_ORDER;
        if (o.coverage) cfg.flags |= S2D_CFG_COVERAGE;
        is_multi = o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI"); // (the variable sends --gpus 1 through the handle)
        if (!is_multi) {
            cfg.device = o.device;
            return s2d_create(&cfg, &ctx);
        }
        std::vector<int32_t> devs((size_t)o.gpus);
        for (int r = 0; r < o.gpus; r++) devs[(size_t)r] = o.device + (o.share_gpu ? 0 : r);
        return s2d_multi_create(&cfg, devs.data(), o.gpus,
                                (o.share_gpu ? S2D_MULTI_SHARE_GPU : 0u) | (o.replicated ? S2D_MULTI_REPLICATED : 0u), &multi);
    }
    void destroy()
    {
        if (ctx) s2d_destroy(ctx);
        if (multi) s2d_multi_destroy(multi);
        ctx = nullptr;
        multi = nullptr;
    }
    int set_target(const std::vector<float>& rgba)
    {
        if (rgba.empty()) return is_multi ? s2d_multi_set_target_synthetic(multi) : s2d_set_target_synthetic(ctx);
        return is_multi ? s2d_multi_set_target(multi, rgba.data()) : s2d_set_target(ctx, rgba.data());
    }
    int init() { return is_multi ? s2d_multi_init_splats(multi) : s2d_init_splats(ctx); }
    int set_splats(const s2d_splat* p) { return is_multi ? s2d_multi_set_splats(multi, p) : s2d_set_splats(ctx, p); }
    int get_splats(s2d_splat* p) { return is_multi ? s2d_multi_get_splats(multi, p) : s2d_get_splats(ctx, p); }
    int set_adam(const s2d_splat_adam* p, float b1, float b2, int32_t it)
    {
        return is_multi ? s2d_multi_set_adam(multi, p, b1, b2, it) : s2d_set_adam(ctx, p, b1, b2, it);
    }
    int get_adam(s2d_splat_adam* p, float* b1, float* b2, int32_t* it)
    {
        return is_multi ? s2d_multi_get_adam(multi, p, b1, b2, it) : s2d_get_adam(ctx, p, b1, b2, it);
    }
    int step(int iters, uint32_t flags, double* mse) { return is_multi ? s2d_multi_step(multi, iters, flags, mse) : s2d_step(ctx, iters, flags, mse); }
    int forward() { return is_multi ? s2d_multi_forward(multi) : s2d_forward(ctx); }
    int get_image(float* rgba) { return is_multi ? s2d_multi_get_image(multi, rgba) : s2d_get_image(ctx, rgba); }
    // how the devices were kept consistent, for the summary line
    std::string exchange_summary(const Options& o)
    {
        int64_t info[4] = {0, 0, 0, 0};
        if (!is_multi || s2d_multi_exchange_info(multi, info) != S2D_OK) return "";
        char how[240];
        if (info[0] == 2)
            std::snprintf(how, sizeof(how), ", %d ranks: row slabs; replicated state, %s of all gradients", o.gpus,
                          o.share_gpu ? "host-staged sum (ranks share one GPU)" : "RCCL all-reduce");
        else if (info[0] == 1)
            std::snprintf(how, sizeof(how), ", %d ranks: row slabs; slab ownership, %lld gradient rows swapped per iteration by %s, %lld state rows handed over",
                          o.gpus, (long long)info[1], o.share_gpu ? "device copies (ranks share one GPU)" : "peer-to-peer copies", (long long)info[2]);
        else
            std::snprintf(how, sizeof(how), ", %d ranks: one device, nothing to exchange", o.gpus);
        return how;
    }
};

#define CK(call)                                                                        \
    do {                                                                                \
        int rc_ = (call);                                                               \
        if (rc_ != S2D_OK) {                                                            \
            std::fprintf(stderr, "%s -> %d: %s\n", #call, rc_, S.last_error());         \
            S.destroy();                                                                \
            return rc_ == S2D_E_NONFINITE ? 3 : 1; /* the reference abort()s, main.cpp:752-785 */ \
        }                                                                               \
    } while (0)

} // namespace

int main(int argc, char** argv)
{
    Options o;
    bool have_alive_from = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&](const char* what) -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", what); std::exit(2); }
            return argv[++i];
        };
        if (a == "--image") o.image = next("--image");
        else if (a == "--synthetic") { if (std::sscanf(next("--synthetic"), "%dx%d", &o.syn_w, &o.syn_h) != 2) return usage(); }
        else if (a == "--splats") o.n_splats = std::atoi(next("--splats"));
        else if (a == "--iters") o.iters = std::atoi(next("--iters"));
        else if (a == "--batch") o.batch = std::atoi(next("--batch"));
        else if (a == "--optimize-opacity") o.optimize_opacity = true;
        else if (a == "--opacity-from") o.opacity_from = std::atoi(next("--opacity-from"));
        else if (a == "--restart-at") o.restart_at = std::atoi(next("--restart-at"));
        else if (a == "--out-ppm" || a == "--out-image") o.out_image = next("--out-image");
        else if (a == "--out-size") { if (std::sscanf(next("--out-size"), "%dx%d", &o.view_w, &o.view_h) != 2) return usage(); o.have_view = true; }
        else if (a == "--out-view") { if (std::sscanf(next("--out-view"), "%f,%f,%f", &o.view_x, &o.view_y, &o.view_zoom) != 3) return usage(); o.have_view = true; }
        else if (a == "--out-samples") { o.view_samples = std::atoi(next("--out-samples")); o.have_view = true; }
        else if (a == "--out-filter") { o.view_filter = (float)std::atof(next("--out-filter")); o.have_view = true; }
        else if (a == "--overlay") o.overlay = next("--overlay");
        else if (a == "--overlay-scale") o.overlay_scale = std::atoi(next("--overlay-scale"));
        else if (a == "--overlay-stride") o.overlay_stride = std::atoi(next("--overlay-stride"));
        else if (a == "--overlay-vertices") o.overlay_dump = next("--overlay-vertices");
        else if (a == "--convert") { o.convert_in = next("--convert"); o.convert_out = next("--convert"); }
        else if (a == "--load-checkpoint") o.load_ckpt = next("--load-checkpoint");
        else if (a == "--save-checkpoint") o.save_ckpt = next("--save-checkpoint");
        else if (a == "--device") o.device = std::atoi(next("--device"));
        else if (a == "--gpus") o.gpus = std::atoi(next("--gpus"));
        else if (a == "--share-gpu") o.share_gpu = true;
        else if (a == "--exchange") {
            const std::string v = next("--exchange");
            if (v != "halo" && v != "dense") return usage();
            o.replicated = v == "dense";
        }
        else if (a == "--rebin-interval") o.rebin_interval = std::atoi(next("--rebin-interval"));
        else if (a == "--quiet") o.quiet = true;
        else if (a == "--lr") o.lr = (float)std::atof(next("--lr"));
        else if (a == "--deterministic") o.deterministic = true;
        else if (a == "--reference-order") o.reference_order = true;
        else if (a == "--stall-timeout-ms") o.stall_ms = std::atoi(next("--stall-timeout-ms"));
        else if (a == "--loss-weights") {
            o.loss.struct_size = sizeof(o.loss);
            if (std::sscanf(next("--loss-weights"), "%f,%f,%f", &o.loss.w_mse, &o.loss.w_l1, &o.loss.w_dssim) != 3) return usage();
            o.have_loss = true;
        }
        else if (a == "--lr-groups" || a == "--lr-final-ratio") {
            float* v = a == "--lr-groups" ? o.lr_groups : o.lr_ratio;
            if (std::sscanf(next(a.c_str()), "%f,%f,%f,%f,%f", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5) return usage();
            (a == "--lr-groups" ? o.have_lr_groups : o.have_lr_ratio) = true;
        }
        else if (a == "--lr-decay-iters") o.lr_decay_iters = std::atoi(next("--lr-decay-iters"));
        else if (a == "--rebin-margin") o.rebin_margin = (float)std::atof(next("--rebin-margin"));
        else if (a == "--freeze-unmoved") o.freeze_unmoved = true;
        else if (a == "--relocate-every") o.relocate_every = std::atoi(next("--relocate-every"));
        else if (a == "--relocate-window") o.relocate_window = std::atoi(next("--relocate-window"));
        else if (a == "--relocate-max-fraction") o.relocate_max_fraction = (float)std::atof(next("--relocate-max-fraction"));
        else if (a == "--relocate-min-weight") o.relocate_min_weight = (float)std::atof(next("--relocate-min-weight"));
        else if (a == "--seed-init") o.seed_init = next("--seed-init");
        else if (a == "--reseed-every") o.reseed_every = std::atoi(next("--reseed-every"));
        else if (a == "--reseed-window") o.reseed_window = std::atoi(next("--reseed-window"));
        else if (a == "--reseed-max-fraction") o.reseed_max_fraction = (float)std::atof(next("--reseed-max-fraction"));
        else if (a == "--reseed-min-weight") o.reseed_min_weight = (float)std::atof(next("--reseed-min-weight"));
        else if (a == "--reseed-scale") o.reseed_scale = (float)std::atof(next("--reseed-scale"));
        else if (a == "--alive-from") { o.alive_from = std::atoi(next("--alive-from")); have_alive_from = true; }
        else if (a == "--grow-every") o.grow_every = std::atoi(next("--grow-every"));
        else if (a == "--grow-count") o.grow_count = std::atoi(next("--grow-count"));
        else if (a == "--grow-scale") o.grow_scale = (float)std::atof(next("--grow-scale"));
        else if (a == "--prune-every") o.prune_every = std::atoi(next("--prune-every"));
        else if (a == "--prune-min-weight") o.prune_min_weight = (float)std::atof(next("--prune-min-weight"));
        else if (a == "--prune-window") o.prune_window = std::atoi(next("--prune-window"));
        else if (a == "--coverage") o.coverage = true;
        else if (a == "--coarse") o.coarse_malformed = !parse_coarse(next("--coarse"), &o.coarse);
        else if (a == "--coarse-samples") o.coarse_samples = std::atoi(next("--coarse-samples"));
        else if (a == "--weight-image") o.weight_image = next("--weight-image");
        else if (a == "--weight-gain") {
            char* end = nullptr;
            const char* text = next("--weight-gain");
            o.weight_gain = std::strtof(text, &end);
            o.weight_gain_malformed = end == text || *end != '\0' || !(o.weight_gain >= 0.0f) || !std::isfinite(o.weight_gain);
            o.have_weight_gain = true;
        }
        else if (a == "--background") { o.background_malformed = !parse_background(next("--background"), o.background); o.have_background = true; }
        else return usage();
    }
    if (!o.convert_in.empty()) { // file conversion between .s2di / .ppm / .png; touches no GPU
        s2dio::Image8 im;
        if (!s2dio::load_image(o.convert_in, &im)) { std::fprintf(stderr, "cannot read %s\n", o.convert_in.c_str()); return 1; }
        if (!s2dio::save_image(o.convert_out, im)) { std::fprintf(stderr, "cannot write %s\n", o.convert_out.c_str()); return 1; }
        return 0;
    }
    if (o.image.empty() == (o.syn_w == 0) || o.n_splats < 0 || o.iters < 0 || o.batch < 1 || o.overlay_scale < 1) return usage();

    // imageRef, main.cpp:253-259
    int W = o.syn_w, H = o.syn_h;
    std::vector<float> imageRef;
    if (o.coverage) { // (all of it before a file or the device is touched)
        if (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI")) {
            std::fprintf(stderr, "--coverage works on one context: the multi-device handle has no coverage channel\n");
            return 2;
        }
        if (o.have_loss) {
            std::fprintf(stderr, "--coverage trains with the squared error over four channels: not together with --loss-weights\n");
            return 2;
        }
        if (o.relocate_every > 0 || o.reseed_every > 0 || o.prune_every > 0) {
            std::fprintf(stderr, "--coverage has no density statistics: not together with --relocate-every, --reseed-every or --prune-every\n");
            return 2;
        }
        if (o.reference_order) {
            std::fprintf(stderr, "--coverage is not available with --reference-order\n");
            return 2;
        }
        if (!o.out_image.empty() && !s2dio::ends_with(o.out_image, ".png")) {
            std::fprintf(stderr, "--coverage writes --out-image with its alpha: the file must be a .png\n");
            return 2;
        }
    }
    if (o.have_background) { // (all of it before a file or the device is touched)
        if (o.background_malformed) {
            std::fprintf(stderr, "--background takes three finite values R,G,B, e.g. 1,1,1\n");
            return 2;
        }
        if (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI")) {
            std::fprintf(stderr, "--background works on one context: the multi-device handle has no backdrop\n");
            return 2;
        }
        if (o.coverage || o.reference_order || !o.coarse.empty() || o.coarse_malformed) {
            std::fprintf(stderr, "--background is not available with --coverage, --reference-order or --coarse\n");
            return 2;
        }
    }
    if (o.have_weight_gain && o.weight_image.empty()) {
        std::fprintf(stderr, "--weight-gain scales a weight image: give --weight-image as well\n");
        return 2;
    }
    if (!o.weight_image.empty()) { // (all of it before a file or the device is touched)
        if (o.weight_gain_malformed) {
            std::fprintf(stderr, "--weight-gain takes one finite value >= 0, e.g. 3\n");
            return 2;
        }
        if (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI")) {
            std::fprintf(stderr, "--weight-image works on one context: the multi-device handle has no pixel weights\n");
            return 2;
        }
        if (o.coverage || !o.coarse.empty() || o.coarse_malformed) {
            std::fprintf(stderr, "--weight-image is not available with --coverage or --coarse\n");
            return 2;
        }
    }
    if (!o.image.empty() && o.coverage) {
        s2dio::ImageRGBA8 im;
        if (!s2dio::load_image_rgba(o.image, &im)) {
            std::fprintf(stderr, "cannot read %s (.s2di, binary .ppm, 8-bit non-interlaced .png and Huffman .jpg are supported)\n", o.image.c_str());
            return 1;
        }
        W = im.w;
        H = im.h;
        imageRef = s2dio::premultiplied_target(im);
    } else if (!o.image.empty()) {
        s2dio::Image8 im;
        if (!s2dio::load_image(o.image, &im)) {
            std::fprintf(stderr, "cannot read %s (.s2di, binary .ppm, 8-bit non-interlaced .png and Huffman .jpg are supported)\n", o.image.c_str());
            return 1;
        }
        W = im.w;
        H = im.h;
        const std::vector<uint8_t>& rgb = im.rgb;
        imageRef.resize((size_t)W * H * 4);
        for (size_t p = 0; p < (size_t)W * H; p++) { // Image2DRGBA8_to_Image2DRGBA32: byte / 255.0f
            for (int c = 0; c < 3; c++) imageRef[p * 4 + c] = (float)rgb[p * 3 + c] / 255.0f;
            imageRef[p * 4 + 3] = 1.0f;
        }
    }

    if (o.gpus < 1) return usage();
    if (o.relocate_every < 0 || o.relocate_window < 1 || !(o.relocate_max_fraction >= 0.0f) || !(o.relocate_min_weight >= 0.0f)) return usage();
    if (o.have_loss && (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI"))) {
        std::fprintf(stderr, "--loss-weights works on one context: the multi-device handle has no loss but the squared error\n");
        return 2;
    }
    if (o.relocate_every > 0 && (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI"))) {
        std::fprintf(stderr, "--relocate-every works on one context: the multi-device handle has no relocation\n");
        return 2;
    }
    if (o.have_view && (o.view_w < 0 || o.view_h < 0 || (o.view_samples != 1 && o.view_samples != 2 && o.view_samples != 4) || !(o.view_zoom > 0.0f) ||
                        !(o.view_filter >= 0.0f)))
        return usage();
    if (o.have_view && (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI"))) {
        std::fprintf(stderr, "--out-size, --out-view, --out-samples and --out-filter work on one context: the multi-device handle has no views\n");
        return 2;
    }
    if (!o.seed_init.empty() && o.seed_init != "edges" && o.seed_init != "uniform") return usage();
    if (o.reseed_every < 0 || o.reseed_window < 1 || !(o.reseed_max_fraction >= 0.0f) || !(o.reseed_min_weight >= 0.0f) || !(o.reseed_scale >= 0.0f))
        return usage();
    if ((o.reseed_every > 0 || !o.seed_init.empty()) && (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI"))) {
        std::fprintf(stderr, "--seed-init and --reseed-every work on one context: the multi-device handle has no placement\n");
        return 2;
    }
    if (o.reseed_every > 0 && o.relocate_every > 0) {
        std::fprintf(stderr, "--reseed-every and --relocate-every both own the statistics window: choose one\n");
        return 2;
    }
    const bool have_optim = o.have_lr_groups || o.have_lr_ratio || o.lr_decay_iters != 0;
    if (!(o.rebin_margin >= 0.0f) || o.lr_decay_iters < 0) return usage();
    if ((have_optim || o.freeze_unmoved) && (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI"))) {
        std::fprintf(stderr, "--lr-groups, --lr-final-ratio, --lr-decay-iters and --freeze-unmoved work on one context: the multi-device handle has no optimiser controls\n");
        return 2;
    }
    if (o.freeze_unmoved && o.reseed_every == 0 && o.relocate_every == 0) {
        std::fprintf(stderr, "--freeze-unmoved needs --reseed-every or --relocate-every: it freezes what their events did not write\n");
        return 2;
    }
    const bool alive_options = have_alive_from || o.grow_every != 0 || o.grow_count != 0 || o.prune_every != 0;
    if (alive_options) { // (all of it before the device is touched)
        if ((have_alive_from && (o.alive_from < 0 || o.alive_from > o.n_splats)) || o.grow_every < 0 || o.grow_count < 0 || !(o.grow_scale >= 0.0f) ||
            o.prune_every < 0 || o.prune_window < 1 || !(o.prune_min_weight > 0.0f))
            return usage();
        if ((o.grow_every > 0) != (o.grow_count > 0)) {
            std::fprintf(stderr, "--grow-every and --grow-count go together\n");
            return 2;
        }
        if (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI")) {
            std::fprintf(stderr, "--alive-from, --grow-every and --prune-every work on one context: the multi-device handle has no alive set\n");
            return 2;
        }
        if (o.reference_order) {
            std::fprintf(stderr, "--alive-from, --grow-every and --prune-every are not available with --reference-order\n");
            return 2;
        }
        if (!o.save_ckpt.empty() || !o.load_ckpt.empty()) {
            std::fprintf(stderr, "--alive-from, --grow-every and --prune-every: the checkpoint format does not carry the alive set\n");
            return 2;
        }
        if (o.prune_every > 0 && (o.relocate_every > 0 || o.reseed_every > 0)) {
            std::fprintf(stderr, "--prune-every owns the statistics window: not together with --relocate-every / --reseed-every\n");
            return 2;
        }
    }
    if (o.coarse_malformed || !o.coarse.empty() || o.coarse_samples != 1) { // (all of it before the device is touched)
        if (o.coarse_malformed || o.coarse.empty()) {
            std::fprintf(stderr, "--coarse takes a list of stages Z:K[,Z:K...] (zoom:iterations), e.g. 0.25:100,0.5:100%s\n",
                         o.coarse_malformed ? "" : "; --coarse-samples goes with it");
            return 2;
        }
        for (const auto& st : o.coarse) {
            if (!(st.first >= 1.0f / 256.0f) || !(st.first <= 65536.0f) || st.second < 0 || st.second > (1 << 24)) { // (the library resamples no target below 1/256)
                std::fprintf(stderr, "--coarse %g:%d: the zoom must be at least 1/256 and the iteration count >= 0\n", (double)st.first, st.second);
                return 2;
            }
        }
        if (o.coarse_samples != 1 && o.coarse_samples != 2 && o.coarse_samples != 4) {
            std::fprintf(stderr, "--coarse-samples must be 1, 2 or 4\n");
            return 2;
        }
        if (o.gpus > 1 || std::getenv("S2D_TRAIN_FORCE_MULTI")) {
            std::fprintf(stderr, "--coarse works on one context: the multi-device handle has no views\n");
            return 2;
        }
        if (o.coverage || o.reference_order || o.have_loss) {
            std::fprintf(stderr, "--coarse trains views with the squared error: not together with --coverage, --reference-order or --loss-weights\n");
            return 2;
        }
        if (o.relocate_every > 0 || o.reseed_every > 0 || o.prune_every > 0 || o.grow_every > 0) {
            std::fprintf(stderr, "--coarse gathers no density statistics: not together with --relocate-every, --reseed-every, --prune-every or --grow-every\n");
            return 2;
        }
    }
    // The stage iteration `it` lies in (nullptr: none, full size), and where it ends.
    auto coarse_stage_at = [&](int it, int* end) -> const std::pair<float, int>* {
        int begin = 0;
        for (const auto& st : o.coarse) {
            if (it >= begin && it < begin + st.second) {
                *end = begin + st.second;
                return &st;
            }
            begin += st.second;
        }
        return nullptr;
    };
    std::vector<float> weight_plane; // --weight-image: read and sized before the device is asked for anything
    if (!o.weight_image.empty()) {
        s2dio::Image8 wim;
        if (!s2dio::load_image(o.weight_image, &wim)) {
            std::fprintf(stderr, "cannot read the weight image %s\n", o.weight_image.c_str());
            return 1;
        }
        if (wim.w != W || wim.h != H) {
            std::fprintf(stderr, "the weight image %s is %dx%d, the target %dx%d: --weight-image needs the target's size\n",
                         o.weight_image.c_str(), wim.w, wim.h, W, H);
            return 2;
        }
        weight_plane.resize((size_t)W * H);
        for (size_t p = 0; p < weight_plane.size(); p++) {
            const float v = (float)wim.rgb[p * 3] / 255.0f;
            weight_plane[p] = o.have_weight_gain ? 1.0f + o.weight_gain * v : v;
        }
    }
    const bool weighted = !o.weight_image.empty();
    static const s2d_loss_config mse_only = {(uint32_t)sizeof(s2d_loss_config), 1.0f, 0.0f, 0.0f};
    bool views_held = false; // a stage ran and s2d_view_release has not followed yet
    Session S;
    CK(S.create(o, W, H));
    if (o.have_background) CK(s2d_set_backdrop(S.ctx, o.background));
    if (!o.weight_image.empty()) CK(s2d_set_pixel_weights(S.ctx, weight_plane.data()));
    if (have_optim) { // (groups without a rate of their own: the one --lr)
        s2d_optim_config oc;
        std::memset(&oc, 0, sizeof(oc));
        oc.struct_size = sizeof(oc);
        for (int g = 0; g < 5; g++) {
            oc.rate[g] = o.have_lr_groups ? o.lr_groups[g] : (o.lr > 0.0f ? o.lr : 0.05f);
            oc.final_ratio[g] = o.have_lr_ratio ? o.lr_ratio[g] : 0.0f;
        }
        oc.decay_iterations = o.lr_decay_iters;
        CK(s2d_set_optim(S.ctx, &oc));
    }
    // --freeze-unmoved: the state in front of an event, to tell afterwards which rows it wrote
    std::vector<s2d_splat> before_sp;
    std::vector<s2d_splat_adam> before_ad;
    auto remember_rows = [&]() -> int {
        if (!o.freeze_unmoved) return S2D_OK;
        before_sp.resize((size_t)o.n_splats);
        before_ad.resize((size_t)o.n_splats);
        if (int rc = s2d_get_splats(S.ctx, before_sp.data())) return rc;
        return s2d_get_adam(S.ctx, before_ad.data(), nullptr, nullptr, nullptr);
    };
    auto freeze_unwritten_rows = [&]() -> int {
        if (!o.freeze_unmoved) return S2D_OK;
        std::vector<s2d_splat> sp((size_t)o.n_splats);
        std::vector<s2d_splat_adam> ad((size_t)o.n_splats);
        if (int rc = s2d_get_splats(S.ctx, sp.data())) return rc;
        if (int rc = s2d_get_adam(S.ctx, ad.data(), nullptr, nullptr, nullptr)) return rc;
        std::vector<uint8_t> frozen((size_t)o.n_splats);
        int trained = 0;
        for (size_t i = 0; i < frozen.size(); i++) {
            frozen[i] = std::memcmp(&sp[i], &before_sp[i], sizeof(s2d_splat)) == 0 && std::memcmp(&ad[i], &before_ad[i], sizeof(s2d_splat_adam)) == 0;
            trained += frozen[i] ? 0 : 1;
        }
        std::fprintf(stderr, "froze %d splats, %d stay trained\n", o.n_splats - trained, trained);
        return s2d_set_frozen(S.ctx, frozen.data());
    };
    if (S.is_multi && o.stall_ms >= 0) CK(s2d_multi_set_stall_timeout(S.multi, o.stall_ms));
    if (S.is_multi) { // which GPU runs which rows (stderr: stdout is the reference's trace)
        for (int r = 0; r < s2d_multi_device_count(S.multi); r++) {
            int32_t dev = 0, r0 = 0, r1 = 0;
            char pci[64] = "", name[128] = "";
            if (s2d_multi_device_info(S.multi, r, &dev, &r0, &r1, pci, (int32_t)sizeof(pci), name, (int32_t)sizeof(name)) == S2D_OK)
                std::fprintf(stderr, "rank %d: device %d (%s, %s), rows %d..%d\n", r, dev, pci, name, r0, r1);
        }
    }
    CK(S.set_target(imageRef)); // (empty: the synthetic target is generated on the device)
    // init(), and with --seed-init every row drawn again from the target (the moments init() zeroed stay zero)
    auto seed_all = [&]() -> int {
        if (o.seed_init.empty() || (have_alive_from && o.alive_from == 0)) return S2D_OK; // (no row alive: none to seed)
        s2d_seed_config sc;
        std::memset(&sc, 0, sizeof(sc));
        sc.struct_size = sizeof(sc);
        sc.source = S2D_SEED_TARGET_EDGES;
        sc.floor = o.seed_init == "uniform" ? 4095u : 0u;
        int32_t placed = 0;
        std::vector<int32_t> last; // --alive-from: only the rows that will be alive
        for (int i = o.n_splats - o.alive_from; have_alive_from && i < o.n_splats; i++) last.push_back(i);
        const int rc = have_alive_from ? s2d_seed_splats(S.ctx, &sc, last.data(), (int32_t)last.size(), &placed)
                                       : s2d_seed_splats(S.ctx, &sc, nullptr, o.n_splats, &placed);
        if (rc == S2D_OK) std::fprintf(stderr, "seeded %d splats from the target (%s)\n", (int)placed, o.seed_init.c_str());
        return rc;
    };
    // --alive-from: the last K0 rows -- the back of the blend order, so that what --grow-every adds lies in front of them
    auto alive_from_start = [&]() -> int {
        if (!have_alive_from) return S2D_OK;
        std::vector<uint8_t> mask((size_t)o.n_splats, 0);
        for (int i = o.n_splats - o.alive_from; i < o.n_splats; i++) mask[(size_t)i] = 1;
        const int rc = s2d_set_alive(S.ctx, mask.data());
        if (rc == S2D_OK) std::fprintf(stderr, "%d of %d splats alive at the start\n", o.alive_from, o.n_splats);
        return rc;
    };
    CK(S.init());               // init(); main.cpp:307
    CK(seed_all());
    CK(alive_from_start());

    int iterations = 0; // main.cpp:278
    if (!o.load_ckpt.empty()) {
        FILE* f = std::fopen(o.load_ckpt.c_str(), "rb");
        CkptHeader h;
        std::vector<s2d_splat> sp((size_t)o.n_splats);
        std::vector<s2d_splat_adam> ad((size_t)o.n_splats);
        const bool ok = f && std::fread(&h, sizeof(h), 1, f) == 1 && std::memcmp(h.magic, "S2DC", 4) == 0 &&
                        (int)h.n_splats == o.n_splats && (int)h.width == W && (int)h.height == H &&
                        std::fread(sp.data(), sizeof(s2d_splat), sp.size(), f) == sp.size() &&
                        std::fread(ad.data(), sizeof(s2d_splat_adam), ad.size(), f) == ad.size();
        if (f) std::fclose(f);
        if (!ok) {
            std::fprintf(stderr, "cannot load checkpoint %s (wrong size or format)\n", o.load_ckpt.c_str());
            S.destroy();
            return 1;
        }
        CK(S.set_splats(sp.data()));
        CK(S.set_adam(ad.data(), h.beta1t, h.beta2t, h.iterations));
        iterations = h.iterations;
        o.iters += iterations; // --iters counts iterations to run from the checkpoint
    }
    std::vector<double> mse((size_t)o.batch), loss((size_t)o.batch);
    int frames = 0; // iterations run by this process (the trace numbering restarts at Restart, this does not)
    const auto t0 = std::chrono::steady_clock::now();
    while (iterations < o.iters) { // while (pr::NextFrame() == false), main.cpp:334
        if (iterations == o.restart_at) { // ImGui::Button("Restart"), main.cpp:828-831: init() also sets
            CK(S.init());                 // iterations = 0 (main.cpp:281), so the trace restarts at "0 itr"
            CK(seed_all());
            CK(alive_from_start());
            o.iters -= iterations;        // --iters is the number of frames to run in total
            iterations = 0;
            o.restart_at = -1;
        }
        int k = o.batch;
        if (k > o.iters - iterations) k = o.iters - iterations;
        if (o.optimize_opacity && iterations < o.opacity_from && iterations + k > o.opacity_from) k = o.opacity_from - iterations;
        if (o.restart_at > iterations && iterations + k > o.restart_at) k = o.restart_at - iterations;
        const bool opacity_now = o.optimize_opacity && iterations >= o.opacity_from; // bool optimizeOpacity, main.cpp:317
        uint32_t density = 0u;
        if (o.relocate_every > 0 || o.reseed_every > 0 || o.prune_every > 0) {
            // iterations [mK - S, mK) gather the statistics; the relocation (or the reseeding) runs in front of iteration mK
            const bool reseed = o.reseed_every > 0; // (never both: refused above)
            const bool prune = o.prune_every > 0;   // (alone: refused above)
            const int K = prune ? o.prune_every : reseed ? o.reseed_every : o.relocate_every;
            const int window = prune ? o.prune_window : reseed ? o.reseed_window : o.relocate_window;
            const int S_ = window < K ? window : K;
            int32_t passes = 0;
            if (iterations > 0 && iterations % K == 0) CK(s2d_density_get(S.ctx, nullptr, &passes));
            if (passes > 0 && prune) {
                s2d_prune_config pc;
                pc.struct_size = sizeof(pc);
                pc.min_weight = o.prune_min_weight;
                pc.min_opacity = 0.0f;
                int32_t pruned = 0, alive = 0;
                CK(s2d_prune(S.ctx, &pc, &pruned));
                CK(s2d_get_alive(S.ctx, nullptr, &alive));
                std::fprintf(stderr, "pruned %d splats before iteration %d, %d alive\n", (int)pruned, iterations, (int)alive);
            } else if (passes > 0 && reseed) {
                s2d_seed_config sc;
                std::memset(&sc, 0, sizeof(sc));
                sc.struct_size = sizeof(sc);
                sc.source = S2D_SEED_ERROR;
                sc.flags = S2D_SEED_SQUARED;
                sc.seed = (uint32_t)(iterations / K);
                sc.scale = o.reseed_scale;
                int32_t moved = 0;
                CK(s2d_forward(S.ctx)); // the error map is that of the current parameters
                CK(remember_rows());
                CK(s2d_reseed(S.ctx, &sc, (int32_t)(o.reseed_max_fraction * (float)o.n_splats), o.reseed_min_weight, &moved));
                std::fprintf(stderr, "reseeded %d splats before iteration %d\n", (int)moved, iterations);
                CK(freeze_unwritten_rows());
            } else if (passes > 0) { // (none: the run began here, from a checkpoint or a Restart)
                s2d_relocate_config rc;
                rc.struct_size = sizeof(rc);
                rc.max_moves = (int32_t)(o.relocate_max_fraction * (float)o.n_splats);
                rc.min_weight = o.relocate_min_weight;
                rc.shrink = 0.0f;
                int32_t moved = 0;
                CK(remember_rows());
                CK(s2d_relocate(S.ctx, &rc, &moved));
                std::fprintf(stderr, "relocated %d splats before iteration %d\n", (int)moved, iterations);
                CK(freeze_unwritten_rows());
            }
            const int next_reloc = (iterations / K + 1) * K, window_begin = next_reloc - S_;
            if (iterations >= window_begin) density = S2D_STEP_DENSITY_STATS;
            else if (iterations + k > window_begin) k = window_begin - iterations;
            if (iterations + k > next_reloc) k = next_reloc - iterations;
        }
        if (o.grow_every > 0) { // before iteration M, 2M, ...: while a row is dead
            int32_t alive = o.n_splats;
            if (iterations > 0 && iterations % o.grow_every == 0) CK(s2d_get_alive(S.ctx, nullptr, &alive));
            if (alive < o.n_splats) {
                s2d_seed_config sc;
                std::memset(&sc, 0, sizeof(sc));
                sc.struct_size = sizeof(sc);
                sc.source = S2D_SEED_ERROR;
                sc.flags = S2D_SEED_SQUARED;
                sc.seed = (uint32_t)(iterations / o.grow_every);
                sc.scale = o.grow_scale;
                int32_t grown = 0;
                CK(s2d_forward(S.ctx)); // the error map is that of the current parameters
                CK(s2d_grow(S.ctx, &sc, nullptr, o.grow_count, &grown));
                std::fprintf(stderr, "grew %d splats before iteration %d, %d alive\n", (int)grown, iterations, (int)(alive + grown));
            }
            const int next_grow = (iterations / o.grow_every + 1) * o.grow_every;
            if (iterations + k > next_grow) k = next_grow - iterations;
        }
        const uint32_t step_flags = (opacity_now ? S2D_STEP_OPTIMIZE_OPACITY : 0u) | density;
        int stage_end = 0;
        const std::pair<float, int>* stage = coarse_stage_at(iterations, &stage_end);
        if (!stage && views_held) { // behind the last stage: what the views allocated goes
            CK(s2d_view_release(S.ctx));
            views_held = false;
        }
        if (stage) { // k iterations at the stage's zoom, against the library's own resampled target
            if (iterations + k > stage_end) k = stage_end - iterations;
            s2d_view_config vc;
            std::memset(&vc, 0, sizeof(vc));
            vc.struct_size = sizeof(vc);
            vc.out_width = (int32_t)std::ceil((double)W * (double)stage->first);
            vc.out_height = (int32_t)std::ceil((double)H * (double)stage->first);
            vc.zoom = stage->first;
            vc.samples = o.coarse_samples;
            vc.format = S2D_VIEW_RGBA32F;
            CK(s2d_step_view(S.ctx, &vc, nullptr, k, step_flags, mse.data()));
            views_held = true;
        } else if (o.have_loss || weighted) // (under a plane s2d_step is s2d_step_loss of the squared error: this way the loss comes back)
            CK(s2d_step_loss(S.ctx, k, step_flags, o.have_loss ? &o.loss : &mse_only, loss.data(), mse.data()));
        else CK(S.step(k, step_flags, mse.data()));
        if (!o.quiet)
            for (int j = 0; j < k; j++) {
                std::printf("%d itr, mse %.4f", iterations + j, mse[(size_t)j]); // main.cpp:807
                if (o.have_loss) std::printf(", loss %.6f", loss[(size_t)j]);
                if (weighted) std::printf(", wloss %.6f", loss[(size_t)j]);
                std::printf("\n");
            }
        iterations += k; // main.cpp:809
        frames += k;
    }
    if (views_held) CK(s2d_view_release(S.ctx)); // (the stages reached the end of the run)
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "%d iterations in %.3f s = %.2f it/s (%dx%d, %d splats%s)\n", frames, secs,
                 secs > 0 ? frames / secs : 0.0, W, H, o.n_splats, S.exchange_summary(o).c_str());
    if (alive_options) {
        int32_t alive = 0;
        CK(s2d_get_alive(S.ctx, nullptr, &alive));
        std::fprintf(stderr, "%d of %d splats alive at the end\n", (int)alive, o.n_splats);
    }
    int exit_code = 0; // an output file that cannot be written is an error, reported after everything else was tried

    if (!o.save_ckpt.empty()) {
        CkptHeader h;
        std::memcpy(h.magic, "S2DC", 4);
        h.n_splats = (uint32_t)o.n_splats; h.width = (uint32_t)W; h.height = (uint32_t)H;
        std::vector<s2d_splat> sp((size_t)o.n_splats);
        std::vector<s2d_splat_adam> ad((size_t)o.n_splats);
        CK(S.get_splats(sp.data()));
        CK(S.get_adam(ad.data(), &h.beta1t, &h.beta2t, &h.iterations));
        FILE* f = std::fopen(o.save_ckpt.c_str(), "wb");
        const bool ok = f && std::fwrite(&h, sizeof(h), 1, f) == 1 &&
                        std::fwrite(sp.data(), sizeof(s2d_splat), sp.size(), f) == sp.size() &&
                        std::fwrite(ad.data(), sizeof(s2d_splat_adam), ad.size(), f) == ad.size();
        if (f) std::fclose(f);
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", o.save_ckpt.c_str());
            exit_code = 1;
        }
    }
    if (o.have_view && !o.out_image.empty()) { // the RGBA8 view of the final splats (s2d_render_view)
        s2d_view_config vc;
        std::memset(&vc, 0, sizeof(vc));
        vc.struct_size = sizeof(vc);
        vc.out_width = o.view_w > 0 ? o.view_w : W;
        vc.out_height = o.view_h > 0 ? o.view_h : H;
        vc.origin_x = o.view_x; vc.origin_y = o.view_y; vc.zoom = o.view_zoom;
        vc.filter_var = o.view_filter; vc.samples = o.view_samples; vc.format = S2D_VIEW_RGBA8;
        std::vector<uint8_t> rgba((size_t)vc.out_width * (size_t)vc.out_height * 4);
        CK(s2d_render_view(S.ctx, &vc, rgba.data()));
        if (o.coverage) { // premultiplied bytes and the coverage byte -> straight alpha
            s2dio::ImageRGBA8 out;
            out.w = vc.out_width;
            out.h = vc.out_height;
            std::vector<float> f(rgba.size());
            for (size_t i = 0; i < rgba.size(); i++) f[i] = (float)rgba[i] / 255.0f;
            out = s2dio::quantise_straight(f, out.w, out.h);
            if (!s2dio::save_png_rgba(o.out_image, out)) {
                std::fprintf(stderr, "cannot write %s\n", o.out_image.c_str());
                exit_code = 1;
            }
        }
        s2dio::Image8 im;
        im.w = vc.out_width;
        im.h = vc.out_height;
        im.rgb.resize((size_t)im.w * im.h * 3);
        for (size_t p = 0; p < (size_t)im.w * im.h; p++)
            for (int c = 0; c < 3; c++) im.rgb[p * 3 + c] = rgba[p * 4 + c];
        if (!o.coverage && !s2dio::save_image(o.out_image, im)) {
            std::fprintf(stderr, "cannot write %s\n", o.out_image.c_str());
            exit_code = 1;
        }
    }
    if ((!o.out_image.empty() && !o.have_view) || !o.overlay.empty()) {
        std::vector<float> image0((size_t)W * H * 4);
        CK(S.forward());
        CK(S.get_image(image0.data())); // tex0->upload(image0), main.cpp:794
        const s2dio::Image8 im = s2dio::quantise(image0, W, H);
        if (!o.out_image.empty() && !o.have_view &&
            !(o.coverage ? s2dio::save_png_rgba(o.out_image, s2dio::quantise_straight(image0, W, H)) : s2dio::save_image(o.out_image, im))) {
            std::fprintf(stderr, "cannot write %s\n", o.out_image.c_str());
            exit_code = 1;
        }
        if (!o.overlay.empty()) { // the reference's splat visualisation, main.cpp:441-485
            std::vector<s2d_splat> sp((size_t)o.n_splats);
            CK(S.get_splats(sp.data()));
            s2dio::Image8 big = s2dio::upscale(im, o.overlay_scale);
            std::vector<s2dio::OverlayVertex> verts;
            s2dio::draw_splat_overlay(&big, sp, o.overlay_scale, o.overlay_stride, o.overlay_dump.empty() ? nullptr : &verts);
            if (!o.overlay_dump.empty()) {
                // "S2DV", int32 vertex count, then 16 bytes per vertex: float x, y, z (scene coordinates of main.cpp:447:
                // x, -y, 0), uint8 r, g, b, 0 -- 46 vertices per drawn splat, in the reference's PrimVertex order
                FILE* f = std::fopen(o.overlay_dump.c_str(), "wb");
                const int32_t count = (int32_t)verts.size();
                const bool ok = f && std::fwrite("S2DV", 1, 4, f) == 4 && std::fwrite(&count, 4, 1, f) == 1 &&
                                std::fwrite(verts.data(), sizeof(s2dio::OverlayVertex), verts.size(), f) == verts.size();
                if (f) std::fclose(f);
                if (!ok) {
                    std::fprintf(stderr, "cannot write %s\n", o.overlay_dump.c_str());
                    exit_code = 1;
                }
            }
            if (!s2dio::save_image(o.overlay, big)) {
                std::fprintf(stderr, "cannot write %s\n", o.overlay.c_str());
                exit_code = 1;
            }
        }
    }
    S.destroy();
    return exit_code;
}
