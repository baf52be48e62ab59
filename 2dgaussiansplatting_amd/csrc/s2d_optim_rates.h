// s2d_optim_rates.h -- the optimiser controls of s2d_set_optim on the host: what a configuration is refused for, and the
// rate of a parameter group at an iteration.  Host-only and free of the HIP runtime, so that tests/hostcheck compiles it
// with g++ (tests/hostcheck/s2d_optim_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/splat2d.h"

namespace s2d {

constexpr int kOptimGroups = 5;
// scalar k of a splat (pos.xy, sx, sy, rot, color.rgb, opacity: the order of Splat and of SplatAdam) -> its group
constexpr int kOptimGroupOf[9] = {0, 0, 1, 1, 2, 3, 3, 3, 4};

// nullptr: the configuration is acceptable; otherwise what is wrong with it (s2d_set_optim: S2D_E_INVALID).
inline const char* optim_config_refused(const s2d_optim_config* cfg)
{
    if (!cfg) return "NULL";
    if (cfg->struct_size != sizeof(s2d_optim_config)) return "wrong struct_size";
    for (int g = 0; g < kOptimGroups; g++) {
        if (!(cfg->rate[g] > 0.0f) || std::isinf(cfg->rate[g])) return "every rate must be finite and > 0";
        if (!(cfg->final_ratio[g] >= 0.0f) || std::isinf(cfg->final_ratio[g])) return "every final_ratio must be 0 (meaning 1) or finite and > 0";
    }
    if (cfg->decay_iterations < 0) return "decay_iterations must be >= 0";
    return nullptr;
}

// The rate of group g for the step taken while the iteration counter is t: rate[g] itself when nothing decays, otherwise
// log-linear from rate[g] at 0 to rate[g] * final_ratio[g] at decay_iterations, constant from there on.  One double pow,
// rounded to fp32 once.
inline float optim_rate_at(const s2d_optim_config& cfg, int g, int32_t t)
{
    const float ratio = cfg.final_ratio[g] == 0.0f ? 1.0f : cfg.final_ratio[g];
    const int32_t T = cfg.decay_iterations;
    if (T == 0 || ratio == 1.0f) return cfg.rate[g];
    const int32_t tt = t < 0 ? 0 : (t < T ? t : T);
    return (float)((double)cfg.rate[g] * std::pow((double)ratio, (double)tt / (double)T));
}

// The five group rates of iteration t (cfg == nullptr: the context's single training_rate five times).
inline void optim_rates_at(const s2d_optim_config* cfg, float training_rate, int32_t t, float rates[kOptimGroups])
{
    for (int g = 0; g < kOptimGroups; g++) rates[g] = cfg ? optim_rate_at(*cfg, g, t) : training_rate;
}

} // namespace s2d
