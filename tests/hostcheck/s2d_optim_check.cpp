// s2d_optim_check.cpp -- TEST SHIM.  Compiles the host side of the optimiser controls
// (2dgaussiansplatting_amd/csrc/s2d_optim_rates.h: what s2d_set_optim refuses, and the rate of a parameter group at an
// iteration -- the very functions the library calls) for the host, so that tests/test_optim_cpu.py can hold them to the
// header's words and a float64 restatement.  Not a fallback: the product never links this.
#include "../../2dgaussiansplatting_amd/csrc/s2d_optim_rates.h"

extern "C" unsigned oc_config_size(void) { return (unsigned)sizeof(s2d_optim_config); }

// 0: acceptable; 1: refused.
extern "C" int oc_refused(const s2d_optim_config* cfg) { return s2d::optim_config_refused(cfg) != nullptr; }

// The five rates of iteration t (cfg may be null: training_rate five times).
extern "C" void oc_rates_at(const s2d_optim_config* cfg, float training_rate, int32_t t, float* rates5)
{
    s2d::optim_rates_at(cfg, training_rate, t, rates5);
}

extern "C" int oc_group_of(int k) { return s2d::kOptimGroupOf[k]; }
