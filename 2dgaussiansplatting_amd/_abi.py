"""The C ABI of include/splat2d.h and include/splat2d_test.h as ctypes sees it: constants, structures, one signature table.

Everything here is written once and held to the headers by tests/test_abi_cpu.py: every S2D_* constant and status against
the #defines and the enum, every field of every structure against sizeof / offsetof of the C type STRUCTS names, and the
keys of SIGNATURES against the declarations.  A new entry point is one line in SIGNATURES; a symbol without one cannot be
called with ctypes' default `int` arguments, because the test compares the table with the headers.
"""
import ctypes as C

import numpy as np

# == struct Splat (main.cpp:85-93), 36 bytes; == struct SplatAdam (main.cpp:158-166), 72 bytes
SPLAT_DTYPE = np.dtype([("pos", "<f4", 2), ("sx", "<f4"), ("sy", "<f4"), ("rot", "<f4"),
                        ("color", "<f4", 3), ("opacity", "<f4")])
ADAM_DTYPE = np.dtype([("mv", "<f4", (9, 2))])

S2D_ABI_VERSION = 2
ABI_VERSION = S2D_ABI_VERSION  # as this binding was written (checked against the library at load)

S2D_OK, S2D_E_INVALID, S2D_E_HIP, S2D_E_NONFINITE, S2D_E_NOMEM, S2D_E_STATE = 0, 1, 2, 3, 4, 5  # s2d_status
STATUS_NAMES = {S2D_OK: "S2D_OK", S2D_E_INVALID: "S2D_E_INVALID", S2D_E_HIP: "S2D_E_HIP", S2D_E_NONFINITE: "S2D_E_NONFINITE",
                S2D_E_NOMEM: "S2D_E_NOMEM", S2D_E_STATE: "S2D_E_STATE"}

S2D_STEP_OPTIMIZE_OPACITY = 0x1
S2D_STEP_DENSITY_STATS = 0x2
S2D_BWD_SKIP_OPACITY_GRAD = 0x1
S2D_FB_SKIP_IMAGE = 0x2
S2D_BWD_DENSITY_STATS = 0x4
S2D_CFG_COUNT_PAIRS = 0x1
S2D_CFG_FP16_IMAGES = 0x2
S2D_CFG_DETERMINISTIC = 0x4
S2D_CFG_EXACT_EXP = 0x8
S2D_CFG_ADAM_FP32 = 0x10
S2D_CFG_GENERIC_BINNING = 0x20
S2D_CFG_REFERENCE_ORDER = 0x40
S2D_CFG_COVERAGE = 0x80
S2D_SEED_TARGET_EDGES, S2D_SEED_ERROR, S2D_SEED_CALLER = 0, 1, 2
S2D_SEED_SQUARED = 0x1
SEED_SOURCES = {"edges": S2D_SEED_TARGET_EDGES, "error": S2D_SEED_ERROR, "caller": S2D_SEED_CALLER}
S2D_VIEW_RGBA32F, S2D_VIEW_RGBA8 = 0, 1
S2D_VIEW_BWD_FROM_TARGET = 0x8  # s2d_view_backward_device / s2d_view_grads: the buffer is a target, dL = view - target
S2D_ROWS_GRADS, S2D_ROWS_SPLATS, S2D_ROWS_ADAM = 0, 1, 2  # row arrays of the slab-ownership calls
ROWS_GRADS, ROWS_SPLATS, ROWS_ADAM = S2D_ROWS_GRADS, S2D_ROWS_SPLATS, S2D_ROWS_ADAM
S2D_MULTI_SHARE_GPU = 0x1
S2D_MULTI_REPLICATED = 0x2
OPTIM_GROUPS = ("pos", "scale", "rot", "color", "opacity")  # the groups of s2d_optim_config, in its order


# The field names are the C field names: the layout test builds its offsetof() list from them.
class _Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                ("n_splats", C.c_int32), ("device", C.c_int32), ("row_begin", C.c_int32),
                ("row_end", C.c_int32), ("training_rate", C.c_float), ("flags", C.c_uint32),
                ("rebin_interval", C.c_int32), ("rebin_margin", C.c_float), ("stream", C.c_void_p)]


class _Stats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32),
                ("pairs_binned", C.c_uint64), ("pairs_capacity", C.c_uint64), ("rebins", C.c_uint64),
                ("fwd_visited", C.c_uint64), ("fwd_active", C.c_uint64), ("bwd_visited", C.c_uint64),
                ("bwd_active", C.c_uint64), ("fwd_staged", C.c_uint64), ("bwd_staged", C.c_uint64),
                ("fwd_wave_execs", C.c_uint64), ("bwd_wave_execs", C.c_uint64), ("bwd_lane_hist", C.c_uint64 * 65),
                ("iterations", C.c_int32), ("first_nonfinite_iteration", C.c_int32),
                ("fwd_staged_hit", C.c_uint64), ("fwd_rows_hit", C.c_uint64), ("bwd_quadrant_execs", C.c_uint64)]


class _RelocateConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_moves", C.c_int32), ("min_weight", C.c_float), ("shrink", C.c_float)]


class _SeedConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("source", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint32),
                ("floor", C.c_uint32), ("scale", C.c_float), ("opacity", C.c_float), ("importance_device", C.c_void_p)]


class _LossConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("w_mse", C.c_float), ("w_l1", C.c_float), ("w_dssim", C.c_float)]


class _LossTerms(C.Structure):
    _fields_ = [("mse", C.c_double), ("l1", C.c_double), ("dssim", C.c_double), ("total", C.c_double)]


class _OptimConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("rate", C.c_float * 5), ("final_ratio", C.c_float * 5),
                ("decay_iterations", C.c_int32)]


class _PruneConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_weight", C.c_float), ("min_opacity", C.c_float)]


class _ViewConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("out_width", C.c_int32), ("out_height", C.c_int32), ("origin_x", C.c_float),
                ("origin_y", C.c_float), ("zoom", C.c_float), ("filter_var", C.c_float), ("samples", C.c_int32),
                ("format", C.c_uint32)]


# the C type each structure mirrors
STRUCTS = {"s2d_config": _Config, "s2d_stats": _Stats, "s2d_relocate_config": _RelocateConfig, "s2d_seed_config": _SeedConfig,
           "s2d_loss_config": _LossConfig, "s2d_loss_terms": _LossTerms, "s2d_optim_config": _OptimConfig,
           "s2d_prune_config": _PruneConfig, "s2d_view_config": _ViewConfig}

_vp, _i32, _u32, _i64, _f32, _str, _int = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.c_float, C.c_char_p, C.c_int
_P = C.POINTER

# name -> (argtypes, restype) of every symbol the two headers declare, in their order.  Handles, arrays and out-parameters
# are void pointers (numpy and torch hand over addresses); a configuration structure is a pointer to its type.
SIGNATURES = {
    "s2d_abi_version": ([], _int),
    "s2d_create": ([_P(_Config), _P(_vp)], _int),
    "s2d_destroy": ([_vp], None),
    "s2d_set_target": ([_vp, _vp], _int),
    "s2d_set_target_synthetic": ([_vp], _int),
    "s2d_init_splats": ([_vp], _int),
    "s2d_set_splats": ([_vp, _vp], _int),
    "s2d_get_splats": ([_vp, _vp], _int),
    "s2d_set_adam": ([_vp, _vp, _f32, _f32, _i32], _int),
    "s2d_get_adam": ([_vp, _vp, _vp, _vp, _vp], _int),
    "s2d_forward": ([_vp], _int),
    "s2d_get_image": ([_vp, _vp], _int),
    "s2d_get_image_rows": ([_vp, _vp], _int),
    "s2d_backward": ([_vp, _u32], _int),
    "s2d_forward_backward": ([_vp, _u32], _int),
    "s2d_get_grads": ([_vp, _vp], _int),
    "s2d_backward_image_grads": ([_vp, _vp, _u32], _int),
    "s2d_set_splats_device": ([_vp, _vp], _int),
    "s2d_get_image_rows_device": ([_vp, _vp], _int),
    "s2d_density_get": ([_vp, _vp, _vp], _int),
    "s2d_density_get_device": ([_vp, _vp, _vp], _int),
    "s2d_density_reset": ([_vp], _int),
    "s2d_relocate": ([_vp, _P(_RelocateConfig), _vp], _int),
    "s2d_importance": ([_vp, _P(_SeedConfig), _vp, _vp], _int),
    "s2d_seed_splats": ([_vp, _P(_SeedConfig), _vp, _i32, _vp], _int),
    "s2d_reseed": ([_vp, _P(_SeedConfig), _i32, _f32, _vp], _int),
    "s2d_loss_image_grads_device": ([_vp, _P(_LossConfig), _vp], _int),
    "s2d_loss_backward": ([_vp, _P(_LossConfig), _u32], _int),
    "s2d_loss_get": ([_vp, _P(_LossTerms)], _int),
    "s2d_step_loss": ([_vp, _i32, _u32, _P(_LossConfig), _vp, _vp], _int),
    "s2d_adam_step": ([_vp, _u32], _int),
    "s2d_set_optim": ([_vp, _P(_OptimConfig)], _int),
    "s2d_optim_rates_at": ([_vp, _i32, _vp], _int),
    "s2d_set_frozen": ([_vp, _vp], _int),
    "s2d_set_frozen_device": ([_vp, _vp], _int),
    "s2d_set_alive": ([_vp, _vp], _int),
    "s2d_set_alive_device": ([_vp, _vp], _int),
    "s2d_get_alive": ([_vp, _vp, _vp], _int),
    "s2d_prune": ([_vp, _P(_PruneConfig), _vp], _int),
    "s2d_grow": ([_vp, _P(_SeedConfig), _vp, _i32, _vp], _int),
    "s2d_view_splats": ([_vp, _P(_ViewConfig), _vp], _int),
    "s2d_render_view": ([_vp, _P(_ViewConfig), _vp], _int),
    "s2d_render_view_device": ([_vp, _P(_ViewConfig), _vp], _int),
    "s2d_view_release": ([_vp], _int),
    "s2d_view_backward_device": ([_vp, _P(_ViewConfig), _vp, _u32], _int),
    "s2d_view_grads": ([_vp, _P(_ViewConfig), _vp, _u32, _vp], _int),
    "s2d_step": ([_vp, _i32, _u32, _vp], _int),
    "s2d_get_mse": ([_vp, _vp], _int),
    "s2d_halo_masks": ([_vp, _i32, _vp, _f32, _vp], _int),
    "s2d_halo_commit": ([_vp, _vp, _i32, _i32], _int),
    "s2d_rows_gather": ([_vp, _i32, _vp, _i32, _vp], _int),
    "s2d_rows_scatter": ([_vp, _i32, _vp, _i32, _vp], _int),
    "s2d_grads_combine": ([_vp, _vp, _i32, _vp, _i32, _vp], _int),
    "s2d_bind_grads_device": ([_vp, _vp], _int),
    "s2d_grads_device_ptr": ([_vp], _vp),
    "s2d_stream": ([_vp], _vp),
    "s2d_get_sqerr_trace": ([_vp, _i32, _i32, _vp], _int),
    "s2d_synchronize": ([_vp], _int),
    "s2d_multi_create": ([_P(_Config), _vp, _i32, _u32, _P(_vp)], _int),
    "s2d_multi_destroy": ([_vp], None),
    "s2d_multi_last_error": ([_vp], _str),
    "s2d_multi_device_count": ([_vp], _int),
    "s2d_multi_device_info": ([_vp, _i32, _vp, _vp, _vp, _str, _i32, _str, _i32], _int),
    "s2d_multi_set_stall_timeout": ([_vp, _i32], _int),
    "s2d_multi_set_target": ([_vp, _vp], _int),
    "s2d_multi_set_target_synthetic": ([_vp], _int),
    "s2d_multi_init_splats": ([_vp], _int),
    "s2d_multi_set_splats": ([_vp, _vp], _int),
    "s2d_multi_get_splats": ([_vp, _vp], _int),
    "s2d_multi_set_adam": ([_vp, _vp, _f32, _f32, _i32], _int),
    "s2d_multi_get_adam": ([_vp, _vp, _vp, _vp, _vp], _int),
    "s2d_multi_step": ([_vp, _i32, _u32, _vp], _int),
    "s2d_multi_forward": ([_vp], _int),
    "s2d_multi_get_image": ([_vp, _vp], _int),
    "s2d_multi_exchange_info": ([_vp, _vp], _int),
    "s2d_get_stats": ([_vp, _P(_Stats)], _int),
    "s2d_get_rebuild_count": ([_vp, _vp], _int),
    "s2d_last_error": ([_vp], _str),
    # include/splat2d_test.h
    "s2d_test_sincos": ([_i32, _vp, _i32, _vp, _vp], _int),
    "s2d_test_sort_pairs": ([_i32, _vp, _vp, _i64, _i32], _int),
    "s2d_test_sort_tile_offsets": ([_i32, _vp, _vp, _i64, _i32, _vp], _int),
    "s2d_test_exclusive_scan": ([_i32, _vp, _i64, _vp], _int),
    "s2d_debug_get_tile_lists": ([_vp, _vp, _vp, _vp, _i64, _vp, _i64], _int),
    "s2d_debug_view_raster": ([_vp, _P(_ViewConfig), _vp], _int),
    "s2d_test_multi_stall": ([_vp, _i32, _i32, _i32], _int),
}
ABI_SYMBOLS = list(SIGNATURES)


def apply_signatures(L, lenient=False):
    """Sets argtypes and restype of every symbol of the table on the loaded library L.  lenient: a symbol L lacks is skipped
    (an A/B build of an older ABI, tools/gpu_ab.py); otherwise a missing one raises AttributeError."""
    for name, (argtypes, restype) in SIGNATURES.items():
        if lenient and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.argtypes, f.restype = argtypes, restype
