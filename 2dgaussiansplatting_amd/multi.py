"""MultiTrainer: several GPUs behind one handle of the library (s2d_multi)."""
import ctypes as C

import numpy as np

from ._abi import (S2D_CFG_DETERMINISTIC, S2D_CFG_FP16_IMAGES, S2D_CFG_REFERENCE_ORDER, S2D_MULTI_REPLICATED,
                   S2D_MULTI_SHARE_GPU, S2D_STEP_OPTIMIZE_OPACITY, _Config)
from ._handle import _Handle, _p


class MultiTrainer(_Handle):
    """Several GPUs behind one handle (s2d_multi_*, csrc/s2d_multi.h and its units): the Trainer's state and step() on a list of
    devices -- row slabs and, inside the library, either slab ownership with peer-to-peer copies of the shared
    gradient rows (default) or replicated state with an RCCL all-reduce of all gradients (replicated=True).
    share_gpu: every rank on devices[0] (a rehearsal where there are fewer GPUs than ranks)."""

    _PREFIX = "s2d_multi_"
    # set_adam has never asserted the array's shape here as Trainer.set_adam does, and the library cannot refuse a host array
    # of the wrong length, so the difference a caller can observe stays
    _ADAM_SHAPE_ASSERTED = False
    SCHEMES = {0: "none", 1: "ownership", 2: "replicated"}

    def __init__(self, width, height, n_splats, devices, share_gpu=False, training_rate=0.0, rebin_interval=0,
                 fp16_images=False, deterministic=False, replicated=False, reference_order=False):
        self.W, self.H, self.n = int(width), int(height), int(n_splats)
        cfg = _Config()
        cfg.struct_size = C.sizeof(_Config)
        cfg.width, cfg.height, cfg.n_splats = self.W, self.H, self.n
        cfg.training_rate = float(training_rate)
        cfg.rebin_interval = int(rebin_interval)
        cfg.flags = ((S2D_CFG_FP16_IMAGES if fp16_images else 0) | (S2D_CFG_DETERMINISTIC if deterministic else 0) |
                     (S2D_CFG_REFERENCE_ORDER if reference_order else 0))  # (refused: a single-context mode)
        devs = (C.c_int32 * len(devices))(*devices)
        self._create(C.byref(cfg), devs, len(devices),
                     (S2D_MULTI_SHARE_GPU if share_gpu else 0) | (S2D_MULTI_REPLICATED if replicated else 0))
        self.optimize_opacity = False

    def step(self, iters=1, want_mse=True):
        out = np.zeros(iters, dtype=np.float64) if want_mse else None
        flags = S2D_STEP_OPTIMIZE_OPACITY if self.optimize_opacity else 0
        self._ck(self.L.s2d_multi_step(self._h, int(iters), flags, _p(out) if want_mse else None))
        return out

    def device_info(self, rank):
        """Which GPU runs which rows: {rank, device, row_begin, row_end, pci_bus_id, name} of one rank."""
        dev, r0, r1 = C.c_int32(), C.c_int32(), C.c_int32()
        pci, name = C.create_string_buffer(64), C.create_string_buffer(256)
        self._ck(self.L.s2d_multi_device_info(self._h, int(rank), C.byref(dev), C.byref(r0), C.byref(r1), pci, 64, name, 256))
        return {"rank": int(rank), "device": dev.value, "row_begin": r0.value, "row_end": r1.value,
                "pci_bus_id": pci.value.decode(), "name": name.value.decode()}

    def set_stall_timeout(self, milliseconds):
        """Every wait of one rank for another (and for its own stream) gives up after this long: step() then raises
        S2D_E_STATE naming the rank instead of hanging (0 = wait without bound)."""
        self._ck(self.L.s2d_multi_set_stall_timeout(self._h, int(milliseconds)))

    def test_stall(self, rank, iteration, milliseconds):
        """Failure injection (include/splat2d_test.h): rank `rank` stops answering at `iteration`."""
        self._ck(self.L.s2d_test_multi_stall(self._h, int(rank), int(iteration), int(milliseconds)))

    def exchange_info(self):
        """scheme, gradient rows swapped per iteration (all ranks), state rows handed over, splats held (all ranks)."""
        a = np.zeros(4, dtype=np.int64)
        self._ck(self.L.s2d_multi_exchange_info(self._h, _p(a)))
        return {"scheme": self.SCHEMES[int(a[0])], "rows_per_iteration": int(a[1]), "state_handovers": int(a[2]), "held": int(a[3])}
