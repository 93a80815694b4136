#!/usr/bin/env python3
"""What a growing MSTORE costs kernel 1 against an in-range one: four programs on
converged waves (every lane runs the same code) through the diagnostic library
built with -DMG_K1_CLOCKS (MYTHGPU_LIB, as scripts/k1_clocks.py), reading the
MSTORE, MLOAD, prologue and epilogue clock bins of a `run_batches` launch.
The difference between two programs' MSTORE bins is the second store's cost.
stack_cap 8 keeps the stack window at eight slots: the diagnostic build's static
LDS is larger than what the LDS plan reserves, and with a code this small the
plan would otherwise ask for more than a workgroup can have."""
import ctypes
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
os.environ.setdefault("MYTHGPU_LIB", "ab/clk.so")
import numpy as np  # noqa: E402

from mythril_amd.device import GpuDevice  # noqa: E402
from mythril_amd.lanes import LaneBatch, LaneShape  # noqa: E402

BINS = 262
PROGRAMS = {
    "grow_0_96": bytes([0x60, 0x60, 0x60, 0x40, 0x52, 0x00]),
    "grow_0_96+inrange": bytes([0x60, 0x60, 0x60, 0x40, 0x52, 0x60, 0x01, 0x60, 0x00, 0x52, 0x00]),
    "grow_0_96+grow_96_160": bytes([0x60, 0x60, 0x60, 0x40, 0x52, 0x60, 0x01, 0x60, 0x80, 0x52, 0x00]),
    "grow_0_96+mload_inrange": bytes([0x60, 0x60, 0x60, 0x40, 0x52, 0x60, 0x40, 0x51, 0x00]),
}


def main(n=4096):
    dev = GpuDevice(0)
    dev.lib.mg_k1_clocks.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    for name, code in PROGRAMS.items():
        cid = dev.load_code(code)
        b = LaneBatch(LaneShape(n=n, stack_cap=8, mem_cap=1024, calldata_cap=32, storage_cap=1))
        for i in range(n):
            b.set_lane(i, code_id=cid, gas_limit=10 ** 7)
        dev.alloc(b.shape)
        dev.upload(b)
        dev.run_batches(2)
        dev.run_batches(1)
        buf = (ctypes.c_uint32 * (4096 * BINS))()
        assert dev.lib.mg_k1_clocks(dev.ctx, buf, 4096 * BINS) == 0
        raw = np.frombuffer(buf, dtype=np.uint32).reshape(4096, BINS)[: n // 64]
        clk, cnt = (raw & 0xFFFFFF).astype(float), (raw >> 24).astype(float)
        bins = {k: (float(cnt[:, j].mean()), int(round(clk[:, j].mean())))
                for k, j in (("MSTORE", 0x52), ("MLOAD", 0x51), ("prologue", 257), ("epilogue", 258))}
        print(f"{name}: (iterations, cycles) per wave {bins}, all bins {int(round(clk.sum(axis=1).mean()))}", flush=True)
    dev.close()


if __name__ == "__main__":
    main()
