"""Kernel 1's memory, copy and SHA3 opcodes on an MI355X, byte-exact three ways.

Each test runs one opcode's case list (memcases.py) on the device and asserts
that the lanes equal oracle/evm_ref.c's (diff_batches) and, field by field, the
pymem model's, which restates the reference's Python with a bytearray and
Python ints.  Every list runs under LDS memory windows of 160 (the default), 0,
32 and 96 bytes and once with the straight-line runs in their register form:
the lists put unaligned words, copies and hash inputs across each window's
edge and across the lanes' initial memory sizes.  test_memory_ops_cpu.py checks
on the CPU that the lists hold every outcome class and mix them within waves.
"""
import os

import pytest

import memcases
import pymem
from mythril_amd.device import GpuDevice
from mythril_amd.lanes import diff_batches
from test_gpu_lanes import run_both

pytestmark = pytest.mark.gpu

SWITCHES = ("MG_K1_MEMWIN", "MG_K1_RUNS")
CONFIGS = [{}, {"MG_K1_MEMWIN": "0"}, {"MG_K1_MEMWIN": "32"}, {"MG_K1_MEMWIN": "96"},
           {"MG_K1_RUNS": "reg"}]
CONFIG_IDS = ["default", "memwin0", "memwin32", "memwin96", "runs-reg"]


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


@pytest.fixture
def env():
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def check(dev, name, rec_cap=0):
    codes, b = memcases.sha3_cases(rec_cap) if name == "sha3" else memcases.CASES[name]()
    assert b.n <= 8192 and b.shape.mem_cap <= 2048 and b.shape.calldata_cap <= 256
    out, ref, _ = run_both(dev, codes, b)
    assert diff_batches(out, ref) == []
    want = memcases.model_results(name, rec_cap)
    assert len(want) == out.n
    bad = []
    for i, r in enumerate(want):
        bad += pymem.lane_diff(out, i, r)
        if len(bad) > 10:
            break
    assert bad == []


@pytest.mark.parametrize("switches", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("name", ["mload", "mstore", "mstore8", "calldataload", "calldatacopy",
                                  "codecopy", "return"])
def test_opcode_equals_oracle_and_model(dev, env, name, switches):
    env.update(switches)
    check(dev, name)


@pytest.mark.parametrize("switches", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("rec_cap", [0, 256])
def test_sha3_equals_oracle_and_model(dev, env, rec_cap, switches):
    env.update(switches)
    check(dev, "sha3", rec_cap)


@pytest.mark.parametrize("switches", CONFIGS, ids=CONFIG_IDS)
def test_mem_extend_gas_edges_equal_oracle_and_model(dev, env, switches):
    """MSTORE, SHA3 and CALLDATACOPY with the gas limit at, below and above the
    need; past mem_cap the limit decides between out of gas and the escape."""
    env.update(switches)
    check(dev, "gas")
