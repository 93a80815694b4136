"""Kernel 2's interpreter on the MI355X, value by value: every case list of
tests/k2_opcases.py through mg_eval_terms (k_bv_terms) and mg_eval_bits
(k_bv_eval), compared as uint32 limbs with the Python reference of the program
format (tests/k2_insn_ref.py) -- never with device output or the C oracle
alone.  tests/test_k2_opcases_cpu.py pins that reference on the CPU."""
import functools

import numpy as np
import pytest

import k2_opcases as cases
from k2_terms_ref import limbs_to_int
from mythril_amd.device import GpuDevice

pytestmark = pytest.mark.gpu
GROUPS = cases.group_names()
FUSION = cases.group_names("fuse:")


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def _pool(name):
    return cases.all_groups()[name].pool()


def check_values(dev, name):
    """dev.eval_terms of a group == the reference, every program under every model; a
    mismatch names the op, width, operand kinds, model and both values."""
    g = cases.all_groups()[name]
    want = cases.reference_limbs(name)
    got, _ = dev.eval_terms(g.prog, _pool(name))
    assert got.shape == want.shape and got.dtype == np.uint32
    bad = np.argwhere((got != want).any(axis=2))
    if len(bad):
        d, m = map(int, bad[0])
        pytest.fail(f"{len(bad)} of {want.shape[0] * want.shape[1]} values differ; first: {g.describe(d, m)}: "
                    f"device {limbs_to_int(got[d, m]):#x}, reference {limbs_to_int(want[d, m]):#x}")


def check_bits(dev, name):
    """dev.eval_bits of a group: bit m of program d's bitmap == bit 0 of the reference
    value, the last word's padding bits are 0, and first_sat / sat_count follow."""
    g = cases.all_groups()[name]
    want = (cases.reference_limbs(name)[:, :, 0] & 1).astype(bool)
    n_models = want.shape[1]
    fs, sc, bits, _ = dev.eval_bits(g.prog, _pool(name))
    flat = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert flat.shape[1] == 64 * ((n_models + 63) // 64)
    assert not flat[:, n_models:].any(), "padding bits of the last bitmap word are set"
    bad = np.argwhere(flat[:, :n_models] != want)
    if len(bad):
        d, m = map(int, bad[0])
        pytest.fail(f"{len(bad)} bitmap bits differ; first: {g.describe(d, m)}: device {int(flat[d, m])}, "
                    f"reference {int(want[d, m])}")
    assert np.array_equal(sc, want.sum(axis=1).astype(np.uint32))
    first = np.where(want.any(axis=1), want.argmax(axis=1), 0xFFFFFFFF).astype(np.uint32)
    assert np.array_equal(fs, first)


@pytest.mark.parametrize("name", GROUPS)
def test_term_values_equal_the_reference(dev, name):
    check_values(dev, name)


@pytest.mark.parametrize("name", GROUPS)
def test_satisfaction_bitmaps_equal_bit_0_of_the_reference(dev, name):
    check_bits(dev, name)


@pytest.mark.parametrize("name", FUSION)
def test_fusion_shapes_unfused(dev, monkeypatch, name):
    """The fusion shapes uploaded as given (MG_BV_FUSE=0); the default upload runs in
    the two tests above."""
    monkeypatch.setenv("MG_BV_FUSE", "0")
    check_values(dev, name)
    check_bits(dev, name)
