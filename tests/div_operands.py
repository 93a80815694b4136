"""Directed operands for the device's Knuth-D division (u256.cuh), shared by the
kernel-1 lane tests and kernel 2's case lists."""
import pysem


def division_operand(rng):
    """Operands that reach every branch of the device's Knuth-D division
    (u256.cuh): every divisor length, top-limb ties (qhat = 2^32 - 1), estimates
    that need refinement or an add-back, and wave-mixed quotient lengths."""
    kind = rng.randrange(8)
    bits = rng.randint(1, 256)
    if kind == 0:
        return rng.getrandbits(bits) | (1 << (bits - 1))
    if kind == 1:   # all-ones limbs
        return (1 << bits) - 1
    if kind == 2:   # top limb 0x80000000.., low limbs zero or ones
        k = rng.randint(1, 8)
        return ((1 << 31) << (32 * (k - 1))) | (rng.choice([0, (1 << (32 * (k - 1))) - 1]))
    if kind == 3:   # repeated limb pattern (equal top limbs in u and v)
        limb = rng.getrandbits(32) | (1 << 31)
        return sum(limb << (32 * i) for i in range(rng.randint(1, 8)))
    if kind == 4:   # 2^k +- small
        return max(1, ((1 << rng.randint(1, 255)) + rng.randint(-3, 3)) & pysem.M)
    if kind == 5:   # limbs of 0xffffffff and 0x00000000 mixed
        return sum(rng.choice([0, 0xFFFFFFFF, 1, 0x80000000]) << (32 * i) for i in range(8))
    if kind == 6:
        return rng.getrandbits(256)
    return rng.getrandbits(rng.choice([32, 33, 63, 64, 65, 96, 224, 225]))
