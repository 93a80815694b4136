"""A Python model of mg_explore_check_fn (include/mythgpu.h): tests/pathmodel.py's
contract plus the two rules that read the models' uninterpreted functions.

Written from the header's rules with Python integers, like pathmodel.py, whose
lane reader, operator table and unknown signal it shares; it never goes through
the host's decoder (``symbolic._Decoder``).  A table is read at ``(k0, k1)``:
``keccak256_<w>`` at ``(x mod 2^256, x >> 256)``, ``Power`` at ``(base, exponent)``.

``check(image, paths, pool, bindings, lane_binding, functions, allowed, first, n)``
gives ``(first_sat uint32[n], sat_bits uint64[n, words])``; ``functions`` is an
object with mg_path_functions' fields, or None for nothing bound.
"""
from __future__ import annotations

import numpy as np

from mythril_amd import abi
from mythril_amd.smt.semantics import apply_op
from pathmodel import BIN, BYTE, CONST, M256, NO_MODEL, UNBOUND, UNKNOWN, _Lane, _Unknown, _word

POWER = 0x0A
LEAVES = abi.MG_PATH_KECCAK_LEAVES


class Functions:
    """mg_path_functions as plain Python: tab_power and {width: table}."""

    def __init__(self, functions=None):
        self.tab_power, self.keccak = UNBOUND, {}
        if functions is not None:
            self.tab_power = int(functions.tab_power)
            for j in range(int(functions.n_keccak)):
                self.keccak[int(functions.keccak_bits[j])] = int(functions.keccak_tab[j])

    def table(self, bits: int) -> int:
        return self.keccak.get(bits, UNBOUND)


def leaves(lane: _Lane, k: int, y: int, bits: int):
    """The leaves [(ref, width)] of KECCAK node k's input, high part first; raises
    _Unknown for a tree the contract does not take."""
    out = []

    def ref(parent, r, width):
        if not 1 <= width <= 512:
            raise _Unknown("part width")
        if r & CONST:
            if width > 256 or (r & ~CONST) >= lane.nc:
                raise _Unknown("constant part")
            out.append((r, width))
            return
        if r >= parent:
            raise _Unknown("part not below its referrer")
        x, ny, nz, w = lane.rows[r]
        if x >> 8 != width:
            raise _Unknown("part width mismatch")
        if x & 0xFF == abi.MG_SYM_CONCAT and width > 256:
            wy, wz = w & 0xFFFF, w >> 16
            if wy + wz != width:
                raise _Unknown("concat widths")
            ref(r, ny, wy)
            ref(r, nz, wz)
        elif width > 256:
            raise _Unknown("wide node")
        else:
            out.append((r, width))

    ref(k, y, bits)
    if len(out) > LEAVES:
        raise _Unknown("too many leaves")
    return out


def cone(lane: _Lane, path_row, bind, fn: Functions):
    """The nodes the path needs, ascending; raises _Unknown for an unknown lane."""
    nn = lane.nn
    if nn > lane.node_cap or nn > abi.MG_PATH_MAX_NODES:
        raise _Unknown("arena size")
    marked = set()
    for entry in path_row:
        tag = int(entry) >> 1
        if tag == 0 or tag - 1 >= nn:
            raise _Unknown("condition tag")
        marked.add(tag - 1)
    cd = bind.var_cdsize != UNBOUND and bind.tab_calldata != UNBOUND

    def ref(k, r):
        if r & CONST:
            if (r & ~CONST) >= lane.nc:
                raise _Unknown("constant ref")
        elif r >= k:
            raise _Unknown("node ref")
        else:
            marked.add(r)

    for k in range(nn - 1, -1, -1):
        if k not in marked:
            continue
        x, y, z, w = lane.rows[k]
        kind, width = x & 0xFF, x >> 8
        if not 1 <= width <= 256:               # a wide CONCAT has no value of its own
            raise _Unknown("width")
        if kind == abi.MG_SYM_CDSIZE:
            ok = width == 256 and bind.var_cdsize != UNBOUND
        elif kind == abi.MG_SYM_ENV:
            ok = width == 256 and w < abi.MG_ENV_WORDS and bind.var_env[w] != UNBOUND
        elif kind == abi.MG_SYM_CDLOAD:
            ok = width == 256 and cd
            if ok:
                ref(k, y)
        elif kind == abi.MG_SYM_CDBYTE:
            ok = width == 8 and cd
        elif kind == abi.MG_SYM_CDBYTEX:
            ok = width == 8 and cd
            if ok:
                ref(k, y)
        elif kind == abi.MG_SYM_BIN:
            ok = w in BIN or w == BYTE or (w == POWER and width == 256 and fn.tab_power != UNBOUND)
            if ok:
                ref(k, y)
                ref(k, z)
                if w == BYTE:
                    ok = bool(y & CONST) and lane.const(y) < 32
        elif kind == abi.MG_SYM_UN:
            ok = w in (0x15, 0x19)
            if ok:
                ref(k, y)
        elif kind == abi.MG_SYM_EXTRACT:
            hi, lo = w >> 16, w & 0xFFFF
            ok = not y & CONST and y < k and lo <= hi and width == hi - lo + 1 and hi < (lane.rows[y][0] >> 8)
            if ok:
                marked.add(y)
        elif kind == abi.MG_SYM_CONCAT:
            wy, wz = w & 0xFFFF, w >> 16
            ok = wy >= 1 and wz >= 1 and wy + wz == width
            if ok:
                ref(k, y)
                ref(k, z)
        elif kind == abi.MG_SYM_SLOAD:
            ok = width == 256 and z <= lane.sc and not (lane.symstore and bind.tab_storage == UNBOUND)
            if ok:
                ref(k, y)
                for e in range(z):
                    for tag, _ in lane.entry(e):
                        if tag:
                            if tag - 1 >= k:
                                raise _Unknown("chain tag")
                            marked.add(tag - 1)
        elif kind == abi.MG_SYM_KECCAK:
            ok = width == 256 and 1 <= w <= 512 and fn.table(w) != UNBOUND
            if ok:
                marked.update(r for r, _ in leaves(lane, k, y, w) if not r & CONST)
        else:                       # TERM, MLOADK, MSTOREK, BALANCE, anything else
            ok = False
        if not ok:
            raise _Unknown(f"node {k}")
    return sorted(marked)


class _Pool:
    """A ModelPool's values and tables as Python ints, read on demand."""

    def __init__(self, pool):
        self.pool = pool
        self._tabs = {}

    def var(self, v: int, m: int) -> int:
        return _word(self.pool.values[v, m])

    def table(self, t: int, m: int, k0: int, k1: int, width: int) -> int:
        tm = self._tabs.get((t, m))
        if tm is None:
            p = self.pool
            s, c = int(p.tab_start[t, m]), int(p.tab_count[t, m])
            entries = {}
            for row in p.tab_entries[s:s + c]:
                entries.setdefault((_word(row[:8]), _word(row[8:16])), _word(row[16:24]))   # first match wins
            tm = self._tabs[(t, m)] = (entries, _word(p.tab_default[t, m, :8]))
        return tm[0].get((k0, k1), tm[1]) & ((1 << width) - 1)


def values(lane: _Lane, nodes, bind, fn: Functions, pool: _Pool, m: int) -> dict:
    """node -> value under model m, for the cone's nodes in ascending order."""
    val = {}

    def ref(r):
        return lane.const(r) if r & CONST else val[r]

    def cd_byte(i, size):
        return pool.table(bind.tab_calldata, m, i, 0, 8) if apply_op("bvslt", 1, (i, size), (256, 256)) else 0

    for k in nodes:
        x, y, z, w = lane.rows[k]
        kind, width = x & 0xFF, x >> 8
        if kind == abi.MG_SYM_CDSIZE:
            v = pool.var(bind.var_cdsize, m)
        elif kind == abi.MG_SYM_ENV:
            v = pool.var(bind.var_env[w], m)
        elif kind == abi.MG_SYM_CDLOAD:
            size, off = pool.var(bind.var_cdsize, m), ref(y)
            v = 0
            for j in range(32):
                v = v << 8 | cd_byte((off + j) & M256, size)
        elif kind == abi.MG_SYM_CDBYTE:
            v = cd_byte(w, pool.var(bind.var_cdsize, m))
        elif kind == abi.MG_SYM_CDBYTEX:
            v = cd_byte((ref(y) + w) & M256, pool.var(bind.var_cdsize, m))
        elif kind == abi.MG_SYM_BIN:
            a, c = ref(y), ref(z)
            if w == BYTE:
                v = apply_op("extract", 8, (c,), (256,), ((31 - a) * 8 + 7, (31 - a) * 8))
            elif w == POWER:
                v = pool.table(fn.tab_power, m, a, c, 256)          # (base, exponent)
            else:
                op, swap = BIN[w]
                v = apply_op(op, 256, (c, a) if swap else (a, c), (256, 256))
        elif kind == abi.MG_SYM_UN:
            a = ref(y)
            v = int(a == 0) if w == 0x15 else apply_op("bvnot", width, (a,), (width,))
        elif kind == abi.MG_SYM_EXTRACT:
            v = apply_op("extract", width, (val[y],), (lane.rows[y][0] >> 8,), (w >> 16, w & 0xFFFF))
        elif kind == abi.MG_SYM_CONCAT:
            wy, wz = w & 0xFFFF, w >> 16
            v = apply_op("concat", width, (ref(y) & ((1 << wy) - 1), ref(z) & ((1 << wz) - 1)), (wy, wz))
        elif kind == abi.MG_SYM_KECCAK:
            xin = 0
            for r, pw in leaves(lane, k, y, w):                     # high part first
                xin = xin << pw | (ref(r) & ((1 << pw) - 1))
            v = pool.table(fn.table(w), m, xin & M256, xin >> 256, 256)
        else:                       # MG_SYM_SLOAD: newest entry first
            key = ref(y)
            for e in range(z - 1, -1, -1):
                (kt, kv), (vt, vv) = lane.entry(e)
                if (val[kt - 1] if kt else kv) == key:
                    v = val[vt - 1] if vt else vv
                    break
            else:
                v = pool.table(bind.tab_storage, m, key, 0, 256) if lane.symstore else 0
        val[k] = v & ((1 << width) - 1)
    return val


def _cone_of(b, i, path_row, root, bindings, lane_binding, fn):
    if root >= len(lane_binding):
        raise _Unknown("root")
    bi = int(lane_binding[root])
    if bi == UNBOUND or bi >= len(bindings):
        raise _Unknown("lineage")
    lane = _Lane(b, i)
    return lane, bi, cone(lane, path_row, bindings[bi], fn)


def lane_unknown(b, i: int, path_row, root: int, bindings, lane_binding, functions=None) -> bool:
    """Whether lane i is MG_PATH_UNKNOWN (no model needed)."""
    try:
        _cone_of(b, i, path_row, root, bindings, lane_binding, Functions(functions))
    except _Unknown:
        return True
    return False


def check(b, paths, pool, bindings, lane_binding, functions=None, allowed=None, first: int = 0, n: int = None):
    path, path_len, root = paths
    n = len(path_len) - first if n is None else n
    fn = Functions(functions)
    n_models = pool.n_models
    words = (n_models + 63) // 64
    first_sat = np.full(n, NO_MODEL, dtype=np.uint32)
    bits = np.zeros((n, words), dtype=np.uint64)
    P = _Pool(pool)
    for j in range(n):
        i = first + j
        row = [int(e) for e in path[i, :int(path_len[i])]] if int(path_len[i]) <= path.shape[1] else None
        try:
            if row is None:
                raise _Unknown("path length")
            lane, bi, nodes = _cone_of(b, i, row, int(root[i]), bindings, lane_binding, fn)
        except _Unknown:
            first_sat[j] = UNKNOWN
            continue
        for m in range(n_models):
            if allowed is not None and not (int(allowed[bi, m >> 6]) >> (m & 63)) & 1:
                continue
            val = values(lane, nodes, bindings[bi], fn, P, m)
            if all((val[(e >> 1) - 1] != 0) == bool(e & 1) for e in row):
                bits[j, m >> 6] |= np.uint64(1 << (m & 63))
                if first_sat[j] == NO_MODEL:
                    first_sat[j] = m
    return first_sat, bits
