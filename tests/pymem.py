"""Pure-Python model of the reference's concrete memory, copy and SHA3 opcodes (test-only).

Restated from the reference's Python, one function per mutator:

* ``mem_extend`` and its gas: state/machine_state.py:132-191;
* memory reads and writes: state/memory.py:125-208 (a missing byte reads 0, a
  write at or past ``len(memory)`` is dropped, indices are 256-bit);
* calldata: state/calldata.py:46-90,137-146 (K(256, 8, 0) plus one store per
  byte, indices wrap at 2^256);
* the mutators in instructions.py: ``sha3_`` :1013-1051, ``calldatacopy_``
  :806-891, ``codecopy_`` :1074-1098 with ``_code_copy_helper`` :1179,
  ``mload_`` / ``mstore_`` / ``mstore8_`` :1439-1490, ``return_`` :1857-1874,
  ``revert_`` :1899-1934;
* ``StateTransition`` :98-202: the mutator runs on a copy of the state, then
  the table gas is added and ``check_gas_usage_limit`` runs; an exception
  discards the copy.

Memory is a ``bytearray``, words are Python ints, Keccak is the pure-Python
``mythril_amd.keccak.keccak256``.  The lane record's own conventions come from
include/mythgpu.h: a lane that stops (halt, exception, escape) keeps the state
it had before the instruction, ``steps`` counts every instruction but an
escaping one, ``pc`` is an instruction index, and a lane whose memory would
grow past ``mem_cap`` escapes with MG_ESC_MEMORY exactly when the reference
would have completed the instruction (an instruction the reference ends in
OutOfGasException is out of gas whatever the page size).
"""
from functools import lru_cache

import numpy as np

from mythril_amd.keccak import keccak256
from mythril_amd.lanes import (MG_ESC_MEMORY, MG_ESCAPE, MG_EXC_OUT_OF_GAS, MG_HALT_RETURN,
                               MG_HALT_REVERT, MG_HALT_STOP, MG_REC_KECCAK, MG_VMEXC,
                               MSTATE_GAS_LIMIT, LaneBatch, word_to_limbs)

T256 = 1 << 256
M = T256 - 1

# support/opcodes.py: (min, max) table gas
GAS = {0x00: (0, 0), 0x20: (30, 30 + 6 * 8), 0x35: (3, 3), 0x37: (2, 2 + 3 * 768),
       0x39: (2, 2 + 3 * 768), 0x50: (2, 2), 0x51: (3, 96), 0x52: (3, 98), 0x53: (3, 98),
       0x55: (5000, 25000), 0x59: (2, 2), 0xF3: (0, 0), 0xFD: (0, 0)}
GAS.update({0x5F + n: (3, 3) for n in range(1, 33)})
GAS_MEMORY, GAS_MEMORY_QUADRATIC_DENOMINATOR = 3, 512
GAS_SHA3, GAS_SHA3WORD = 30, 6
EMPTY_KECCAK = 0xC5D2460186F7233C927E7DB2DCC703C0E500B653CA82273B7BFAD8045D85A470


def ceil32(x):
    return x if x % 32 == 0 else x + 32 - x % 32


@lru_cache(maxsize=None)
def keccak_int(data: bytes) -> int:
    return int.from_bytes(keccak256(data), "big")


class OutOfGas(Exception):
    pass


class _End(Exception):            # transaction end signal: stop / return / revert
    def __init__(self, status, data=None):
        self.status, self.data = status, data


def disassemble(code: bytes):
    """[(opcode, push argument or None)], one entry per instruction."""
    out, a = [], 0
    while a < len(code):
        op = code[a]
        if 0x60 <= op <= 0x7F:
            n = op - 0x5F
            out.append((op, int.from_bytes(code[a + 1: a + 1 + n].ljust(n, b"\0"), "big")))
            a += n
        else:
            out.append((op, None))
        a += 1
    return out


class _State:
    """What StateTransition copies: machine state, storage, the record log."""

    def __init__(self, memory, stack, storage, records, gmin, gmax, pc):
        self.memory, self.stack, self.storage, self.records = memory, stack, storage, records
        self.gmin, self.gmax, self.pc = gmin, gmax, pc
        self.over = 0      # memory size wanted past the lane's page (bytes not kept)

    def copy(self):
        s = _State(bytearray(self.memory), list(self.stack), dict(self.storage), list(self.records),
                   self.gmin, self.gmax, self.pc)
        return s

    @property
    def msize(self):
        return self.over or len(self.memory)


class Result:
    FIELDS = ("status", "aux", "pc", "steps", "msize", "gas_min", "gas_max", "stack", "memory",
              "storage", "ret", "records")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def outcome(self):
        if self.status == MG_VMEXC:
            return "oog"
        if self.status == MG_ESCAPE:
            return "escape"
        return "normal"


class Model:
    def __init__(self, code, calldata, gas_limit, memory=b"", mem_cap=1024, stack=(), rec_cap=0):
        self.code, self.ins = bytes(code), disassemble(code)
        self.calldata, self.gas_limit = bytes(calldata), gas_limit
        self.mem_cap, self.rec_cap = mem_cap, rec_cap
        assert len(memory) % 32 == 0
        self.s = _State(bytearray(memory), list(stack), {}, [], 0, 0, 0)
        self.steps = 0

    # ---- state/machine_state.py ------------------------------------------------
    def mem_extend(self, s, start, size):
        if s.msize > start + size:                       # calculate_extension_size
            return
        new_size, old_size = ceil32(start + size) // 32, s.msize // 32
        if (new_size - old_size) * 32:
            fee = (new_size * GAS_MEMORY + new_size ** 2 // GAS_MEMORY_QUADRATIC_DENOMINATOR) - \
                  (old_size * GAS_MEMORY + old_size ** 2 // GAS_MEMORY_QUADRATIC_DENOMINATOR)
            s.gmin += fee
            s.gmax += fee
            if s.gmin > MSTATE_GAS_LIMIT:                # check_gas
                raise OutOfGas()
            if new_size * 32 > self.mem_cap:
                s.over = new_size * 32                   # the host's business: no bytes kept
            else:
                s.memory.extend(bytes(new_size * 32 - len(s.memory)))

    def check_gas_usage_limit(self, s):                  # instructions.py:143-160
        if s.gmin > MSTATE_GAS_LIMIT or s.gmin >= self.gas_limit:
            raise OutOfGas()

    # ---- state/memory.py --------------------------------------------------------
    @staticmethod
    def mget(s, k):
        k &= M
        return s.memory[k] if k < len(s.memory) else 0

    @staticmethod
    def mset(s, k, v):
        k &= M
        if k >= s.msize:
            return
        assert 0 <= v <= 0xFF
        if k < len(s.memory):
            s.memory[k] = v

    def cd(self, k):                                     # ConcreteCalldata._load
        k &= M
        return self.calldata[k] if k < len(self.calldata) else 0

    # ---- instructions.py ---------------------------------------------------------
    def mutate(self, s, op, arg):
        st = s.stack
        if 0x60 <= op <= 0x7F:
            st.append(arg)
        elif op == 0x00:
            raise _End(MG_HALT_STOP)
        elif op == 0x50:
            st.pop()
        elif op == 0x59:
            st.append(s.msize)
        elif op == 0x55:
            k, v = st.pop(), st.pop()
            s.storage[k] = v
        elif op == 0x35:                                 # calldataload_
            off = st.pop()
            st.append(int.from_bytes(bytes(self.cd(off + k) for k in range(32)), "big"))
        elif op == 0x51:                                 # mload_
            off = st.pop()
            self.mem_extend(s, off, 32)
            st.append(int.from_bytes(bytes(self.mget(s, off + k) for k in range(32)), "big"))
        elif op == 0x52:                                 # mstore_
            off, v = st.pop(), st.pop()
            try:
                self.mem_extend(s, off, 32)
            except OutOfGas:                             # "except Exception: log.debug"
                pass
            for k, byte in enumerate(v.to_bytes(32, "big")):
                self.mset(s, off + k, byte)
        elif op == 0x53:                                 # mstore8_
            off, v = st.pop(), st.pop()
            self.mem_extend(s, off, 1)
            self.mset(s, off, v % 256)
        elif op == 0x37:                                 # calldatacopy_
            mstart, dstart, size = st.pop(), st.pop(), st.pop()
            if size > 0:
                self.mem_extend(s, mstart, size)
                new_memory = [self.cd(dstart + k) for k in range(self._span(s, size))]
                for k, byte in enumerate(new_memory):
                    self.mset(s, k + mstart, byte)
        elif op == 0x39:                                 # codecopy_ -> _code_copy_helper
            moff, coff, size = st.pop(), st.pop(), st.pop()
            self.mem_extend(s, moff, size)
            for k in range(self._span(s, size)):
                if coff + k + 1 > len(self.code):
                    break
                self.mset(s, moff + k, self.code[coff + k])
        elif op == 0x20:                                 # sha3_ (enable_gas=False)
            index, length = st.pop(), st.pop()
            g = GAS_SHA3 + GAS_SHA3WORD * (ceil32(length) // 32)
            s.gmin += g
            s.gmax += g
            self.check_gas_usage_limit(s)
            self.mem_extend(s, index, length)
            data = bytes(self.mget(s, index + k) for k in range(self._span(s, length)))
            if len(data) == 0:
                st.append(EMPTY_KECCAK)
            else:
                h = keccak_int(data)
                if self.rec_cap:                         # concrete_hashes[data] = hash
                    s.records.append((self.steps, "keccak", data, h))
                st.append(h)
        elif op == 0xF3:                                 # return_
            off, length = st.pop(), st.pop()
            self.mem_extend(s, off, length)
            self.check_gas_usage_limit(s)
            raise _End(MG_HALT_RETURN, bytes(self.mget(s, off + k) for k in range(self._span(s, length))))
        elif op == 0xFD:                                 # revert_
            off, length = st.pop(), st.pop()
            raise _End(MG_HALT_REVERT, bytes(self.mget(s, off + k) for k in range(length)))
        else:
            raise NotImplementedError(hex(op))

    @staticmethod
    def _span(s, size):
        # a state whose memory left the page is discarded (escape): skip its byte loop
        return 0 if s.over else size

    def run(self) -> Result:
        status = aux = 0
        ret = None
        while True:
            op, arg = self.ins[self.s.pc]
            new = self.s.copy()                          # call_on_state_copy
            try:
                self.mutate(new, op, arg)
                if op != 0x20:                           # accumulate_gas (sha3_: enable_gas=False)
                    new.gmin += GAS[op][0]
                    new.gmax += GAS[op][1]
                    self.check_gas_usage_limit(new)
                new.pc += 1
            except OutOfGas:
                self.steps += 1
                status, aux = MG_VMEXC, MG_EXC_OUT_OF_GAS
                break
            except _End as e:
                if e.status == MG_HALT_RETURN and new.over:
                    status, aux = MG_ESCAPE, op | (MG_ESC_MEMORY << 8)
                    break
                self.steps += 1
                status, ret = e.status, e.data
                break
            if new.over:
                status, aux = MG_ESCAPE, op | (MG_ESC_MEMORY << 8)
                break
            self.steps += 1
            self.s = new
        s = self.s
        rec_words = sum(11 + (len(r[2]) + 3) // 4 for r in s.records)
        assert rec_words <= max(self.rec_cap, 0) or not self.rec_cap, "size rec_cap for the cases"
        return Result(status=status, aux=aux, pc=s.pc, steps=self.steps, msize=len(s.memory),
                      gas_min=s.gmin, gas_max=s.gmax, stack=list(s.stack), memory=bytes(s.memory),
                      storage=dict(s.storage), ret=ret, records=list(s.records))


# ---- program builders: operands come from the lane's calldata ------------------------
def _cd(k):   # PUSH1 32k CALLDATALOAD: operand k
    return bytes([0x60, 32 * k, 0x35])


MSIZE, STOP = b"\x59", b"\x00"


def mload_program():      # cd: [offset] -> stack [word, msize]
    return _cd(0) + b"\x51" + MSIZE + STOP


def mstore_program():     # cd: [offset, value, offset - 1] -> stack [msize, word, word', msize]
    return (_cd(1) + _cd(0) + b"\x52" + MSIZE + _cd(0) + b"\x51" + _cd(2) + b"\x51" + MSIZE + STOP)


def mstore8_program():    # cd: [offset, value, offset'] -> stack [msize, word at offset', msize]
    return _cd(1) + _cd(0) + b"\x53" + MSIZE + _cd(2) + b"\x51" + MSIZE + STOP


def calldataload_program():
    """Operands on the initial stack [off2, off1] (the calldata is what is under
    test, down to length 0): slot 0 = word at off1, stack [word at off2, msize]."""
    return b"\x35" + bytes([0x60, 0x00, 0x55]) + b"\x35" + MSIZE + STOP


def calldatacopy_program():
    """Operands on the initial stack [size, src, dst] (dst on top)."""
    return b"\x37" + MSIZE + STOP


# distinctive bytes after the STOP: the code CODECOPY reads
CODE_TAIL = bytes((37 * k + 11) & 0xFF or 0x5B for k in range(61))


def codecopy_program():   # cd: [dst, src, size]
    return _cd(2) + _cd(1) + _cd(0) + b"\x39" + MSIZE + STOP + CODE_TAIL


def sha3_program():       # cd: [off1, len1, off2, len2] -> stack [hash1, hash2, msize]
    return _cd(1) + _cd(0) + b"\x20" + _cd(3) + _cd(2) + b"\x20" + MSIZE + STOP


def return_program(op=0xF3):   # cd: [offset, length]; op 0xfd: REVERT
    return _cd(1) + _cd(0) + bytes([op])


def words(*xs):
    return b"".join((x & M).to_bytes(32, "big") for x in xs)


# ---- lanes <-> model -----------------------------------------------------------------
def set_lane(batch: LaneBatch, i, *, code_id, calldata=b"", gas_limit=10 ** 7, msize=0, stack=()):
    """batch.set_lane plus a preset memory size and stack.  batch.memory[i] is
    left alone: the caller filled it with the pattern and the junk."""
    mem = batch.memory[i].copy()
    batch.set_lane(i, code_id=code_id, calldata=calldata, gas_limit=gas_limit)
    batch.memory[i] = mem
    # non-zero junk past calldata_len too: those bytes are not calldata
    tail = np.arange(len(calldata), batch.shape.calldata_cap)
    batch.calldata[i, len(calldata):] = (tail * 7 + i) % 255 + 1
    batch.msize[i] = msize
    for k, v in enumerate(stack):
        batch.stack[i, k] = word_to_limbs(v)
    batch.sp[i] = len(stack)


def fill_memory(batch: LaneBatch, seed):
    """Every byte non-zero and random: below msize it is the lane's pattern, from
    msize up to mem_cap junk that an extension has to clear."""
    rng = np.random.default_rng(seed)
    batch.memory[...] = rng.integers(1, 256, size=batch.memory.shape, dtype=np.uint8)


def model_lane(batch: LaneBatch, codes, i) -> Result:
    ms = int(batch.msize[i])
    return Model(codes[int(batch.code_id[i])], bytes(batch.calldata[i, : int(batch.calldata_len[i])]),
                 int(batch.gas_limit[i]), memory=bytes(batch.memory[i, :ms]),
                 mem_cap=batch.shape.mem_cap, stack=batch.stack_words(i),
                 rec_cap=batch.shape.rec_cap).run()


def record_words(records):
    """The MG_REC_KECCAK layout of include/mythgpu.h: kind, input length, step,
    the hash as 8 little-endian limbs, then the input as big-endian words with
    the last one zero-padded."""
    out = []
    for step, _, data, h in records:
        out += [MG_REC_KECCAK, len(data), step] + [int(x) for x in word_to_limbs(h)]
        padded = data + bytes(-len(data) % 4)
        out += [int.from_bytes(padded[k: k + 4], "big") for k in range(0, len(padded), 4)]
    return out


def lane_diff(out: LaneBatch, i, r: Result):
    """Fields of lane i of a run image that differ from the model's result."""
    bad = []
    for f, want in (("status", r.status), ("aux", r.aux), ("pc", r.pc), ("steps", r.steps),
                    ("msize", r.msize), ("gas_min", r.gas_min), ("gas_max", r.gas_max),
                    ("sp", len(r.stack))):
        if int(getattr(out, f)[i]) != want:
            bad.append(f"lane {i}: {f} {int(getattr(out, f)[i])} != model {want}")
    if out.stack_words(i) != r.stack:
        bad.append(f"lane {i}: stack {[hex(x) for x in out.stack_words(i)]} != model "
                   f"{[hex(x) for x in r.stack]}")
    if out.memory_bytes(i) != r.memory:
        m = out.memory_bytes(i)
        k = next((k for k in range(min(len(m), len(r.memory))) if m[k] != r.memory[k]), -1)
        bad.append(f"lane {i}: memory differs from the model's at byte {k}")
    if out.storage_dict(i, drop_zero=False) != r.storage:
        bad.append(f"lane {i}: storage {out.storage_dict(i, drop_zero=False)} != model {r.storage}")
    if r.status in (MG_HALT_RETURN, MG_HALT_REVERT):
        if int(out.ret_len[i]) != len(r.ret) or out.return_data(i) != r.ret:
            bad.append(f"lane {i}: return data differs from the model's")
    if out.shape.rec_cap:
        if out.records(i) != r.records:
            bad.append(f"lane {i}: keccak records differ from the model's")
        elif [int(x) for x in out.rec[i, : int(out.rec_len[i])]] != record_words(r.records):
            bad.append(f"lane {i}: raw record words differ from the model's (payload padding?)")
    return bad
