"""The lane-transfer layer of libmythgpu.so on an MI355X -- XferPlan, xfer_up /
xfer_down, the LDS-tiled transposes k_xfer_scatter / k_xfer_gather, the range and
`live` entry points and the symbolic / taint plane transfers -- against the plain
NumPy model of the contract (tests/xfermodel.py), bit for bit.

The device shape gives every field whole 64-lane x 64-dword tiles plus a ragged
edge (200 lanes: the last tile holds 8; stack W = 8 with 20 units, memory 72
dwords, calldata 17, storage W = 16 with 6 units, trace 70, records 130, arena
nodes W = 4 with 35 units, constants W = 8 with 9, object masks W = 2 with 40).

a. a fixed-seed sequence of uploads and downloads (live or not, full or slim
   host images, ranges that start and end inside tiles) checked against the
   model after every step, over whole capacities;
b. a layout anchor: words, memory bytes, calldata bytes and storage entries of a
   live range upload are read by kernel 1 (a round trip cannot see an error
   made the same way in both directions);
c. a partial upload into the resident reset image (mg_lanes_reset,
   mg_run_batches) and its freshness rule;
d. symbolic and taint lanes stepped on dirty planes equal the same lanes on
   the zeroed planes of a new allocation;
e. every documented refusal leaves the device image and the context intact,
   NULL fields are skipped on download, and a live download refuses a NULL
   count array whose rows are requested;
f. the path planes (mg_explore_upload, mg_explore_download): ranges inside and
   across tiles, zeros at and above path_len in both directions, the refusals.
"""
import ctypes
import dataclasses
from copy import copy

import numpy as np
import pytest

import symcases
from mythril_amd import native
from mythril_amd.device import GpuDevice
from mythril_amd.lanes import (MG_FENT_NONE, MG_FORK, MG_HALT_RETURN, MG_HALT_REVERT, MG_HALT_STOP,
                               MG_SYM_MLOADK, MG_SYM_MSTOREK, MG_TAINT_OBJ0, LaneBatch, LaneShape, diff_batches,
                               limbs_to_word, word_to_limbs)
from mythril_amd.laser import BreadthFirstSearchStrategy, LaserEVM
from mythril_amd.laser import symbolic as sym
from mythril_amd.laser.opcodes import OPCODES
from oracle.evm_ref import OracleEVM
from oracle_device import OracleDevice
from xfermodel import DeviceImage, live_diff, saturated, sentinel_filled, whole_diff

pytestmark = pytest.mark.gpu

N = 200
CAPS = dict(stack_cap=20, mem_cap=288, calldata_cap=68, storage_cap=6, trace_cap=70, rec_cap=130)
SLIM = dict(stack_cap=12, mem_cap=96, calldata_cap=36, storage_cap=3, rec_cap=50)
PLANES = {"plain": ({}, {}), "symbolic": (dict(node_cap=35, const_cap=9), dict(node_cap=20, const_cap=5)),
          "taint": (dict(obj_cap=40), dict(obj_cap=20))}
RANGES = [(0, 200), (0, 1), (199, 1), (37, 1), (37, 27), (63, 2), (64, 64), (1, 198), (130, 70)]
# the range's largest count per upload: tile edges of each field's unit width
MAXIMA = {"sp": (0, 1, 7, 8, 9, 16, 17, 20), "storage_count": (0, 1, 3, 4, 5, 6),
          "msize": (0, 32, 224, 256, 288), "trace_len": (0, 1, 63, 64, 65, 70),
          "rec_len": (0, 1, 64, 65, 129, 130), "n_nodes": (0, 1, 15, 16, 17, 35), "n_consts": (0, 1, 8, 9),
          "n_obj": (7, 8, 32, 33, 40)}
CAP_OF = {"sp": "stack_cap", "storage_count": "storage_cap", "msize": "mem_cap", "trace_len": "trace_cap",
          "rec_len": "rec_cap", "n_nodes": "node_cap", "n_consts": "const_cap", "n_obj": "obj_cap"}


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def _shape(kind, n=N, slim=False, trace_cap=None):
    caps = dict(CAPS)
    if slim:
        caps.update(SLIM)
        caps["trace_cap"] = trace_cap or 0
    caps.update(PLANES[kind][1 if slim else 0])
    return LaneShape(n=n, **caps)


def _distinct_bytes(rng, arr):
    """Random bytes, the four of every dword all different (a missing or a wrong
    byte swap cannot go unseen)."""
    n, cap = arr.shape
    base = rng.integers(0, 256, size=(n, cap // 4, 1))
    off = np.arange(4) * 64 + rng.integers(0, 32, size=(n, cap // 4, 4))
    arr[...] = ((base + off) % 256).astype(np.uint8).reshape(n, cap)


def _saturated(shape, rng, code_id):
    b = saturated(shape, rng, code_id)
    _distinct_bytes(rng, b.memory)
    _distinct_bytes(rng, b.calldata)
    return b


def _host(shape, rng, code_id, lo, n, maxima):
    """Random rows everywhere; lanes [lo, lo + n) get counts up to `maxima`, one
    lane of the range at the maximum; never MG_RUNNING."""
    b = _saturated(shape, rng, code_id)
    b.status[:] = rng.choice([MG_HALT_STOP, MG_HALT_RETURN, MG_HALT_REVERT], size=shape.n)
    b.calldata_len[:] = rng.integers(0, shape.calldata_cap + 1, size=shape.n)
    if shape.obj_cap:
        b.n_atoms[:] = rng.integers(0, 65, size=shape.n)
    for count, top in maxima.items():
        step = 32 if count == "msize" else 1
        low = MG_TAINT_OBJ0 if count == "n_obj" else 0
        c = getattr(b, count)
        c[lo:lo + n] = rng.integers(low // step, top // step + 1, size=n) * step
        c[lo + int(rng.integers(0, n))] = top
    return b


def _maxima(shape, turn):
    """An upload's range maxima: each field cycles through the values of its set
    that the host's capacities allow (`turn` counts per field and capacity, the
    fields out of step with each other)."""
    out = {}
    for k, (count, values) in enumerate(MAXIMA.items()):
        cap = getattr(shape, CAP_OF[count])
        if not cap:
            continue
        ok = [v for v in values if v <= cap]
        t = turn.setdefault((count, cap), k)
        turn[(count, cap)] = t + 1
        out[count] = ok[t % len(ok)]
    return out


def _full(dev, shape):
    out = sentinel_filled(shape)
    dev.download(out)
    return out


def _expected_full(model):
    """What a full non-live download shows of the model's image: everything, but
    the arena and the object table only below the device's largest counts."""
    out = sentinel_filled(model.shape)
    model.download(out, 0, model.shape.n)
    return out


def _code(dev):
    return dev.load_code(bytes.fromhex("00"))


# ------------------------------------------------------------------ a. sequence
@pytest.mark.parametrize("kind", ["plain", "symbolic", "taint"])
def test_transfer_sequence_equals_the_model(dev, kind):
    rng = np.random.default_rng(0x7AFE + len(kind))
    shape = _shape(kind)
    cid = _code(dev)
    dev.alloc(shape)
    model = DeviceImage(shape)
    base = _saturated(shape, rng, cid)
    dev.upload(base)
    model.upload(base, 0, N)
    assert whole_diff(_full(dev, shape), _expected_full(model)) == []
    turn = {}
    seen_max = {c: set() for c in MAXIMA}
    seen = set()
    for step in range(54):
        first, n = RANGES[step % len(RANGES)]
        up = (step // len(RANGES)) % 2 == 0 or step % 4 == 1
        live = bool((step // 2 + step // len(RANGES)) % 2)
        slim = step % 3 == 1
        whole_batch = step % 5 in (2, 3)              # upload(batch, first) / download(batch, first): host lane 0
        hn = n if whole_batch else N
        hshape = _shape(kind, hn, slim, trace_cap=20 if step % 2 else 0)
        lo = 0 if whole_batch else first
        seen.add((first, n, up))
        tag = (step, "up" if up else "down", first, n, "live" if live else "", "slim" if slim else "",
               "batch" if whole_batch else "range")
        if up:
            maxima = _maxima(hshape, turn)
            for c, v in maxima.items():
                seen_max[c].add(v)
            host = _host(hshape, rng, cid, lo, n, maxima)
            if whole_batch:
                dev.upload(host, first)
            else:
                dev.upload_range(host, first, n, live=live)
            model.upload(host, first, n, host_first=lo, live=live)
            # whole capacities: neighbours of the range's tiles and rows above the bounds kept
            after = _full(dev, shape)
            assert whole_diff(after, _expected_full(model)) == [], tag
            if step % 6 == 0 and not whole_batch:
                # mg_lanes_upload and mg_lanes_upload_live of one image leave one device image
                dev.upload_range(host, first, n, live=not live)
                assert whole_diff(_full(dev, shape), after) == [], tag
        else:
            got, want = sentinel_filled(hshape), sentinel_filled(hshape)
            if whole_batch:
                dev.download(got, first)
            else:
                dev.download_range(got, first, n, live=live)
            model.download(want, first, n, host_first=lo, live=live and not whole_batch)
            assert whole_diff(got, want) == [], tag
    # the sequence covered what it is there for
    assert {(f, n) for f, n, up in seen if up} == set(RANGES) == {(f, n) for f, n, up in seen if not up}
    for c, values in seen_max.items():
        if getattr(shape, CAP_OF[c]):
            assert values == set(MAXIMA[c]), (c, values)


# -------------------------------------------------------------- b. layout anchor
def test_kernel_reads_what_a_live_range_upload_wrote(dev):
    rng = np.random.default_rng(0xA7C4)
    shape = _shape("plain")
    code = bytes.fromhex("600051" "600151" "600035" "600335" "600054" "00")
    cid = dev.load_code(code)
    dev.alloc(shape)
    base = _saturated(shape, rng, cid)
    dev.upload(base)
    first, n = 37, 70
    b = base.copy()
    words, stored = {}, {}
    for i in range(first, first + n):
        cd = bytes(rng.integers(0, 256, size=40, dtype=np.uint8))
        stored[i] = int.from_bytes(bytes(rng.integers(0, 256, size=32, dtype=np.uint8)), "big")
        other = int.from_bytes(bytes(rng.integers(0, 256, size=32, dtype=np.uint8)), "big")
        b.set_lane(i, code_id=cid, calldata=cd, address=0xC0DE, caller=i, gas_limit=10 ** 6,
                   storage={5: other, 0: stored[i]})
        words[i] = [int.from_bytes(bytes(rng.integers(0, 256, size=32, dtype=np.uint8)), "big") for _ in range(2)]
        b.sp[i] = 2
        b.stack[i, 0], b.stack[i, 1] = word_to_limbs(words[i][0]), word_to_limbs(words[i][1])
        b.msize[i] = 64
        b.trace_len[i] = b.rec_len[i] = 0
    _distinct_bytes(rng, b.memory[first:first + n])
    dev.upload_range(b, first, n, live=True)
    st = dev.step()
    out = _full(dev, shape)
    assert st.lane_steps == 11 * n
    for i in range(first, first + n):
        mem, cd = bytes(b.memory[i, :64]), bytes(b.calldata[i, :40])
        want = words[i] + [int.from_bytes(mem[0:32], "big"), int.from_bytes(mem[1:33], "big"),
                           int.from_bytes(cd[0:32], "big"), int.from_bytes(cd[3:35], "big"), stored[i]]
        assert int(out.status[i]) == MG_HALT_STOP and int(out.sp[i]) == 7, i
        assert [limbs_to_word(out.stack[i, k]) for k in range(7)] == want, i
        assert bytes(out.memory[i, :64]) == mem and int(out.msize[i]) == 64
    # rows above what the lanes wrote, and every lane outside the range, over whole capacities
    inside = range(first, first + n)
    assert np.array_equal(out.stack[inside, 7:], base.stack[inside, 7:])
    assert np.array_equal(out.memory[inside, 64:], base.memory[inside, 64:])
    assert np.array_equal(out.storage[inside, 2:], base.storage[inside, 2:])
    outside = [i for i in range(N) if i not in inside]
    assert whole_diff(out, base, lanes=outside) == []


# ------------------------------------------------- c. partial upload, reset image
# PUSH 1, PUSH 2, ADD, POP | PUSH 0, SLOAD, PUSH 1, ADD, PUSH 0, SSTORE, PUSH 1, SLOAD, PUSH 9, SSTORE, STOP
RESET_CODES = ["6001600201" "50" "600054" "600101" "600055" "600154" "600955" "00",
               # CALLDATALOAD 0, DUP1, PUSH 0, MSTORE, PUSH 3, SLOAD, ADD, PUSH 3, SSTORE, STOP
               "600035" "80" "600052" "600354" "01" "600355" "00"]


def _fresh(rng, cids, pcs, salt):
    b = LaneBatch(_shape("plain"))
    for i in range(N):
        k = int(rng.integers(0, len(cids)))
        b.set_lane(i, code_id=cids[k], calldata=bytes(rng.integers(0, 256, size=32, dtype=np.uint8)),
                   address=0xC0DE, caller=salt + i, gas_limit=int(rng.integers(10 ** 5, 10 ** 6)),
                   storage={key: int(rng.integers(1, 1 << 62)) + salt for key in (0, 1, 3)[:int(rng.integers(0, 4))]})
        b.pc[i] = pcs[k]
        b.gas_min[i] = b.gas_max[i] = int(rng.integers(0, 1000)) + salt
    return b


def test_partial_upload_into_the_reset_image(dev):
    rng = np.random.default_rng(0x5E7)
    codes = [bytes.fromhex(c) for c in RESET_CODES]
    cids = [dev.load_code(c) for c in codes]
    o = OracleEVM()
    oids = [o.load_code(c) for c in codes]
    shape = _shape("plain")
    dev.alloc(shape)
    whole = _fresh(rng, cids, (0, 0), 0)
    other = _fresh(rng, cids, (4, 0), 5000)          # another pc, other storage, other gas
    first, n = 63, 70
    dev.upload(whole)
    dev.upload_range(other, first, n)
    comp = whole.copy()
    for f in ("code_id", "pc", "gas_min", "gas_max", "gas_limit", "calldata", "calldata_len", "env", "storage",
              "storage_count"):
        getattr(comp, f)[first:first + n] = getattr(other, f)[first:first + n]
    ref = comp.copy()
    remap = dict(zip(cids, oids))
    ref.code_id[:] = [remap[int(c)] for c in comp.code_id]
    o.run(ref)
    ref.code_id[:] = comp.code_id

    def result():
        out = LaneBatch(shape)
        dev.download(out)
        return out
    dev.reset()
    dev.step()
    assert diff_batches(result(), ref) == []
    # the resident image (the uploads' second destinations, at first > 0) restores the composite
    dev.run_batches(2)
    assert diff_batches(result(), ref) == []
    # the first code takes 15 steps from pc 0 and 11 from pc 4: the range runs from its own pc
    assert (ref.status == MG_HALT_STOP).all() and 15 in ref.steps[:first] and 15 not in ref.steps[first:first + n]
    # a partial upload of lanes that are not fresh: no reset until a fresh whole upload
    used = result()
    dev.upload_range(used, first, n)
    with pytest.raises(native.MythGpuError, match=f"rc={native.MG_ESTATE}"):
        dev.reset()
    dev.upload(comp)
    dev.reset()
    dev.step()
    assert diff_batches(result(), ref) == []


# ------------------------------------------------------- d. dirty planes: taint
def test_taint_lanes_on_dirty_planes_match_the_restatement(dev):
    import test_gpu_taint as t
    hook = [0, 0, 0, 0]
    for op in ("STOP", "RETURN"):
        hook[OPCODES[op] >> 6] |= 1 << (OPCODES[op] & 63)
    rng = np.random.default_rng(0x7A1)
    b0, codes, n_c2 = t._batch(obj_cap=16)           # a small table: handle compaction runs
    t._load(dev, b0, codes, n_c2)
    ref = b0.copy()
    ora = OracleDevice()
    oids = [ora.load_code(c) for c in codes]         # code ids are each side's own
    ref.code_id[:n_c2] = oids[0]
    for k in range(b0.n - n_c2):
        ref.code_id[n_c2 + k] = oids[1 + k // 2]
    ora.alloc(b0.shape)
    ora.set_taint_program(t.ACTIONS)
    ora.upload(ref)
    for _ in range(3):
        ora.step(hook, max_steps=400)
    ora.download(ref)
    dev.alloc(b0.shape)
    dev.set_taint_program(t.ACTIONS)
    # twice: the second pass also finds the device's own remap table used
    for _ in range(2):
        dev.upload(saturated(b0.shape, rng, int(b0.code_id[0])))
        b = b0.copy()
        dev.upload(b)
        for _ in range(3):
            dev.step(hook, max_steps=400)
        dev.download(b)
        for f in ("pc", "sp", "status", "aux", "steps", "gas_min", "gas_max", "rec_len", "n_atoms", "sink",
                  "ymask", "tflags"):
            assert np.array_equal(getattr(b, f), getattr(ref, f)), f
        for i in range(b.n):
            assert np.array_equal(b.rec[i, : int(b.rec_len[i])], ref.rec[i, : int(ref.rec_len[i])]), i
            assert t._partition(b, i) == t._partition(ref, i), i
            assert np.array_equal(b.stack[i, : int(b.sp[i])], ref.stack[i, : int(ref.sp[i])]), i
    assert int(b.status[n_c2 + 14]) == 6             # the compaction loop ran (until out of gas)


# ---------------------------------------------------- d. dirty planes: symbolic
def _dirty_against_clean(dev, name, rng, rounds):
    """The co-simulation loop of test_gpu_symbolic over `rounds` BFS rounds of a
    symbolic call into `name`, every round stepped twice: on planes a saturated
    upload dirtied, and on the zeroed planes of a new allocation.  Returns the
    tallies of what the compared runs contained."""
    import test_gpu_symbolic as ts
    tally = dict(rounds=0, lanes=0, forks=0, symkeccak=0, mtag=0, sttag=0, memk=0)
    ws, addr = symcases.deploy(dev, name)
    vm = LaserEVM(requires_statespace=False, device=dev, strategy=BreadthFirstSearchStrategy)
    queue = [ts._initial(ws, addr)]
    while queue and tally["rounds"] < rounds:
        states, queue = queue[:32], queue[32:]
        shape = vm._shape(states)
        b = LaneBatch(shape)
        for i, s in enumerate(states):
            vm._pack(b, i, s)
            b.steps[i] = 0
        up = b.copy()
        dev.alloc(shape)                             # dirty: every row and plane random, every count full
        dev.upload(saturated(shape, rng, int(b.code_id[0])))
        dev.upload(up)
        dev.step()
        dirty = LaneBatch(shape)
        dev.download(dirty)
        dev.alloc(shape)                             # clean
        dev.upload(up)
        dev.step()
        dev.download(b)
        assert live_diff(b, dirty) == [], (name, tally)
        tally["rounds"] += 1
        tally["lanes"] += len(states)
        for i, s0 in enumerate(states):
            tally["symkeccak"] += sum(1 for r in b.records(i) if r[1] == "symkeccak")
            tally["mtag"] += int(np.count_nonzero(b.mtag[i, :int(b.msize[i])]))
            tally["sttag"] += int(np.count_nonzero(b.sttag[i, :int(b.storage_count[i])]))
            kinds = b.node[i, :int(b.n_nodes[i]), 0] & 0xFF
            tally["memk"] += int(np.isin(kinds, (MG_SYM_MSTOREK, MG_SYM_MLOADK)).sum())
            if int(b.status[i]) == MG_FORK:
                tally["forks"] += 1
                got = vm._materialise(b, i, copy(s0))
                queue.extend(x for x in sym.jumpi_successors(got) if sym.lane_eligible(x))
    return tally


SYM_CASES = ("overflow.sol.o", "symkey_sha3", symcases.FIELD[0])


def test_symbolic_lanes_on_dirty_planes_equal_clean_ones(dev):
    rng = np.random.default_rng(0x5B1)
    total = {}
    for name in SYM_CASES:
        for k, v in _dirty_against_clean(dev, name, rng, rounds=4).items():
            total[k] = total.get(k, 0) + v
    assert total["forks"] >= 3 and total["symkeccak"] >= 1 and total["mtag"] >= 1 and total["sttag"] >= 1 and \
        total["memk"] >= 1, total


# --------------------------------------------------- e. refusals and NULL fields
def _soa(batch, lo, n):
    return batch.soa_range(lo, n)


def test_refusals_leave_the_device_image_and_the_context_intact(dev):
    rng = np.random.default_rng(0xE44)
    shape = LaneShape(n=N, **CAPS, node_cap=35, const_cap=9, obj_cap=40)
    cid = _code(dev)
    dev.alloc(shape)
    base = _saturated(shape, rng, cid)
    dev.upload(base)
    lib, ctx = dev.lib, dev.ctx
    n = 10
    good = _host(shape, rng, cid, 20, n, {"sp": 5, "msize": 64, "storage_count": 2})

    def lanes(host, first, cnt, lo=20, patch=None, fn="mg_lanes_upload"):
        s = _soa(host, lo, n)
        if patch:
            patch(s)
        return getattr(lib, fn)(ctx, ctypes.addressof(s), first, cnt)

    def with_lane(**fields):
        h = good.copy()
        for f, v in fields.items():
            getattr(h, f)[23] = v
        return h

    def setattr_(name, value):
        return lambda s: setattr(s, name, value)

    EINVAL, ENOCODE = native.MG_EINVAL, native.MG_ENOCODE
    big = LaneBatch(LaneShape(n=N, **{**CAPS, "stack_cap": 21}))
    big.code_id[:] = cid
    cases = [
        ("range past the batch", lambda: lanes(good, 195, n), EINVAL),
        ("download past the batch", lambda: lanes(good.copy(), 195, n, fn="mg_lanes_download"), EINVAL),
        ("h->n != n", lambda: lanes(good, 20, n - 1), EINVAL),
        ("host caps above the device's", lambda: lanes(big, 20, n), EINVAL),
        ("mem_cap % 4", lambda: lanes(good, 20, n, patch=setattr_("mem_cap", 30)), EINVAL),
        ("sp > stack_cap", lambda: lanes(with_lane(sp=21), 20, n), EINVAL),
        ("msize % 32", lambda: lanes(with_lane(msize=16), 20, n), EINVAL),
        ("storage_count > storage_cap", lambda: lanes(with_lane(storage_count=7), 20, n), EINVAL),
        ("unknown code_id", lambda: lanes(with_lane(code_id=1 << 20), 20, n), ENOCODE),
    ]

    def sym_up(**fields):
        h = with_lane(**fields)
        s = h.sym_soa_range(20, n)
        return lib.mg_sym_upload(ctx, ctypes.addressof(s), 20, n)

    def taint_up(slot=None, **fields):
        h = with_lane(**fields)
        if slot is not None:
            h.sobj[23, 19] = slot
        s = h.taint_soa_range(20, n)
        return lib.mg_taint_upload(ctx, ctypes.addressof(s), 20, n)
    cases += [("n_nodes > node_cap", lambda: sym_up(n_nodes=36), EINVAL),
              ("a handle >= obj_cap", lambda: taint_up(slot=40), EINVAL),
              ("n_fixed < MG_TAINT_OBJ0", lambda: taint_up(n_fixed=MG_TAINT_OBJ0 - 1), EINVAL),
              ("n_atoms > 64", lambda: taint_up(n_atoms=65), EINVAL)]
    for what, call, code in cases:
        assert call() == code, what
        assert lib.mg_last_error(ctx), what
        assert whole_diff(_full(dev, shape), base) == [], what
    # the context still works: the accepted image goes up and comes back
    model = DeviceImage(shape)
    model.upload(base, 0, N)
    dev.upload_range(good, 20, n)
    model.upload(good, 20, n)
    assert whole_diff(_full(dev, shape), _expected_full(model)) == []


def test_null_fields_and_live_counts(dev):
    rng = np.random.default_rng(0xE45)
    shape = _shape("plain")
    cid = _code(dev)
    dev.alloc(shape)
    base = _saturated(shape, rng, cid)
    dev.upload(base)
    model = DeviceImage(shape)
    model.upload(base, 0, N)
    lib, ctx = dev.lib, dev.ctx
    first, n = 37, 27
    host = _host(shape, rng, cid, first, n, {"sp": 9, "msize": 224, "storage_count": 3, "trace_len": 65,
                                             "rec_len": 64})
    # upload with fent = NULL: the range's fent becomes MG_FENT_NONE
    s = host.soa_range(first, n)
    s.fent = None
    assert lib.mg_lanes_upload(ctx, ctypes.addressof(s), first, n) == native.MG_OK
    host.fent = None
    model.upload(host, first, n)
    full = _full(dev, shape)
    assert whole_diff(full, _expected_full(model)) == []
    assert (full.fent[first:first + n] == MG_FENT_NONE).all() and (full.fent[:first] != MG_FENT_NONE).any()

    # a non-live download that skips fields: the rest arrives, the skipped arrays stay
    skipped = ("stack", "memory", "storage", "env", "calldata", "pc", "gas_min", "status")
    got, want = sentinel_filled(shape), sentinel_filled(shape)
    s = got.soa_range(first, n)
    for f in skipped:
        setattr(s, f, None)
    assert lib.mg_lanes_download(ctx, ctypes.addressof(s), first, n) == native.MG_OK
    model.download(want, first, n)
    keep = sentinel_filled(shape)
    for f in skipped:
        getattr(want, f)[...] = getattr(keep, f)
    assert whole_diff(got, want) == []
    assert np.array_equal(got.trace[first:first + n], model.img.trace[first:first + n])

    # a live download bounds rows by their count array: a NULL count with its rows
    # requested is refused by name before anything moves
    for count, rows in (("sp", "stack"), ("storage_count", "storage"), ("msize", "memory"),
                        ("trace_len", "trace"), ("rec_len", "rec")):
        got = sentinel_filled(shape)
        s = got.soa_range(first, n)
        setattr(s, count, None)
        assert lib.mg_lanes_download_live(ctx, ctypes.addressof(s), first, n) == native.MG_EINVAL, count
        assert count.encode() in lib.mg_last_error(ctx)
        assert whole_diff(got, keep) == [], count
        # with the rows skipped too there is nothing to bound
        setattr(s, rows, None)
        assert lib.mg_lanes_download_live(ctx, ctypes.addressof(s), first, n) == native.MG_OK, count
        want = sentinel_filled(shape)
        model.download(want, first, n, live=True)
        getattr(want, count)[...] = getattr(keep, count)
        getattr(want, rows)[...] = getattr(keep, rows)
        assert whole_diff(got, want) == [], count
    assert whole_diff(_full(dev, shape), _expected_full(model)) == []


# ------------------------------------------------ f. the path planes of mg_explore
PATH_RANGES = [(0, 600), (63, 130), (560, 40), (599, 1)]
SENTINEL = 0xA5A5A5A5


def _paths_down(dev, cap, first, n):
    """mg_explore_download into sentinel-filled arrays: (rc, path, path_len, root)."""
    path = np.full((n, cap), SENTINEL, dtype=np.uint32)
    path_len, root = np.full(n, SENTINEL, dtype=np.uint32), np.full(n, SENTINEL, dtype=np.uint32)
    rc = dev.lib.mg_explore_download(dev.ctx, path.ctypes.data, path_len.ctypes.data, root.ctypes.data, first, n)
    return rc, path, path_len, root


def _masked(path, path_len):
    """The rows with 0 at and above each lane's length."""
    keep = np.arange(path.shape[1])[None, :] < path_len[:, None]
    return np.where(keep, path, 0).astype(np.uint32)


def _model_rows(p):
    """[path with 0 at and above each length, path_len, root] of a model's paths, copied."""
    return [_masked(p.path, p.path_len), p.path_len.copy(), p.root.copy()]


def test_path_planes_ranges_tails_and_refusals(dev):
    """mg_explore_upload and mg_explore_download on the harvest tests' batch: 600
    lanes (nine 64-lane transfer tiles and a tail of 24), path_cap 7, every length
    0 .. 7."""
    import test_gpu_harvest as harvest
    n, cap = harvest.N, harvest.HPATH_CAP
    _, _, built = harvest._batch(dev, "explore")                 # uploads its paths; left unchanged here
    assert (n, cap) == (600, 7) and set(built.path_len.tolist()) == set(range(cap + 1))
    lib, ctx = dev.lib, dev.ctx
    want = _model_rows(built)

    def check_ranges(what):
        for first, k in PATH_RANGES:
            rc, path, path_len, root = _paths_down(dev, cap, first, k)
            assert rc == native.MG_OK, lib.mg_last_error(ctx)
            assert np.array_equal(path_len, want[1][first:first + k]), (what, first, k)
            assert np.array_equal(root, want[2][first:first + k]), (what, first, k)
            assert np.array_equal(path, want[0][first:first + k]), (what, first, k)
            # at and above path_len: 0, whatever the host array held
            assert not (path[np.arange(cap)[None, :] >= path_len[:, None]]).any(), (what, first, k)

    check_ranges("as uploaded")
    # a sub-range with other rows: the lanes outside it keep theirs
    first, k = 64, 65
    rng = np.random.default_rng(0x9A7)
    new_len = ((np.arange(k) * 3 + 5) % (cap + 1)).astype(np.uint32)
    assert set(new_len.tolist()) == set(range(cap + 1))
    new_path = _masked(rng.integers(1, 1 << 32, size=(k, cap), dtype=np.uint32), new_len)
    new_root = rng.integers(0, n, size=k, dtype=np.uint32)
    dev.explore_upload_paths(new_path, new_len, new_root, first)
    want[0][first:first + k], want[1][first:first + k], want[2][first:first + k] = new_path, new_len, new_root
    check_ranges("after the sub-range")
    # junk above path_len on the host never reaches a reader: the range download and a
    # harvest of those lanes at the full path capacity both return zeros there
    junk = rng.integers(1, 1 << 32, size=(k, cap), dtype=np.uint32)
    junk_len = new_len[::-1].copy()
    dev.explore_upload_paths(junk, junk_len, new_root, first)
    want[0][first:first + k], want[1][first:first + k] = _masked(junk, junk_len), junk_len
    check_ranges("after the junk rows")
    chosen = list(range(first, first + k))
    info = dev.harvest_select(0xFFFFFFFF, sorted(set(range(n)) - set(chosen)))
    assert info.n == k and info.path_len == cap
    got = sentinel_filled(dataclasses.replace(dev.shape, n=k))
    rc, lanes, path, path_len, root = harvest._download(dev, got, True, cap)
    assert rc == native.MG_OK and lanes.tolist() == chosen
    assert np.array_equal(path, want[0][first:first + k]) and np.array_equal(path_len, junk_len)
    assert np.array_equal(root, new_root)

    # refusals keep their codes and move nothing
    ok = [a.copy() for a in (new_path, new_len, new_root)]
    ptr = lambda a: a.ctypes.data
    for fn in (lib.mg_explore_upload, lib.mg_explore_download):
        assert fn(ctx, ptr(ok[0]), ptr(ok[1]), ptr(ok[2]), n - k + 1, k) == native.MG_EINVAL       # past the batch
        assert fn(ctx, ptr(ok[0]), ptr(ok[1]), ptr(ok[2]), n, 1) == native.MG_EINVAL
        assert fn(ctx, ptr(ok[0]), ptr(ok[1]), ptr(ok[2]), 0xFFFFFFFF, 2) == native.MG_EINVAL
        assert fn(ctx, None, ptr(ok[1]), ptr(ok[2]), first, k) == native.MG_EINVAL
        assert fn(ctx, ptr(ok[0]), None, ptr(ok[2]), first, k) == native.MG_EINVAL
        assert fn(ctx, ptr(ok[0]), ptr(ok[1]), None, first, k) == native.MG_EINVAL
        assert fn(ctx, None, None, None, first, 0) == native.MG_OK                                 # nothing to move
    long_len = new_len.copy()
    long_len[k - 1] = cap + 1
    assert lib.mg_explore_upload(ctx, ptr(ok[0]), ptr(long_len), ptr(ok[2]), first, k) == native.MG_EINVAL
    assert b"path_len" in lib.mg_last_error(ctx)
    assert all(np.array_equal(a, b) for a, b in zip(ok, (new_path, new_len, new_root)))
    check_ranges("after the refusals")
    # before mg_explore_alloc
    harvest._forget(dev)
    dev.alloc(_shape("symbolic", n=8))
    small = [np.zeros((8, cap), dtype=np.uint32), np.zeros(8, dtype=np.uint32), np.zeros(8, dtype=np.uint32)]
    for fn in (lib.mg_explore_upload, lib.mg_explore_download):
        assert fn(ctx, ptr(small[0]), ptr(small[1]), ptr(small[2]), 0, 8) == native.MG_ESTATE
        assert b"mg_explore_alloc" in lib.mg_last_error(ctx)

