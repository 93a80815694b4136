"""The lane-transfer model (tests/xfermodel.py) pinned without a device: one
hand-worked example with literal expected arrays, property tests of the model,
and OracleDevice moving exactly what the model says (live bounds included), so
the CPU end-to-end tests run with the transfers the GPU has.
"""
import numpy as np

from mythril_amd.lanes import _ALL_FIELDS, MG_FENT_NONE, MG_HALT_STOP, LaneBatch, LaneShape
from oracle_device import OracleDevice
from xfermodel import (DeviceImage, fields_of, live_diff, live_equal, saturated, sentinel_filled, whole_diff)

S32 = 0xA5A5A5A5          # sentinel_filled's pattern as a dword
S8 = 0xA5


def _w(v):                 # one 256-bit word / storage half with every limb v
    return [v] * 8


def test_hand_worked_range_upload_and_live_download():
    shape = LaneShape(n=3, stack_cap=3, mem_cap=32, calldata_cap=4, storage_cap=2)
    dev = DeviceImage(shape)
    d = dev.img
    # the device before: lane l, slot s holds 0xD00 + 16 l + s in every limb
    d.stack[...] = np.array([[_w(0xD00), _w(0xD01), _w(0xD02)],
                             [_w(0xD10), _w(0xD11), _w(0xD12)],
                             [_w(0xD20), _w(0xD21), _w(0xD22)]], dtype=np.uint32)
    d.storage[...] = np.array([[_w(0xE00) + _w(0xE08), _w(0xE01) + _w(0xE09)],
                               [_w(0xE10) + _w(0xE18), _w(0xE11) + _w(0xE19)],
                               [_w(0xE20) + _w(0xE28), _w(0xE21) + _w(0xE29)]], dtype=np.uint32)
    d.memory[...] = np.array([[0xC0] * 32, [0xC1] * 32, [0xC2] * 32], dtype=np.uint8)
    d.calldata[...] = np.array([[0xB0] * 4, [0xB1] * 4, [0xB2] * 4], dtype=np.uint8)
    d.sp[:] = [3, 3, 3]
    d.msize[:] = [32, 32, 32]
    d.storage_count[:] = [2, 2, 2]
    d.pc[:] = [70, 71, 72]
    d.status[:] = MG_HALT_STOP
    d.fent[:] = [7, 8, 9]
    # the host: lane l, slot s holds 0xA00 + 16 l + s
    h = LaneBatch(shape)
    h.stack[...] = np.array([[_w(0xA00), _w(0xA01), _w(0xA02)],
                             [_w(0xA10), _w(0xA11), _w(0xA12)],
                             [_w(0xA20), _w(0xA21), _w(0xA22)]], dtype=np.uint32)
    h.storage[...] = np.array([[_w(0xF00) + _w(0xF08), _w(0xF01) + _w(0xF09)],
                               [_w(0xF10) + _w(0xF18), _w(0xF11) + _w(0xF19)],
                               [_w(0xF20) + _w(0xF28), _w(0xF21) + _w(0xF29)]], dtype=np.uint32)
    h.memory[...] = np.array([[0x30] * 32, [0x31] * 32, [0x32] * 32], dtype=np.uint8)
    h.calldata[...] = np.array([[0x40] * 4, [0x41] * 4, [0x42] * 4], dtype=np.uint8)
    h.env[...] = np.array([[_w(0x500)] * 5, [_w(0x510)] * 5, [_w(0x520)] * 5], dtype=np.uint32)
    h.sp[:] = [3, 2, 1]
    h.msize[:] = [32, 32, 0]
    h.storage_count[:] = [2, 0, 1]
    h.pc[:] = [10, 11, 12]
    h.status[:] = MG_HALT_STOP
    h.fent = None                                   # the host passes no fent

    dev.upload(h, 1, 2)                             # lanes [1, 3): sp = [2, 1]

    # range maxima: sp 2, msize 32, storage_count 1.  Lane 0 keeps everything; in
    # lanes 1 and 2 slots 0..1, storage entry 0 and the whole memory are the
    # host's (lane 2's slot 1 too, above its own sp), slot 2 and entry 1 stay.
    assert d.stack.tolist() == [[_w(0xD00), _w(0xD01), _w(0xD02)],
                                [_w(0xA10), _w(0xA11), _w(0xD12)],
                                [_w(0xA20), _w(0xA21), _w(0xD22)]]
    assert d.storage.tolist() == [[_w(0xE00) + _w(0xE08), _w(0xE01) + _w(0xE09)],
                                  [_w(0xF10) + _w(0xF18), _w(0xE11) + _w(0xE19)],
                                  [_w(0xF20) + _w(0xF28), _w(0xE21) + _w(0xE29)]]
    assert d.memory.tolist() == [[0xC0] * 32, [0x31] * 32, [0x32] * 32]
    assert d.calldata.tolist() == [[0xB0] * 4, [0x41] * 4, [0x42] * 4]
    assert d.env.tolist() == [[_w(0)] * 5, [_w(0x510)] * 5, [_w(0x520)] * 5]
    assert d.sp.tolist() == [3, 2, 1]
    assert d.msize.tolist() == [32, 32, 0]
    assert d.storage_count.tolist() == [2, 0, 1]
    assert d.pc.tolist() == [70, 11, 12]
    assert d.fent.tolist() == [7, MG_FENT_NONE, MG_FENT_NONE]

    out = sentinel_filled(shape)
    dev.download(out, 1, 2, live=True)

    # device maxima of the range: sp 2, msize 32, storage_count 1
    assert out.stack.tolist() == [[_w(S32), _w(S32), _w(S32)],
                                  [_w(0xA10), _w(0xA11), _w(S32)],
                                  [_w(0xA20), _w(0xA21), _w(S32)]]
    assert out.storage.tolist() == [[_w(S32) + _w(S32), _w(S32) + _w(S32)],
                                    [_w(0xF10) + _w(0xF18), _w(S32) + _w(S32)],
                                    [_w(0xF20) + _w(0xF28), _w(S32) + _w(S32)]]
    assert out.memory.tolist() == [[S8] * 32, [0x31] * 32, [0x32] * 32]
    assert out.calldata.tolist() == [[S8] * 4] * 3            # live: calldata and env stay the host's
    assert out.env.tolist() == [[_w(S32)] * 5] * 3
    assert out.sp.tolist() == [S32, 2, 1]
    assert out.msize.tolist() == [S32, 32, 0]
    assert out.storage_count.tolist() == [S32, 0, 1]
    assert out.pc.tolist() == [S32, 11, 12]
    assert out.fent.tolist() == [S32, MG_FENT_NONE, MG_FENT_NONE]
    assert out.gas_min.tolist() == [0xA5A5A5A5A5A5A5A5, 0, 0]


# ------------------------------------------------------------- property tests
DEV = LaneShape(n=23, stack_cap=7, mem_cap=96, calldata_cap=12, storage_cap=3, trace_cap=5, rec_cap=9,
                node_cap=6, const_cap=3, obj_cap=17)
SLIM = LaneShape(n=23, stack_cap=4, mem_cap=32, calldata_cap=8, storage_cap=2, trace_cap=0, rec_cap=4,
                 node_cap=3, const_cap=2, obj_cap=15)
COUNTS = (("sp", "stack_cap", 1), ("storage_count", "storage_cap", 1), ("msize", "mem_cap", 32),
          ("trace_len", "trace_cap", 1), ("rec_len", "rec_cap", 1), ("n_nodes", "node_cap", 1),
          ("n_consts", "const_cap", 1))


def _host(shape, rng):
    """Random rows everywhere, random counts within the capacities."""
    b = saturated(shape, rng, 0)
    for count, cap, step in COUNTS:
        c = getattr(shape, cap) // step
        getattr(b, count)[:] = rng.integers(0, c + 1, size=shape.n) * step
    b.n_obj[:] = rng.integers(7, shape.obj_cap + 1, size=shape.n)
    return b


def _cases():
    for seed in range(12):
        rng = np.random.default_rng(seed)
        first = int(rng.integers(0, DEV.n))
        n = int(rng.integers(1, DEV.n - first + 1))
        yield seed, rng, first, n, (SLIM if seed % 2 else DEV)


def test_upload_then_full_download_returns_the_live_data_and_spares_other_lanes():
    for seed, rng, first, n, hshape in _cases():
        dev = DeviceImage(DEV)
        base = saturated(DEV, rng, 0)
        dev.upload(base, 0, DEV.n)
        assert whole_diff(dev.img, base) == []
        host = _host(hshape, rng)
        dev.upload(host, first, n, live=bool(seed & 2))
        outside = [i for i in range(DEV.n) if not first <= i < first + n]
        assert whole_diff(dev.img, base, lanes=outside) == [], seed       # lanes outside never change
        out = sentinel_filled(hshape)
        dev.download(out, first, n)
        got, want = LaneBatch(LaneShape(**{**hshape.__dict__, "n": n})), None
        want = LaneBatch(got.shape)
        for f in fields_of(hshape):
            getattr(got, f)[...] = getattr(out, f)[first:first + n]
            getattr(want, f)[...] = getattr(host, f)[first:first + n]
        assert live_diff(got, want) == [], seed
        # live_equal looks below each lane's own counts only
        i = int(np.argmin(want.sp))
        if int(want.sp[i]) < hshape.stack_cap:
            want.stack[i, int(want.sp[i])] ^= 1
            assert live_equal(got, want)
        if int(want.sp[i]):
            want.stack[i, int(want.sp[i]) - 1] ^= 1
            assert not live_equal(got, want)
        # and above the range's largest count the device kept what it had
        k = int(host.sp[first:first + n].max())
        assert np.array_equal(dev.img.stack[first:first + n, k:], base.stack[first:first + n, k:])
        assert k == hshape.stack_cap or not np.array_equal(dev.img.stack[first:first + n, k:hshape.stack_cap],
                                                           host.stack[first:first + n, k:])


def test_live_download_leaves_the_sentinel_exactly_above_the_bound():
    for seed, rng, first, n, hshape in _cases():
        dev = DeviceImage(DEV)
        dev.upload(saturated(DEV, rng, 0), 0, DEV.n)
        dev.upload(_host(DEV, rng), 0, DEV.n)
        out = sentinel_filled(hshape)
        dev.download(out, first, n, live=True)
        r = slice(first, first + n)
        assert (out.env.view(np.uint8) == S8).all() and (out.calldata == S8).all()
        rows = [("stack", "sp"), ("storage", "storage_count"), ("memory", "msize"), ("rec", "rec_len"),
                ("node", "n_nodes"), ("cval", "n_consts"), ("omask", "n_obj")]
        if hshape.trace_cap:
            rows.append(("trace", "trace_len"))
        for f, count in rows:
            x, dx = getattr(out, f), getattr(dev.img, f)
            k = min(int(getattr(dev.img, count)[r].max()), x.shape[1])
            assert np.array_equal(x[r, :k], dx[r, :k]), (seed, f)
            assert (x[r, k:].view(np.uint8) == S8).all(), (seed, f)
            assert (x[:first].view(np.uint8) == S8).all() and (x[first + n:].view(np.uint8) == S8).all(), (seed, f)
        for f in ("sp", "pc", "gas_max", "n_obj"):
            assert (getattr(out, f)[:first].view(np.uint8) == S8).all()
            assert np.array_equal(getattr(out, f)[r], getattr(dev.img, f)[r])


def test_a_host_without_traces_or_records_zeroes_the_lengths():
    rng = np.random.default_rng(3)
    dev = DeviceImage(DEV)
    dev.upload(saturated(DEV, rng, 0), 0, DEV.n)
    host = _host(SLIM, rng)                       # trace_cap 0
    dev.upload(host, 4, 9)
    assert (dev.img.trace_len[4:13] == 0).all() and (dev.img.trace_len[:4] == DEV.trace_cap).all()
    assert np.array_equal(dev.img.rec_len[4:13], host.rec_len[4:13])


# ------------------------------------------------------------- OracleDevice
def test_oracle_device_honours_live_and_bounded_uploads():
    rng = np.random.default_rng(11)
    ora = OracleDevice()
    cid = ora.load_code(b"\x00")
    ora.alloc(DEV)
    base = saturated(DEV, rng, cid)
    ora.upload(base)
    model = DeviceImage(DEV)
    model.upload(base, 0, DEV.n)
    host = _host(DEV, rng)
    host.code_id[:] = cid
    host.sp[5:12] = rng.integers(0, 4, size=7)    # the range's largest sp stays below the capacity
    host.sp[8] = 3
    for live in (False, True):                    # a non-live upload is bounded as well
        ora.upload_range(host, 5, 7, live=live)
        model.upload(host, 5, 7, live=live)
        full = sentinel_filled(DEV)
        ora.download(full)
        assert whole_diff(full, model.img) == []
        assert np.array_equal(full.stack[5:12, 3:], base.stack[5:12, 3:])       # kept above the bound
        assert np.array_equal(full.stack[5:12, :3], host.stack[5:12, :3])
    out, want = sentinel_filled(DEV), sentinel_filled(DEV)
    ora.download_range(out, 5, 7, live=True)
    model.download(want, 5, 7, live=True)
    assert whole_diff(out, want) == []
    assert (out.stack[5:12, 3:] == S32).all() and (out.stack[:5] == S32).all() and (out.stack[12:] == S32).all()
    assert (out.env == S32).all() and (out.calldata == S8).all()
    assert np.array_equal(out.stack[5:12, :3], host.stack[5:12, :3])
    # a slim image through download(batch, first): written at the slim stride
    slim, want = sentinel_filled(LaneShape(**{**SLIM.__dict__, "n": 6})), None
    want = sentinel_filled(slim.shape)
    ora.download(slim, 9)
    model.download(want, 9, 6, host_first=0)
    assert whole_diff(slim, want) == []
    assert np.array_equal(slim.stack, model.img.stack[9:15, :SLIM.stack_cap])


def test_soa_is_soa_range_of_every_lane():
    """soa() is soa_range(0, n), and soa_range(first, n) points first rows into each array."""
    shape = LaneShape(n=12, stack_cap=5, mem_cap=64, calldata_cap=8, storage_cap=3, trace_cap=6, rec_cap=7,
                      node_cap=4, const_cap=2, obj_cap=20)
    b = LaneBatch(shape)
    whole, ranged = b.soa(), b.soa_range(0, shape.n)
    names = [f for f, _ in type(whole)._fields_ if not f.startswith("_pad")]
    assert {"n", "stack_cap", "mem_cap", "calldata_cap", "storage_cap", "trace_cap", "rec_cap"} < set(names)
    arrays = [f for f in names if not (f == "n" or f.endswith("_cap"))]
    assert len(arrays) == 26 and set(arrays) == set(_ALL_FIELDS)
    for f in names:
        assert getattr(whole, f) == getattr(ranged, f), f
    for f in arrays:
        assert getattr(whole, f) == getattr(b, f).ctypes.data, f
    for f in names:
        if f.endswith("_cap"):
            assert getattr(whole, f) == getattr(shape, f), f
    part = b.soa_range(7, 5)
    assert part.n == 5 and part.trace_cap == 6 and part.rec_cap == 7
    for f in arrays:
        arr = getattr(b, f)
        assert getattr(part, f) == arr.ctypes.data + 7 * arr.strides[0], f
