"""Kernel 2's launch geometry on the MI355X: more than one model chunk per block
(bv_grid's chunks_per_block > 1) for k_bv_terms and k_bv_eval, tile edges by DAG
count and by instruction count, partial model chunks, DAG ranges of mg_eval_run
that begin and end inside a tile, and bv_upload's refusals.  Expected results are
analytic (NumPy) and checked against tests/k2_insn_ref.py on a sample."""
import numpy as np
import pytest

from k2_insn_ref import values
from mythril_amd.device import GpuDevice
from mythril_amd.native import MythGpuError
from mythril_amd.smt.program import (OPCODE, REF_ACC, REF_CONST, REF_SLOT, REF_VAR, TAB_LO_SHIFT, TILE_INSNS, ModelPool,
                                     ProgramBatch, enc_w0, ref)

pytestmark = pytest.mark.gpu
ACC = ref(REF_ACC, 0)
NO_MODEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def dev():
    d = GpuDevice(0)
    yield d
    d.close()


def rand_words(rng, *shape):
    return rng.integers(0, 1 << 32, size=shape + (8,), dtype=np.uint64).astype(np.uint32)


def padded_programs(lengths, last_op, n_vars, consts, w3=0):
    """Program d: copy x[d % n_vars]; lengths[d] - 2 x 256-bit bvnot (the fuser leaves
    them alone); `last_op` acc, const[d].  Returns the batch and, per program,
    whether the bvnot run inverts."""
    rows, off = [], [0]
    for d, n in enumerate(lengths):
        assert n >= 2
        rows.append([enc_w0("copy", 256), ref(REF_VAR, d % n_vars), 0, 0])
        rows += [[enc_w0("bvnot", 256), ACC, 0, 0]] * (n - 2)
        rows.append([enc_w0(last_op, 1 if w3 else 256), ACC, ref(REF_CONST, d), w3])
        off.append(len(rows))
    prog = ProgramBatch(np.asarray(rows, dtype=np.uint32), np.asarray(off, dtype=np.uint32), consts, 1,
                        [f"x{k}" for k in range(n_vars)], [256] * n_vars)
    return prog, np.array([(n - 2) % 2 == 1 for n in lengths])


def sample_check(prog, pool, got, dags, ms):
    """The device's values at (dags x ms) against k2_insn_ref on those models."""
    models = [{n: int.from_bytes(pool.values[v, m].astype("<u4").tobytes(), "little")
               for v, n in enumerate(prog.var_names)} for m in ms]
    sub = ProgramBatch(np.concatenate([prog.program(d) for d in dags]),
                       np.cumsum([0] + [len(prog.program(d)) for d in dags]).astype(np.uint32), prog.consts,
                       prog.n_slots, prog.var_names, prog.var_widths)
    want = values(sub, models)
    for i, d in enumerate(dags):
        for j, m in enumerate(ms):
            assert int.from_bytes(got[d, m].astype("<u4").tobytes(), "little") == want[i][j], (d, m)


def sat_reference(sat):
    """(first_sat, sat_count, bitmap words) of a Boolean [n_dags, n_models] array."""
    n_dags, n_models = sat.shape
    padded = np.zeros((n_dags, 64 * ((n_models + 63) // 64)), dtype=np.uint8)
    padded[:, :n_models] = sat
    bits = np.packbits(padded, axis=1, bitorder="little").view(np.uint64)
    first = np.where(sat.any(axis=1), sat.argmax(axis=1), NO_MODEL).astype(np.uint32)
    return first, sat.sum(axis=1).astype(np.uint32), bits


# ------------------------------------------------- more than one chunk per block
N_BIG, M_BIG = 2048, 1030      # 2048 tiles of one program: groups_wanted = 2; 5 chunks: cpb = 2, 3 groups,
                               # the last with one chunk of 6 live lanes


@pytest.fixture(scope="module")
def big_pool():
    rng = np.random.default_rng(7)
    return ModelPool(rand_words(rng, 4, M_BIG))


@pytest.mark.parametrize("fuse", ["default", "0"])
def test_terms_with_two_chunks_per_block(dev, monkeypatch, big_pool, fuse):
    if fuse == "0":
        monkeypatch.setenv("MG_BV_FUSE", "0")
    rng = np.random.default_rng(11)
    consts = rand_words(rng, N_BIG)
    prog, inverts = padded_programs([130] * N_BIG, "bvxor", 4, consts)     # 130 > 128: one program per 256-slot tile
    assert not inverts.any()
    got, ms = dev.eval_terms(prog, big_pool)
    print(f"eval_terms {N_BIG} programs x {M_BIG} models: kernel_ms = {ms:.3f}")
    want = big_pool.values[np.arange(N_BIG) % 4] ^ consts[:, None, :]
    assert np.array_equal(got, want)
    sample_check(prog, big_pool, got, [0, 1, N_BIG // 2 + 3, N_BIG - 1], [0, 255, 256, 511, 512, 1023, 1024, 1029])


@pytest.mark.parametrize("fuse", ["default", "0"])
def test_eval_with_two_chunks_per_block(dev, monkeypatch, fuse):
    if fuse == "0":
        monkeypatch.setenv("MG_BV_FUSE", "0")
    # x[m] = m + 1, except: model 1029 alone holds 5000; models 800..899 repeat models 100..199
    x = np.arange(1, M_BIG + 1, dtype=np.uint32)
    x[800:900] = x[100:200]
    x[1029] = 5000
    d = np.arange(N_BIG, dtype=np.uint32)
    c = (d * 7 % 1029 + 1).astype(np.uint32)
    c[d % 8 == 0] = 5000                  # only the last model, the last group's 6th live lane
    c[d % 8 == 1] = 301                   # only model 300: the second chunk of the first group
    c[d % 8 == 2] = 0                     # no model
    c[d % 8 == 3] = 101 + d[d % 8 == 3] % 100     # two models, in the first and in the second group
    consts = np.zeros((N_BIG, 8), dtype=np.uint32)
    consts[:, 0] = c
    vals = np.zeros((1, M_BIG, 8), dtype=np.uint32)
    vals[0, :, 0] = x
    prog, _ = padded_programs([130] * N_BIG, "eq", 1, consts, w3=256)
    sat = x[None, :] == c[:, None]
    first, count, bits = sat_reference(sat)
    assert first[0] == 1029 and first[1] == 300 and first[2] == NO_MODEL and count[3] == 2 and first[3] < 256
    fs, sc, got_bits, ms = dev.eval_bits(prog, ModelPool(vals))
    print(f"eval_bits {N_BIG} programs x {M_BIG} models: kernel_ms = {ms:.3f}")
    assert np.array_equal(fs, first) and np.array_equal(sc, count) and np.array_equal(got_bits, bits)


# ------------------------------------------------------------------- tile edges
MODEL_COUNTS = [1, 63, 64, 65, 255, 256, 257, 513]


@pytest.mark.parametrize("n_dags", [1, 63, 64, 65, 128, 129])
def test_one_instruction_programs_across_tile_and_chunk_edges(dev, n_dags):
    """BV_TILE_DAGS = 64 programs close a tile; 256 models fill a chunk."""
    rng = np.random.default_rng(n_dags)
    consts = rand_words(rng, n_dags)
    consts[::3, 1:] = 0
    off = np.arange(n_dags + 1, dtype=np.uint32)
    add = np.array([[enc_w0("bvadd", 256), ref(REF_VAR, 0), ref(REF_CONST, d), 0] for d in range(n_dags)], dtype=np.uint32)
    ult = np.array([[enc_w0("bvult", 1), ref(REF_VAR, 0), ref(REF_CONST, d), 256] for d in range(n_dags)], dtype=np.uint32)
    ci = np.array([int.from_bytes(r.astype("<u4").tobytes(), "little") for r in consts], dtype=object)
    for n_models in MODEL_COUNTS:
        vals = rand_words(rng, 1, n_models)
        vals[0, ::2, 1:] = 0
        pool = ModelPool(vals)
        xi = np.array([int.from_bytes(r.astype("<u4").tobytes(), "little") for r in vals[0]], dtype=object)
        got, _ = dev.eval_terms(ProgramBatch(add, off, consts, 1, ["x"], [256]), pool)
        want = (xi[None, :] + ci[:, None]) % (1 << 256)
        raw = b"".join(int(v).to_bytes(32, "little") for v in want.ravel())
        assert np.array_equal(got, np.frombuffer(raw, dtype="<u4").reshape(n_dags, n_models, 8)), n_models
        first, count, bits = sat_reference((xi[None, :] < ci[:, None]).astype(bool))
        fs, sc, got_bits, _ = dev.eval_bits(ProgramBatch(ult, off, consts, 1, ["x"], [256]), pool)
        assert np.array_equal(fs, first) and np.array_equal(sc, count) and np.array_equal(got_bits, bits), n_models


def test_mixed_lengths_close_tiles_by_instruction_count(dev):
    """Programs of 2..256 instructions: tiles close on the 256-slot capacity (3 x 100,
    255 + 2, 256 alone, 128 + 128 exactly) and on 64 programs (a run of 70 short ones)."""
    lengths = [100, 100, 100, 2, 255, 2, 256, 128, 128, 3] + [2, 3] * 35 + [256, 2, 254, 2, 2]
    n = len(lengths)
    rng = np.random.default_rng(3)
    consts = rand_words(rng, n)
    pool = ModelPool(rand_words(rng, 3, 300))
    prog, inverts = padded_programs(lengths, "bvxor", 3, consts)
    assert inverts.any() and not inverts.all()
    got, _ = dev.eval_terms(prog, pool)
    base = pool.values[np.arange(n) % 3]
    want = np.where(inverts[:, None, None], ~base, base) ^ consts[:, None, :]
    assert np.array_equal(got, want)
    sample_check(prog, pool, got, [0, 2, 3, 4, 6, 9, 10, n - 1], [0, 63, 255, 256, 299])
    # the same programs ending in an unsigned comparison with the constant, through k_bv_eval
    eqp, _ = padded_programs(lengths, "bvult", 3, consts, w3=256)
    wi = np.where(inverts[:, None, None], ~base, base)
    lt = np.zeros((n, 300), dtype=bool)
    for limb in range(8):                      # little-endian compare, most significant limb last
        lt = np.where(wi[:, :, limb] != consts[:, None, limb], wi[:, :, limb] < consts[:, None, limb], lt)
    first, count, bits = sat_reference(lt)
    fs, sc, got_bits, _ = dev.eval_bits(eqp, pool)
    assert np.array_equal(fs, first) and np.array_equal(sc, count) and np.array_equal(got_bits, bits)


# ------------------------------------------------------------------- DAG ranges
@pytest.mark.parametrize("first,count", [(70, 20), (63, 2), (5, 1), (0, 1), (149, 1), (64, 64), (1, 148)])
def test_dag_ranges_inside_tiles(dev, first, count):
    """150 one-instruction programs (tiles 0..63, 64..127, 128..149), 300 models: a
    range alone, then its complement; a DAG evaluated outside its range would be
    counted twice (sat_count is accumulated)."""
    n, n_models = 150, 300
    rng = np.random.default_rng(first * 1000 + count)
    x = rng.integers(0, 1000, size=n_models).astype(np.uint32)
    c = rng.integers(0, 1000, size=n).astype(np.uint32)
    c[::7] = 0                                                    # no model
    consts = np.zeros((n, 8), dtype=np.uint32)
    consts[:, 0] = c
    vals = np.zeros((1, n_models, 8), dtype=np.uint32)
    vals[0, :, 0] = x
    rows = np.array([[enc_w0("bvult", 1), ref(REF_VAR, 0), ref(REF_CONST, d), 256] for d in range(n)], dtype=np.uint32)
    prog = ProgramBatch(rows, np.arange(n + 1, dtype=np.uint32), consts, 1, ["x"], [256])
    want_first, want_count, _ = sat_reference(x[None, :] < c[:, None])
    dev.eval_upload(prog, ModelPool(vals))
    dev.eval_run(first, count)
    fs, sc = dev.eval_download(first, count)
    assert np.array_equal(fs, want_first[first:first + count]) and np.array_equal(sc, want_count[first:first + count])
    if first > 0:
        dev.eval_run(0, first)
    if first + count < n:
        dev.eval_run(first + count, n - first - count)
    fs, sc = dev.eval_download()
    assert np.array_equal(fs, want_first) and np.array_equal(sc, want_count)
    for bad_first, bad_count in ((0, 0), (10, 0), (0, n + 1), (n, 1), (n - 1, 2)):
        with pytest.raises(MythGpuError) as e:
            dev.eval_run(bad_first, bad_count)
        assert "rc=-1" in str(e.value) and "range" in str(e.value)
    fs, sc = dev.eval_download()                                  # the refusals changed nothing
    assert np.array_equal(fs, want_first) and np.array_equal(sc, want_count)


# ------------------------------------------------------------ bv_upload's refusals
def _good():
    """Three programs over 2 variables, 2 constants, 2 slots and one table."""
    from mythril_amd.smt.lower import TableSig
    from mythril_amd.smt.program import ArrayInterp
    rows = [[enc_w0("bvadd", 256, 1), ref(REF_VAR, 0), ref(REF_CONST, 1), 0],
            [enc_w0("ite", 64), ref(REF_VAR, 1), ref(REF_SLOT, 1), ref(REF_CONST, 0)],
            [enc_w0("bvmul", 256), ref(REF_VAR, 0), ref(REF_VAR, 0), 0],
            [enc_w0("tab", 8), ref(REF_VAR, 0), ref(REF_CONST, 0), 0 | (8 << TAB_LO_SHIFT)]]
    consts = np.zeros((2, 8), dtype=np.uint32)
    consts[1, 0] = 9
    prog = ProgramBatch(np.asarray(rows, dtype=np.uint32), np.array([0, 2, 3, 4], dtype=np.uint32), consts, 2,
                        ["x", "c"], [256, 1], [TableSig("Storage", "array", (256,), 256)])
    models = [{"x": k * 0x10001, "c": k & 1, "Storage": ArrayInterp(0xABCD, {k * 0x10001: 0x123456 + k})} for k in range(70)]
    return prog, models


def _mutated(prog, at=None, word=0, value=None, **fields):
    rows = prog.insns.copy()
    if at is not None:
        rows[at, word] = value
    out = ProgramBatch(rows, prog.prog_off.copy(), prog.consts, prog.n_slots, prog.var_names, prog.var_widths, prog.tables)
    for k, v in fields.items():
        setattr(out, k, v)
    return out


def test_bv_upload_refuses_malformed_batches_before_any_launch(dev):
    prog, models = _good()
    pool = ModelPool.from_dicts(models, prog.var_names, prog.var_widths, prog.tables)
    want = values(prog, models)

    def good_still_works():
        got, _ = dev.eval_terms(prog, pool)
        assert [[int.from_bytes(got[d, m].astype("<u4").tobytes(), "little") for m in range(70)] for d in range(3)] == want

    good_still_works()
    w0 = int(prog.insns[0, 0])
    long_off = np.array([0, TILE_INSNS + 1], dtype=np.uint32)
    long_rows = np.tile(np.array([[enc_w0("bvnot", 256), ref(REF_VAR, 0), 0, 0]], dtype=np.uint32), (TILE_INSNS + 1, 1))
    few_entries = ModelPool(pool.values, pool.tab_start, pool.tab_count, pool.tab_entries[:-1], pool.tab_default)
    past_entries = ModelPool(pool.values, pool.tab_start + np.uint32(0xFFFFFFF0), pool.tab_count, pool.tab_entries,
                             pool.tab_default)
    no_tables = ModelPool(pool.values)
    cases = [
        ("op = MG_BV_NUM_OPS", _mutated(prog, 0, 0, (w0 & ~0xFF) | len(OPCODE)), pool, "bad instruction 0"),
        ("op = 255", _mutated(prog, 2, 0, int(prog.insns[2, 0]) | 0xFF), pool, "bad instruction 2"),
        ("width 0", _mutated(prog, 0, 0, w0 & ~(0x1FF << 8)), pool, "bad instruction 0"),
        ("width 257", _mutated(prog, 0, 0, (w0 & ~(0x1FF << 8)) | (257 << 8)), pool, "bad instruction 0"),
    ] + [(f"bit {bit} of w0", _mutated(prog, 1, 0, int(prog.insns[1, 0]) | (1 << bit)), pool, "bad instruction 1")
         for bit in range(22, 32)] + [
        ("store slot = n_slots", _mutated(prog, 0, 0, (w0 & ~(0xF << 18)) | (2 << 18)), pool, "slot out of range"),
        ("slot operand = n_slots", _mutated(prog, 1, 2, ref(REF_SLOT, 2)), pool, "operand out of range at instruction 1"),
        ("variable = n_vars", _mutated(prog, 2, 1, ref(REF_VAR, 2)), pool, "operand out of range at instruction 2"),
        ("variable index 2^30 - 1", _mutated(prog, 2, 2, ref(REF_VAR, 0x3FFFFFFF)), pool, "operand out of range"),
        ("constant = n_consts", _mutated(prog, 0, 2, ref(REF_CONST, 2)), pool, "operand out of range at instruction 0"),
        ("accumulator in B", _mutated(prog, 2, 2, ACC), pool, "accumulator operand past position A at instruction 2"),
        ("accumulator in C", _mutated(prog, 1, 3, ACC), pool, "accumulator operand past position A at instruction 1"),
        ("table = n_tables", _mutated(prog, 3, 3, 1 | (8 << TAB_LO_SHIFT)), pool, "bad table reference at instruction 3"),
        ("table without tables", prog, no_tables, "bad table reference at instruction 3"),
        ("table lo + width = 257", _mutated(prog, 3, 3, 249 << TAB_LO_SHIFT), pool, "bad table reference at instruction 3"),
        ("table immediate bit 29", _mutated(prog, 3, 3, 1 << 29), pool, "bad table reference at instruction 3"),
        ("decreasing offsets", _mutated(prog, prog_off=np.array([0, 3, 2, 4], dtype=np.uint32)), pool, "bad program offsets"),
        ("program of MG_BV_TILE_INSNS + 1", ProgramBatch(long_rows, long_off, prog.consts, 1, ["x", "c"], [256, 1]), pool,
         "program too long"),
        ("17 slots", _mutated(prog, n_slots=17), pool, "too many slots"),
        ("one table entry short", prog, few_entries, "table entries out of range"),
        ("tab_start + tab_count past n_entries", prog, past_entries, "table entries out of range"),
        ("zero models", prog, ModelPool(np.zeros((2, 0, 8), dtype=np.uint32)), "empty model batch"),
        ("zero DAGs", _mutated(prog, prog_off=np.array([0], dtype=np.uint32)), pool, "empty DAG batch"),
    ]
    for what, bad_prog, bad_pool, message in cases:
        # (an empty batch has no output array to hand to the other two entry points)
        for call in ((dev.eval_upload,) if what.startswith("zero") else (dev.eval_terms, dev.eval_bits, dev.eval_upload)):
            with pytest.raises(MythGpuError) as e:
                call(bad_prog, bad_pool)
            assert "rc=-1" in str(e.value) and message in str(e.value), (what, str(e.value))
    good_still_works()


def test_a_refused_upload_leaves_the_previous_one_runnable(dev):
    """mg_eval_run after a refused mg_eval_upload evaluates the batch uploaded before
    it (every check of bv_upload comes before it replaces anything)."""
    prog, models = _good()
    pool = ModelPool.from_dicts(models, prog.var_names, prog.var_widths, prog.tables)
    want = np.array([[v & 1 for v in row] for row in values(prog, models)], dtype=bool)
    first, count, _ = sat_reference(want)
    dev.eval_upload(prog, pool)
    short = ModelPool(pool.values, pool.tab_start, pool.tab_count, pool.tab_entries[:-1], pool.tab_default)
    for bad_prog, bad_pool in ((prog, short), (_mutated(prog, 2, 1, ref(REF_VAR, 2)), pool)):
        with pytest.raises(MythGpuError):
            dev.eval_upload(bad_prog, bad_pool)
        dev.eval_run()
        fs, sc = dev.eval_download()
        assert np.array_equal(fs, first) and np.array_equal(sc, count)
