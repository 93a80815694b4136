"""tests/harvestmodel.py against hand-worked cases, and the recycle loop
"explore, harvest what finished, put those lanes into the free list, explore
again" on the model: it must terminate and find every path before the loop is
run on a device (tests/test_gpu_harvest.py runs the same program, sizes and loop
there).
"""
import dataclasses
from collections import Counter

import numpy as np

import exploremodel
import forkmodel
import harvestmodel
from mythril_amd.lanes import (MG_DEPTH, MG_ESCAPE, MG_FORK, MG_HALT_END, MG_HALT_RETURN, MG_HALT_REVERT, MG_HALT_STOP,
                               MG_HOOK, MG_LANE_SYMBOLIC, MG_LANE_SYMCD, MG_RUNNING, MG_VMEXC, LaneBatch, LaneShape,
                               word_to_limbs)
from xfermodel import DeviceImage, saturated, sentinel_filled

# ------------------------------------------------------------------ selection by hand
SHAPE10 = LaneShape(n=10, stack_cap=6, mem_cap=96, calldata_cap=8, storage_cap=3, trace_cap=5, rec_cap=7, node_cap=9,
                    const_cap=4)
#            lane:   0           1             2        3               4           5        6             7
STATUS10 = [MG_HALT_STOP, MG_RUNNING, MG_HALT_RETURN, MG_FORK, harvestmodel.NEVER_UPLOADED, 40, MG_HALT_STOP, MG_ESCAPE,
            MG_HALT_STOP, MG_HALT_REVERT]            # 8, 9
FINISHED = 0xFFFFFFFF & ~(1 << MG_RUNNING) & ~(1 << MG_FORK)


def _image10():
    img = LaneBatch(SHAPE10)
    img.status[:] = np.array(STATUS10, dtype=np.uint32)
    img.sp[:] = [1, 6, 2, 6, 6, 6, 3, 0, 4, 5]
    img.msize[:] = [32, 96, 0, 96, 96, 96, 64, 0, 32, 0]
    img.storage_count[:] = [0, 3, 1, 3, 3, 3, 0, 2, 0, 0]
    img.trace_len[:] = [5, 5, 0, 5, 5, 5, 1, 2, 3, 4]
    img.rec_len[:] = [0, 7, 0, 7, 7, 7, 6, 0, 0, 0]
    img.n_nodes[:] = [2, 9, 3, 9, 9, 9, 0, 8, 1, 0]
    img.n_consts[:] = [0, 4, 1, 4, 4, 4, 2, 0, 3, 0]
    return img


PATH_LEN10 = np.array([0, 9, 2, 9, 9, 9, 1, 0, 3, 7], dtype=np.uint32)


def test_selection_by_hand():
    img = _image10()
    # every finished status: lanes 0, 2, 6, 7, 8, 9 (1 runs, 3 is MG_FORK, 4 was never uploaded, 5 holds 40 >= 32)
    lanes, info = harvestmodel.select(img, FINISHED, path_len=PATH_LEN10)
    assert lanes.tolist() == [0, 2, 6, 7, 8, 9]
    assert info.key() == (6, 6, 5, 64, 2, 5, 6, 8, 3, 7)
    # the cap: the lowest three win, the maxima are theirs alone
    lanes, info = harvestmodel.select(img, FINISHED, max_lanes=3, path_len=PATH_LEN10)
    assert lanes.tolist() == [0, 2, 6] and info.key() == (3, 6, 3, 64, 1, 5, 6, 3, 2, 2)
    # skip takes lanes out before the ranking
    lanes, info = harvestmodel.select(img, FINISHED, skip=[0, 1, 6], max_lanes=3, path_len=PATH_LEN10)
    assert lanes.tolist() == [2, 7, 8] and info.key() == (3, 4, 4, 32, 2, 3, 0, 8, 3, 3)
    # one status; several; none; a cap of 0; a cap above the batch
    assert harvestmodel.select(img, 1 << MG_HALT_STOP)[0].tolist() == [0, 6, 8]
    assert harvestmodel.select(img, 1 << MG_HALT_RETURN | 1 << MG_HALT_REVERT | 1 << MG_FORK)[0].tolist() == [2, 3, 9]
    for lanes, info in (harvestmodel.select(img, 0, path_len=PATH_LEN10),
                        harvestmodel.select(img, FINISHED, max_lanes=0, path_len=PATH_LEN10)):
        assert lanes.size == 0 and info.key()[0] == 0 and info.key()[2:] == (0,) * 8
    assert harvestmodel.select(img, 0)[1].matched == 0
    assert harvestmodel.select(img, FINISHED, max_lanes=0)[1].matched == 6
    assert harvestmodel.select(img, FINISHED, max_lanes=1000)[0].tolist() == [0, 2, 6, 7, 8, 9]
    # all ones never reaches lane 4 (never uploaded) or lane 5 (a status above 31)
    assert harvestmodel.select(img, 0xFFFFFFFF)[0].tolist() == [0, 1, 2, 3, 6, 7, 8, 9]
    # absent planes give 0
    plain = dataclasses.replace(SHAPE10, trace_cap=0, rec_cap=0, node_cap=0, const_cap=0)
    b = LaneBatch(plain)
    b.status[:] = MG_HALT_STOP
    b.sp[:] = 2
    b.trace_len[:] = 9                                       # not a plane of this batch
    _, info = harvestmodel.select(b, FINISHED)
    assert info.key() == (10, 10, 2, 0, 0, 0, 0, 0, 0, 0)


# ------------------------------------------------------------------- download by hand
def test_download_by_hand_bounds_clipping_and_untouched_cells():
    rng = np.random.default_rng(0x4A1)
    model = DeviceImage(SHAPE10)
    model.upload(saturated(SHAPE10, rng, 0), 0, 10)
    for f in ("status", "sp", "msize", "storage_count", "trace_len", "rec_len", "n_nodes", "n_consts"):
        getattr(model.img, f)[:] = getattr(_image10(), f)
    paths = exploremodel.Paths(10, 9)
    paths.path[:] = rng.integers(1, 1 << 32, size=paths.path.shape, dtype=np.uint32)
    paths.path_len[:] = PATH_LEN10
    paths.root[:] = [3, 3, 1, 0, 9, 9, 6, 7, 0, 2]
    lanes, info = harvestmodel.select(model.img, FINISHED, skip=[0, 1, 6], max_lanes=3, path_len=paths.path_len)
    assert lanes.tolist() == [2, 7, 8]
    # a full-capacity host image: rows below the selection's maxima, the sentinel above
    host = sentinel_filled(dataclasses.replace(SHAPE10, n=3))
    path, path_len, root = harvestmodel.download(model, lanes, info, host, paths)
    d = model.img
    assert host.status.tolist() == [MG_HALT_RETURN, MG_ESCAPE, MG_HALT_STOP] and host.gas_max.tolist() == d.gas_max[lanes].tolist()
    assert np.array_equal(host.stack[:, :4], d.stack[lanes, :4]) and (host.stack[:, 4:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(host.memory[:, :32], d.memory[lanes, :32]) and (host.memory[:, 32:] == 0xA5).all()
    assert np.array_equal(host.storage[:, :2], d.storage[lanes, :2]) and (host.storage[:, 2:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(host.trace[:, :3], d.trace[lanes, :3]) and (host.trace[:, 3:].view(np.uint8) == 0xA5).all()
    assert (host.rec.view(np.uint8) == 0xA5).all() and host.rec_len.tolist() == [0, 0, 0]      # info.rec_len == 0
    assert np.array_equal(host.node[:, :8], d.node[lanes, :8]) and (host.node[:, 8:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(host.stag[:, :4], d.stag[lanes, :4]) and (host.stag[:, 4:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(host.mtag[:, :32], d.mtag[lanes, :32]) and (host.mtag[:, 32:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(host.sttag[:, :2], d.sttag[lanes, :2]) and (host.sttag[:, 2:].view(np.uint8) == 0xA5).all()
    assert np.array_equal(host.env, d.env[lanes]) and np.array_equal(host.calldata, d.calldata[lanes])
    assert path_len.tolist() == [2, 0, 3] and root.tolist() == [1, 7, 0]
    assert np.array_equal(path[0, :2], paths.path[2, :2]) and not path[0, 2:].any() and not path[1].any()
    assert np.array_equal(path[2, :3], paths.path[8, :3]) and not path[2, 3:].any()
    # a slim host image one below two of the maxima: the capacity clips, the rest is as before
    slim = sentinel_filled(dataclasses.replace(SHAPE10, n=3, stack_cap=3, node_cap=7))
    harvestmodel.download(model, lanes, info, slim, None)
    assert np.array_equal(slim.stack, d.stack[lanes, :3]) and np.array_equal(slim.stag, d.stag[lanes, :3])
    assert np.array_equal(slim.node, d.node[lanes, :7]) and np.array_equal(slim.memory[:, :32], d.memory[lanes, :32])
    # nothing selected: nothing written
    empty = sentinel_filled(dataclasses.replace(SHAPE10, n=0))
    assert harvestmodel.download(model, [], harvestmodel.Info(), empty, paths) is None


# ------------------------------------------------------------- the chain program
# Six JUMPIs on symbolic conditions in sequence.  Level k (k = 0..5), at byte address 6k:
#   PUSH1 32k  CALLDATALOAD  PUSH1 pad_k  JUMPI        instruction indices 4k .. 4k + 3
# then STOP at index 24 (address 36), then pad k = JUMPDEST STOP at indices 25 + 2k, 26 + 2k
# (addresses 37 + 2k, 38 + 2k).  The jump side of level k lands on its pad and stops; the
# fall-through goes on to level k + 1 and stops after the sixth.
DEPTH = 6
PAD = [37 + 2 * k for k in range(DEPTH)]
CHAIN = b"".join(bytes([0x60, 32 * k, 0x35, 0x60, PAD[k], 0x57]) for k in range(DEPTH)) + b"\x00" + b"\x5b\x00" * DEPTH
FINAL_STOP = 4 * DEPTH
ROOTS, SPARE_ONE_SHOT, SPARE_RECYCLE = 8, 48, 4
PATHS_PER_ROOT = DEPTH + 1
MAX_ITERATIONS = 40
CHAIN_PATH_CAP = 8
# gas (min = max) of PUSH1, CALLDATALOAD and JUMPDEST (support/opcodes.py); the JUMPI's 10 is the fork's
G_PUSH, G_CDLOAD, G_JUMPDEST = 3, 3, 1


def chain_step(img):
    """The stepping launch of the chain program, by hand: every MG_RUNNING lane runs
    to its next stop.  At level k < 6 that is the JUMPI, MG_FORK, with the target
    and the condition (a new arena node over a new constant) pushed; on a pad or at
    the final STOP the lane halts MG_HALT_STOP at the STOP (a halt counts one step)."""
    for l in np.nonzero(img.status == MG_RUNNING)[0]:
        pc = int(img.pc[l])
        if pc < FINAL_STOP:
            assert pc % 4 == 0
            k, sp, nn = pc // 4, int(img.sp[l]), int(img.n_nodes[l])
            img.stack[l, sp] = 0
            img.stag[l, sp] = 1 + nn                         # the condition: calldata word 32k
            img.stack[l, sp + 1] = word_to_limbs(PAD[k])
            img.stag[l, sp + 1] = 0
            img.sp[l], img.n_nodes[l], img.n_consts[l] = sp + 2, nn + 1, int(img.n_consts[l]) + 1
            img.pc[l], img.status[l], img.aux[l] = pc + 3, MG_FORK, 0x57
            img.steps[l] += 3
            img.gas_min[l] += 2 * G_PUSH + G_CDLOAD
            img.gas_max[l] += 2 * G_PUSH + G_CDLOAD
        else:
            on_pad = pc > FINAL_STOP
            img.pc[l] = pc + 1 if on_pad else pc
            img.steps[l] += 2 if on_pad else 1
            img.gas_min[l] += G_JUMPDEST if on_pad else 0
            img.gas_max[l] += G_JUMPDEST if on_pad else 0
            img.status[l], img.aux[l] = MG_HALT_STOP, 0


def chain_image(spare: int):
    shape = LaneShape(n=ROOTS + spare, stack_cap=4, mem_cap=32, calldata_cap=32, storage_cap=1, node_cap=8, const_cap=8)
    b = LaneBatch(shape)
    b.status[:] = MG_HALT_STOP                               # the spare lanes: halted and in the free list
    for l in range(ROOTS):
        b.set_lane(l, code_id=0, flags=MG_LANE_SYMBOLIC | MG_LANE_SYMCD)
    model = DeviceImage(shape)
    model.upload(b, 0, shape.n)
    return model, list(range(ROOTS, shape.n))


def finished_paths(img, lanes, path, path_len, root):
    """(root, path entries, status, pc, sp, steps, gas_min, gas_max, n_nodes) per harvested row."""
    return [(int(root[i]), tuple(int(x) for x in path[i, :int(path_len[i])]), int(img.status[i]), int(img.pc[i]),
             int(img.sp[i]), int(img.steps[i]), int(img.gas_min[i]), int(img.gas_max[i]), int(img.n_nodes[i]))
            for i in range(len(lanes))]


def model_one_shot():
    model, free = chain_image(SPARE_ONE_SHOT)
    codes = {0: forkmodel.CodeTable(CHAIN)}
    paths = exploremodel.Paths(model.shape.n, CHAIN_PATH_CAP)
    rounds, forks, used, starved = harvestmodel.explore(model, codes, free, paths, 64, chain_step, resume=False)
    assert (forks, used, starved.size) == (ROOTS * DEPTH, ROOTS * DEPTH, 0) and rounds == DEPTH + 1
    lanes, info = harvestmodel.select(model.img, FINISHED, skip=free[used:], path_len=paths.path_len)
    host = LaneBatch(dataclasses.replace(model.shape, n=info.n))
    got = harvestmodel.download(model, lanes, info, host, paths)
    return finished_paths(host, lanes, *got)


def model_recycle():
    """(finished paths, iterations) of the recycling run on the model."""
    model, free = chain_image(SPARE_RECYCLE)
    codes = {0: forkmodel.CodeTable(CHAIN)}
    paths = exploremodel.Paths(model.shape.n, CHAIN_PATH_CAP)       # root[l] = l, as an upload of it leaves them
    out, iterations = [], 0
    while True:
        iterations += 1
        assert iterations <= MAX_ITERATIONS, "the recycle loop does not terminate"
        _, _, used, _ = harvestmodel.explore(model, codes, free, paths, 2, chain_step, resume=True)
        free = free[used:]
        lanes, info = harvestmodel.select(model.img, FINISHED, skip=free, path_len=paths.path_len)
        host = LaneBatch(dataclasses.replace(model.shape, n=info.n))
        got = harvestmodel.download(model, lanes, info, host, paths)
        if info.n:
            out += finished_paths(host, lanes, *got)
        free = harvestmodel.merge_free(free, lanes)
        alive = [l for l in range(model.shape.n) if l not in set(free)]
        if not alive:
            return out, iterations


def test_the_chain_code_is_what_the_comment_says():
    t = forkmodel.CodeTable(CHAIN)
    assert t.n == 4 * DEPTH + 1 + 2 * DEPTH and t.addrs[FINAL_STOP] == 6 * DEPTH
    for k in range(DEPTH):
        assert t.addrs[4 * k + 3] == 6 * k + 5 and t.resolve(PAD[k]) == FINAL_STOP + 1 + 2 * k
        assert t.jumpdest[FINAL_STOP + 1 + 2 * k] and not t.jumpdest[FINAL_STOP + 2 + 2 * k]


def test_one_shot_finds_seven_paths_per_root():
    got = model_one_shot()
    assert len(got) == ROOTS * PATHS_PER_ROOT == 56
    by_root = Counter(g[0] for g in got)
    assert by_root == {r: PATHS_PER_ROOT for r in range(ROOTS)}
    # per root: the jump side of level k after k fall-throughs, and six fall-throughs
    sides = sorted(tuple(e & 1 for e in g[1]) for g in got if g[0] == 0)
    assert sides == sorted([(0,) * k + (1,) for k in range(DEPTH)] + [(0,) * DEPTH])
    # the condition of level k is arena node k of every lane of the lineage
    assert all(tuple(e >> 1 for e in g[1]) == tuple(range(1, len(g[1]) + 1)) for g in got)


def test_the_recycle_loop_terminates_and_finds_the_same_paths():
    got, iterations = model_recycle()
    assert iterations <= MAX_ITERATIONS
    assert len(got) == 56 and Counter(got) == Counter(model_one_shot())
    print(f"recycle loop: {iterations} iterations for {len(got)} finished paths with {SPARE_RECYCLE} spare lanes")


def test_resume_keeps_the_paths_and_explore_resets_them():
    codes = {0: forkmodel.CodeTable(CHAIN)}
    runs = {}
    for resume in (True, False):
        model, free = chain_image(SPARE_ONE_SHOT)
        paths = exploremodel.Paths(model.shape.n, CHAIN_PATH_CAP)
        _, _, used, _ = harvestmodel.explore(model, codes, free, paths, 2, chain_step, resume=False)
        before = paths.copy()
        assert before.path_len[:ROOTS].tolist() == [2] * ROOTS
        harvestmodel.explore(model, codes, free[used:], paths, 1, chain_step, resume=resume)
        runs[resume] = (before, paths)
    before, after = runs[True]
    assert after.path_len[:ROOTS].tolist() == [3] * ROOTS and np.array_equal(after.path[:ROOTS, :2], before.path[:ROOTS, :2])
    assert after.root[ROOTS:ROOTS + 3 * ROOTS].tolist() == list(range(ROOTS)) * 3
    before, after = runs[False]
    assert after.path_len[:ROOTS].tolist() == [1] * ROOTS and after.root[:3 * ROOTS].tolist() == list(range(3 * ROOTS))
    assert after.root[3 * ROOTS:4 * ROOTS].tolist() == list(range(ROOTS)) and not after.path_len[ROOTS:3 * ROOTS].any()


STATUSES_SEEN = (MG_HALT_STOP, MG_HALT_RETURN, MG_HALT_REVERT, MG_HALT_END, MG_VMEXC, MG_HOOK, MG_ESCAPE, MG_DEPTH)


def test_finished_mask_is_every_status_but_running_and_fork():
    assert all(FINISHED >> s & 1 for s in STATUSES_SEEN) and not FINISHED >> MG_RUNNING & 1 and not FINISHED >> MG_FORK & 1
