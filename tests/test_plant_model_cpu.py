"""tests/plantmodel.py (mg_harvest_upload) against a hand-worked case, against
harvestmodel.download as its inverse, the ABI's presence, and the hook loop
"explore, harvest the hooked lanes, acknowledge on the host, put them back,
resume" on the model: it must terminate and find every path before the loop is
run on a device (tests/test_gpu_plant.py runs the same program, sizes and loop
there, bounded by this file's iteration count).
"""
import dataclasses
import re
from collections import Counter

import numpy as np

import exploremodel
import forkmodel
import harvestmodel
import plantmodel
from mythril_amd import abi, native
from mythril_amd.lanes import MG_FENT_NONE, MG_HOOK, MG_LANE_HOOK_ACK, MG_RUNNING, LaneBatch
from test_harvest_model_cpu import (CHAIN, CHAIN_PATH_CAP, FINAL_STOP, FINISHED, PATH_LEN10, SHAPE10, SPARE_RECYCLE,
                                    _image10, chain_image, chain_step, finished_paths, model_one_shot)
from xfermodel import DeviceImage, live_diff, saturated, sentinel_filled, whole_diff

A5 = 0xA5


def _sentinel_model(shape):
    model = DeviceImage(shape)
    model.upload(sentinel_filled(shape), 0, shape.n)
    for f in ("trace_len", "rec_len", "fent", "n_nodes", "n_consts"):      # upload clips nothing of these here
        assert (getattr(model.img, f).view(np.uint8) == A5).all()
    return model


def _is_sentinel(a):
    return (np.ascontiguousarray(a).view(np.uint8) == A5).all()


# ---------------------------------------------------------------------- by hand
def test_upload_by_hand_bounds_defaults_and_untouched_cells():
    rng = np.random.default_rng(0x97A)
    model = _sentinel_model(SHAPE10)
    paths = exploremodel.Paths(10, 9)
    paths.path[:] = 0xA5A5A5A5
    paths.path_len[:] = 0xA5A5A5A5
    paths.root[:] = 0xA5A5A5A5
    lanes = [2, 7, 8]
    host = saturated(dataclasses.replace(SHAPE10, n=3), rng, 0)
    host.sp[:] = [2, 0, 4]                       # largest 4 of 6
    host.msize[:] = [0, 32, 0]                   # largest 32 of 96
    host.storage_count[:] = [1, 2, 0]            # largest 2 of 3
    host.trace_len[:] = [0, 2, 3]                # largest 3 of 5
    host.rec_len[:] = 0                          # nothing of the records
    host.n_nodes[:] = [3, 8, 1]                  # largest 8 of 9
    host.n_consts[:] = [1, 0, 3]                 # largest 3 of 4
    hpath = rng.integers(1, 1 << 32, size=(3, 9), dtype=np.uint32)
    hlen, hroot = np.array([2, 0, 3], dtype=np.uint32), np.array([1, 7, 0], dtype=np.uint32)
    plantmodel.upload(model, lanes, host, paths, (hpath, hlen, hroot))
    d = model.img
    # the scalars whole, the counters of the call
    assert d.pc[lanes].tolist() == host.pc.tolist() and d.gas_limit[lanes].tolist() == host.gas_limit.tolist()
    assert d.sp[lanes].tolist() == [2, 0, 4] and d.fent[lanes].tolist() == host.fent.tolist()
    assert d.trace_len[lanes].tolist() == [0, 2, 3] and d.rec_len[lanes].tolist() == [0, 0, 0]
    assert np.array_equal(d.env[lanes], host.env) and np.array_equal(d.calldata[lanes], host.calldata)
    # rows below the largest count of the three rows; the cell just above each bound kept
    for rows, k in (("stack", 4), ("memory", 32), ("storage", 2), ("trace", 3), ("rec", 0), ("node", 8), ("cval", 3),
                    ("stag", 4), ("mtag", 32), ("sttag", 2)):
        assert np.array_equal(getattr(d, rows)[lanes, :k], getattr(host, rows)[:, :k]), rows
        assert _is_sentinel(getattr(d, rows)[lanes, k:]) and getattr(d, rows)[lanes, k:k + 1].size, rows
    # unlisted lanes kept, every field
    others = [l for l in range(10) if l not in lanes]
    assert whole_diff(model.img, _sentinel_model(SHAPE10).img, lanes=others) == []
    assert _is_sentinel(paths.path[others]) and _is_sentinel(paths.path_len[others]) and _is_sentinel(paths.root[others])
    # the paths: rows below the call's largest path_len (3), tails inside it zero, the rest kept
    assert paths.path_len[lanes].tolist() == [2, 0, 3] and paths.root[lanes].tolist() == [1, 7, 0]
    assert paths.path[2, :2].tolist() == hpath[0, :2].tolist() and paths.path[2, 2] == 0
    assert not paths.path[7, :3].any() and paths.path[8, :3].tolist() == hpath[2, :3].tolist()
    assert _is_sentinel(paths.path[lanes, 3:])
    # a host image without fent, trace or records: the defaults
    model = _sentinel_model(SHAPE10)
    slim = saturated(dataclasses.replace(SHAPE10, n=3, trace_cap=0, rec_cap=0, stack_cap=3, node_cap=7), rng, 0)
    slim.fent = None
    slim.sp[:], slim.n_nodes[:] = 3, 7
    plantmodel.upload(model, lanes, slim)
    d = model.img
    assert d.fent[lanes].tolist() == [MG_FENT_NONE] * 3 and not d.trace_len[lanes].any() and not d.rec_len[lanes].any()
    assert _is_sentinel(d.trace[lanes]) and _is_sentinel(d.rec[lanes])
    assert np.array_equal(d.stack[lanes, :3], slim.stack) and _is_sentinel(d.stack[lanes, 3:])
    assert np.array_equal(d.node[lanes, :7], slim.node) and _is_sentinel(d.node[lanes, 7:])
    assert _is_sentinel(d.trace_len[others]) and _is_sentinel(d.fent[others])
    # no rows: nothing written
    model = _sentinel_model(SHAPE10)
    plantmodel.upload(model, [], LaneBatch(dataclasses.replace(SHAPE10, n=0)))
    assert whole_diff(model.img, _sentinel_model(SHAPE10).img) == []


def test_upload_of_a_download_is_the_identity_on_the_live_image():
    rng = np.random.default_rng(0x4A2)
    model = DeviceImage(SHAPE10)
    model.upload(saturated(SHAPE10, rng, 0), 0, 10)
    for f in ("status", "sp", "msize", "storage_count", "trace_len", "rec_len", "n_nodes", "n_consts"):
        getattr(model.img, f)[:] = getattr(_image10(), f)
    paths = exploremodel.Paths(10, 9)
    paths.path[:] = rng.integers(1, 1 << 32, size=paths.path.shape, dtype=np.uint32)
    paths.path_len[:] = PATH_LEN10
    before, paths_before = model.img.copy(), paths.copy()
    lanes, info = harvestmodel.select(model.img, FINISHED, path_len=paths.path_len)
    assert lanes.tolist() == [0, 2, 6, 7, 8, 9]
    host = LaneBatch(dataclasses.replace(SHAPE10, n=info.n))
    rows = harvestmodel.download(model, lanes, info, host, paths)
    model.img.sp[lanes] = 0                      # the image moves on, the host rows come back
    model.img.stack[lanes] = 0
    plantmodel.upload(model, lanes, host, paths, rows)
    assert live_diff(model.img, before) == []
    others = [l for l in range(10) if l not in lanes.tolist()]
    assert whole_diff(model.img, before, lanes=others) == []
    assert np.array_equal(paths.path_len, paths_before.path_len) and np.array_equal(paths.root, paths_before.root)
    for l in range(10):
        k = int(paths.path_len[l])
        assert np.array_equal(paths.path[l, :k], paths_before.path[l, :k])
    # into other lanes: the same live image there
    other = DeviceImage(SHAPE10)
    other.upload(sentinel_filled(SHAPE10), 0, 10)
    dest = [1, 3, 4, 5, 7, 9]
    plantmodel.upload(other, dest, host)
    moved, orig = LaneBatch(dataclasses.replace(SHAPE10, n=6)), LaneBatch(dataclasses.replace(SHAPE10, n=6))
    for f in moved._fields():
        getattr(moved, f)[...] = getattr(other.img, f)[dest]
        getattr(orig, f)[...] = getattr(before, f)[lanes]
    assert live_diff(moved, orig) == []


# ------------------------------------------------------------------- the ABI
def test_the_header_declares_the_call_and_native_carries_it():
    text = abi.HEADER.read_text()
    m = re.search(r"\bint\s+mg_harvest_upload\s*\(([^;]*)\)\s*;", text)
    assert m, "include/mythgpu.h does not declare mg_harvest_upload"
    args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
    assert len(args) == 7
    res, argtypes = native.SIGNATURES["mg_harvest_upload"]
    assert len(argtypes) == 7 and res is native.SIGNATURES["mg_harvest_download"][0]
    assert abi.MG_ABI_VERSION == 15


# ------------------------------------------------------------- the hook loop
def hook_step(img):
    """chain_step under a hook mask with JUMPDEST set: a running lane that stands on a
    pad's JUMPDEST and has not been acknowledged stops MG_HOOK there (aux: the
    opcode, no step counted); an acknowledged one executes it (the flag is cleared)
    and halts at the STOP."""
    on_pad = (img.status == MG_RUNNING) & (img.pc > FINAL_STOP)
    hooked = on_pad & ((img.flags & MG_LANE_HOOK_ACK) == 0)
    img.status[hooked], img.aux[hooked] = MG_HOOK, 0x5B
    img.flags[on_pad & ~hooked] &= ~np.uint32(MG_LANE_HOOK_ACK)
    chain_step(img)


def resolve(host):
    """What the host does with harvested MG_HOOK rows: fire the hooks, acknowledge."""
    assert (host.status == MG_HOOK).all()
    host.status[:] = MG_RUNNING
    host.flags[:] |= MG_LANE_HOOK_ACK


def move_to_free(free, lanes, host, rows):
    """The resolved rows go into lanes from the front of the free list, as many as it
    holds (the rest stay where they were), and the lanes they leave join it.  Returns
    (destination lanes ascending, host and rows in that order, the new free list)."""
    lanes = [int(x) for x in lanes]
    k = min(len(free), len(lanes))
    dest = list(free[:k]) + lanes[k:]
    order = np.argsort(np.array(dest), kind="stable")
    for f in host._fields():
        getattr(host, f)[...] = getattr(host, f)[order]
    rows = tuple(np.ascontiguousarray(r[order]) for r in rows)
    return np.array(dest, dtype=np.uint32)[order], host, rows, harvestmodel.merge_free(free[k:], lanes[:k])


def model_hook_loop(in_place: bool):
    """(finished paths, iterations) of the hook loop on the model.  in_place: the
    resolved rows go back into the lanes they came from; else into lanes taken from
    the free list, the old lanes joining it."""
    model, free = chain_image(SPARE_RECYCLE)
    codes = {0: forkmodel.CodeTable(CHAIN)}
    paths = exploremodel.Paths(model.shape.n, CHAIN_PATH_CAP)
    out, iterations = [], 0
    while True:
        iterations += 1
        assert iterations <= 200, "the hook loop does not terminate"
        _, _, used, _ = harvestmodel.explore(model, codes, free, paths, 2, hook_step, resume=True)
        free = free[used:]
        lanes, info = harvestmodel.select(model.img, 1 << MG_HOOK, skip=free, path_len=paths.path_len)
        if info.n:
            host = LaneBatch(dataclasses.replace(model.shape, n=info.n))
            rows = harvestmodel.download(model, lanes, info, host, paths)
            resolve(host)
            dest = lanes
            if not in_place:
                dest, host, rows, free = move_to_free(free, lanes, host, rows)
            plantmodel.upload(model, dest, host, paths, rows)
        lanes, info = harvestmodel.select(model.img, FINISHED & ~(1 << MG_HOOK), skip=free, path_len=paths.path_len)
        host = LaneBatch(dataclasses.replace(model.shape, n=info.n))
        got = harvestmodel.download(model, lanes, info, host, paths)
        if info.n:
            out += finished_paths(host, lanes, *got)
        free = harvestmodel.merge_free(free, lanes)
        if len(free) == model.shape.n:
            return out, iterations


def test_the_hook_loop_finds_the_paths_of_the_unhooked_run():
    want = Counter(model_one_shot())
    for in_place in (True, False):
        got, iterations = model_hook_loop(in_place)
        assert len(got) == 56 and Counter(got) == want, in_place
        print(f"hook loop, {'in place' if in_place else 'into free lanes'}: {iterations} iterations")
