"""The layout of the workgroups that ride in the substep's launches (mpmavatar_amd/csrc/launch_layout.hpp) without a GPU: the
header compiled with g++ (tests/hostlayout/hostlayout.cpp), the host's layout function and the kernels' own decode walked over
every blockIdx of the launch, for the product of the counts below.  127 / 128 / 129 chunks straddle one period of the XCD remap
(8 x XCD_RUN = 128)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import hostbuild

FACE_BINS = (0, 1, 7, 8, 9)
JOINT_WGS = (0, 1, 8)
CHUNKS = (0, 1, 127, 128, 129, 300)
CLEAR_WGS = (0, 1, 5)
PACK_WGS = (0, 3)
CAP = 1024


@pytest.fixture(scope="module")
def lib():
    return hostbuild.host_lib("hostlayout")


@pytest.fixture(scope="module")
def kinds(lib):
    k = (C.c_int32 * 6)()
    lib.hl_kinds(k)
    return dict(zip(("face", "joint", "pad", "chunk", "clear", "pack"), k))


def _layout(lib, counts):
    out = (C.c_int32 * 6)()
    lib.hl_layout(*counts, out)
    return dict(zip(("n_riders", "z_first", "pack_first", "n_scatter", "n_clear", "grid"), out))


def _walk(lib, counts):
    kind, index = np.full(CAP, -7, np.int32), np.full(CAP, -7, np.int32)
    grid = lib.hl_walk(*counts, CAP, kind.ctypes.data_as(C.POINTER(C.c_int32)), index.ctypes.data_as(C.POINTER(C.c_int32)))
    assert 0 <= grid <= CAP
    return kind[:grid], index[:grid]


def _check(lib, kinds, counts):
    n_fbins, n_joint, n_chunks, n_clear, n_pack = counts
    run = lib.hl_xcd_run()
    L = _layout(lib, counts)
    kind, index = _walk(lib, counts)
    grid = len(kind)
    assert grid == L["grid"]
    # every workgroup has exactly one role, and a known one
    assert set(kind.tolist()) <= set(kinds.values())
    # each role's indices are 0 .. count - 1, each once; padding and the holes of the remap get nothing
    want = {"face": n_fbins, "joint": n_joint, "chunk": n_chunks, "clear": n_clear, "pack": n_pack}
    for name, n in want.items():
        idx = index[kind == kinds[name]]
        if name == "chunk":
            idx = idx[idx >= 0]
            assert np.all(index[(kind == kinds["chunk"]) & (index < 0)] == -1)
        assert sorted(idx.tolist()) == list(range(n)), (counts, name)
    # the documented order: face bins, joints, padding, chunk slots, clearing, pack -- each kind one contiguous run
    order = [kinds[k] for k in ("face", "joint", "pad", "chunk", "clear", "pack")]
    rank = np.array([order.index(k) for k in kind.tolist()], np.int64)
    assert np.all(np.diff(rank) >= 0), counts
    # ... and inside a run the face bins, joints, clearing and pack workgroups count up from 0
    for name in ("face", "joint", "clear", "pack"):
        idx = index[kind == kinds[name]]
        assert idx.tolist() == list(range(len(idx))), (counts, name)
    # where the runs begin is what the layout says
    n_front = int(np.sum(rank < 3))
    assert n_front == L["n_riders"] and n_front % 8 == 0 and 0 <= n_front - (n_fbins + n_joint) < 8
    assert int(np.sum(rank < 4)) == L["z_first"] == L["n_scatter"]
    assert int(np.sum(rank < 5)) == L["pack_first"]
    assert L["n_clear"] == n_clear
    # scattering workgroups + clearing + pack = the launch
    assert L["n_scatter"] + n_clear + n_pack == grid
    # the chunk slots are whole periods of the remap, and chunk i runs on XCD (i / XCD_RUN) % 8 (workgroup id % 8): the padding of
    # the riders keeps that mapping
    n_slots = int(np.sum(kind == kinds["chunk"]))
    assert n_slots % (8 * run) == 0 and n_chunks <= n_slots < n_chunks + 8 * run
    bid = np.nonzero((kind == kinds["chunk"]) & (index >= 0))[0]
    assert np.array_equal(bid % 8, (index[bid] // run) % 8), counts


def test_every_blockidx_has_one_role(lib, kinds):
    n = 0
    for counts in itertools.product(FACE_BINS, JOINT_WGS, CHUNKS, CLEAR_WGS, PACK_WGS):
        _check(lib, kinds, counts)
        n += 1
    assert n == 5 * 3 * 6 * 3 * 2 and lib.hl_xcd_run() * 8 == 128


def test_riders_only_form(lib, kinds):
    """a launch of riders alone (a phase of a profiling run, the splat pass in front of the stress launch): the same function with
    no chunks -- no chunk slot and no clearing workgroup, the grid is the padded rider count"""
    for n_fbins, n_joint in itertools.product(FACE_BINS, JOINT_WGS):
        counts = (n_fbins, n_joint, 0, 0, 0)
        _check(lib, kinds, counts)
        kind, _ = _walk(lib, counts)
        L = _layout(lib, counts)
        assert kinds["chunk"] not in kind and kinds["clear"] not in kind and kinds["pack"] not in kind
        assert len(kind) == L["n_riders"] == L["z_first"] == (n_fbins + n_joint + 7) // 8 * 8
