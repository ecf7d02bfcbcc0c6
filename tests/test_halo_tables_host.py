"""The per-peer tables of the multi-GPU exchange (mpmavatar_amd/csrc/halo_tables.hpp) without a GPU: the header compiled with g++
(tests/hostdist/hostdist.cpp) and its builders fed fabricated peer lists -- every pointer a made-up address, never dereferenced.

What a table must hold is worked out HERE from the documented layout, not with the header's functions:
  * a halo record is n_blocks x CH x 64 floats, CH = 8 with a particle mover and 4 without; a ghost record has one item per id;
    one workgroup of 256 threads serves 256 floats / ids, so peer k of a table owns ceil(items / 256) workgroups from wg_off[k]
  * a peer with nothing to exchange takes no slot of a HaloTab / GhostTab; HaloIn is indexed by the peer's position instead
  * a pair's halo goes through its link when the links are in use, the neighbour's arena is mapped and the shared blocks fit it
    (n_blocks <= link_cap); otherwise through halo_send / halo_recv with no flag and no counter
  * an arena is [flag of parity 0 | flag of parity 1 | data of parity 0 | data of parity 1]: the flags 16 ints (64 bytes) apart, the
    data from float 32, link_cap x 8 x 64 floats per parity whatever CH is; the parity of a substep is the lowest bit of its sequence
    number, which is unsigned and wraps; the sender writes the NEIGHBOUR's arena (link_remote), the receiver reads its own (link_local)
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import hostbuild

PEER_FIELDS = ("n_blocks", "blocks", "halo_send", "halo_recv", "n_send_p", "n_recv_p", "n_send_e", "n_recv_e", "send_p", "recv_p",
               "send_e", "recv_e", "ghost_send", "ghost_recv", "link_local", "link_remote", "link_cap", "link_cnt")
POINTERS = ("blocks", "halo_send", "halo_recv", "send_p", "recv_p", "send_e", "recv_e", "ghost_send", "ghost_recv", "link_local",
            "link_remote", "link_cnt")
TAB, WG = 8, 256                 # peers per table, threads per workgroup
LINK_CAP = 5                     # blocks an arena of the fabricated links holds
SEQS = (0, 1, 2**31 - 1, 2**31)  # the last two: where a signed reading of the parity or of the flag value would flip
i64p = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lib():
    L = hostbuild.host_lib("hostdist")
    for f in (L.hd_link_arena_floats, L.hd_halo_floats, L.hd_ghost_floats):
        f.restype = C.c_int64
    L.hd_halo_floats.argtypes = [C.c_int64, C.c_int32]
    L.hd_ghost_floats.argtypes = [C.c_int64, C.c_int64]
    L.hd_halo_tab.argtypes = [i64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, i64p]
    L.hd_halo_in.argtypes = [i64p, C.c_int32, C.c_int64, C.c_int32, C.c_uint32, C.c_int32, i64p]
    L.hd_ghost_tab.argtypes = [i64p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i64p]
    return L


def make_peer(i, n_blocks=0, link=True, link_local=True, link_cap=LINK_CAP, ghosts=(0, 0, 0, 0)):
    """peer i of a list: distinct made-up addresses, 4 KiB apart inside the peer's own 1 MiB, far below 2^47"""
    base = 0x100000000 + i * 0x100000
    p = {f: base + 0x1000 * (k + 1) for k, f in enumerate(POINTERS)}
    p.update(n_blocks=n_blocks, link_cap=link_cap if link else 0)
    p["n_send_p"], p["n_recv_p"], p["n_send_e"], p["n_recv_e"] = ghosts
    if not link:
        p["link_remote"] = p["link_cnt"] = 0
    if not (link and link_local):
        p["link_local"] = 0
    return p


def pack(peers):
    a = np.array([[p[f] for f in PEER_FIELDS] for p in peers], np.int64).reshape(-1)
    return a if len(a) else np.zeros(1, np.int64)


def halo_tab(lib, peers, i0, send, movers, seq, link_on, wide=0):
    out = np.full(3 + TAB + 1 + 5 * TAB, -7, np.int64)
    lib.hd_halo_tab(pack(peers).ctypes.data_as(i64p), len(peers), i0, int(send), int(movers), seq, int(link_on), wide, out.ctypes.data_as(i64p))
    cut = np.split(out[3:], np.cumsum([TAB + 1, TAB, TAB, TAB, TAB]))
    return dict(n=int(out[0]), with_mov=int(out[1]), seq=int(out[2]), wg_off=cut[0], blocks=cut[1], n_blocks=cut[2], buf=cut[3], sig=cut[4],
                cnt=cut[5])


def halo_in(lib, peers, slot, movers, seq, wide=0):
    out = np.full(4 + 2 * TAB, -7, np.int64)
    lib.hd_halo_in(pack(peers).ctypes.data_as(i64p), len(peers), slot, int(movers), seq, wide, out.ctypes.data_as(i64p))
    return dict(slot=int(out[0]), n_peers=int(out[1]), seq=int(out[2]), ch=int(out[3]), buf=out[4:4 + TAB], sig=out[4 + TAB:])


def ghost_tab(lib, peers, i0, send, wide=0):
    out = np.full(1 + TAB + 1 + 5 * TAB, -7, np.int64)
    lib.hd_ghost_tab(pack(peers).ctypes.data_as(i64p), len(peers), i0, int(send), wide, out.ctypes.data_as(i64p))
    cut = np.split(out[1:], np.cumsum([TAB + 1, TAB, TAB, TAB, TAB]))
    return dict(n=int(out[0]), wg_off=cut[0], ids_p=cut[1], ids_e=cut[2], n_p=cut[3], n_e=cut[4], buf=cut[5])


def as_int32(seq):
    return (seq + 2**31) % 2**32 - 2**31


def arena_data(arena, seq, cap):
    return arena + 4 * (32 + (seq & 1) * cap * 8 * 64)


def arena_flag(arena, seq):
    return arena + 4 * (seq & 1) * 16


def check_offsets(tb, items):
    """wg_off of a table against the items (floats / ids) of its non-empty peers, in order"""
    assert tb["n"] == len(items)
    assert tb["wg_off"][0] == 0
    for k, n in enumerate(items):
        assert n > 0
        assert tb["wg_off"][k + 1] - tb["wg_off"][k] == -(-n // WG) >= 1, (k, n)
    assert np.all(np.diff(tb["wg_off"][:len(items) + 1]) > 0)        # monotone: every slot has workgroups
    assert np.all(tb["wg_off"][len(items) + 1:] == 0)                 # nothing behind the last slot


def check_halo_tab(tb, peers, i0, send, movers, seq, link_on):
    ch = 8 if movers else 4
    mine = [p for p in peers[i0:i0 + TAB] if p["n_blocks"]]         # empty peers leave no slot
    assert tb["with_mov"] == int(movers) and tb["seq"] == as_int32(seq)
    check_offsets(tb, [p["n_blocks"] * ch * 64 for p in mine])
    for k, p in enumerate(mine):
        assert tb["blocks"][k] == p["blocks"] and tb["n_blocks"][k] == p["n_blocks"]
        linked = link_on and p["link_remote"] != 0 and p["n_blocks"] <= p["link_cap"]
        if linked:
            arena = p["link_remote"] if send else p["link_local"]
            assert tb["buf"][k] == arena_data(arena, seq, p["link_cap"]), (k, seq)
            assert tb["sig"][k] == arena_flag(arena, seq) and tb["cnt"][k] == p["link_cnt"]
        else:
            assert tb["buf"][k] == (p["halo_send"] if send else p["halo_recv"])
            assert tb["sig"][k] == 0 and tb["cnt"][k] == 0
    for name in ("blocks", "n_blocks", "buf", "sig", "cnt"):
        assert np.all(tb[name][len(mine):] == 0), name


def shapes():
    """every block count the link rule tells apart, with a mapped link and without one"""
    peers = [make_peer(i, n_blocks=nb) for i, nb in enumerate((0, 1, 3, LINK_CAP, LINK_CAP + 1))]
    return peers + [make_peer(5, n_blocks=3, link=False), make_peer(6, n_blocks=0, link=False)]


def test_constants_and_record_sizes(lib):
    c = (C.c_int32 * 6)()
    lib.hd_consts(c)
    assert list(c) == [TAB, WG, 32, 16, 8, len(PEER_FIELDS)]
    for cap in (1, LINK_CAP, 1024):
        assert lib.hd_link_arena_floats(cap) == 32 + 2 * cap * 8 * 64
    for nb, movers in itertools.product((0, 1, 3, 1000), (0, 1)):
        assert lib.hd_halo_floats(nb, movers) == nb * (8 if movers else 4) * 64
    assert lib.hd_ghost_floats(7, 5) == 6 * 7 + 3 * 5
    # the flags and the first data word of an arena do not overlap, nor do the two parities
    assert 4 * 16 + 4 <= 4 * 32 and arena_data(0, 1, LINK_CAP) - arena_data(0, 0, LINK_CAP) == 4 * LINK_CAP * 8 * 64


@pytest.mark.parametrize("wide", (0, 1), ids=("DistPeer", "derived"))
def test_halo_tables_every_shape(lib, wide):
    peers = shapes()
    n = 0
    for send, movers, seq, link_on in itertools.product((True, False), (False, True), SEQS, (True, False)):
        tb = halo_tab(lib, peers, 0, send, movers, seq, link_on, wide)
        check_halo_tab(tb, peers, 0, send, movers, seq, link_on)
        n += 1
    assert n == 2 * 2 * 4 * 2
    # the cases are not vacuous: with the links on, exactly the peers of 1, 3 and LINK_CAP blocks are linked
    tb = halo_tab(lib, peers, 0, True, True, 1, True, wide)
    assert tb["n"] == 5 and [int(s != 0) for s in tb["sig"][:5]] == [1, 1, 1, 0, 0]


def test_parity_follows_the_unsigned_sequence_number(lib):
    """buf / sig of a linked peer sit in the arena of parity seq & 1 for both sides, also across 2^31"""
    peers = [make_peer(0, n_blocks=3)]
    p = peers[0]
    for seq in SEQS + (2**32 - 1,):
        par = seq % 2
        s, r = halo_tab(lib, peers, 0, True, False, seq, True), halo_tab(lib, peers, 0, False, False, seq, True)
        assert s["buf"][0] - p["link_remote"] == 4 * (32 + par * LINK_CAP * 512) and s["sig"][0] - p["link_remote"] == 4 * 16 * par
        assert r["buf"][0] - p["link_local"] == 4 * (32 + par * LINK_CAP * 512) and r["sig"][0] - p["link_local"] == 4 * 16 * par
        assert s["seq"] == r["seq"] == as_int32(seq)


@pytest.mark.parametrize("wide", (0, 1), ids=("DistPeer", "derived"))
def test_halo_in_keeps_peer_positions(lib, wide):
    peers = [make_peer(0, n_blocks=0), make_peer(1, n_blocks=2), make_peer(2, n_blocks=LINK_CAP), make_peer(3, n_blocks=1, link_local=False)]
    slot = 0x7000000
    for movers, seq in itertools.product((False, True), SEQS):
        h = halo_in(lib, peers, slot, movers, seq, wide)
        assert h["slot"] == slot and h["n_peers"] == 4 and h["seq"] == as_int32(seq) and h["ch"] == (8 if movers else 4)
        for i, p in enumerate(peers):
            if i in (1, 2):   # position i, not a compacted slot: halo_slot stores (i << 24) | index
                assert h["buf"][i] == arena_data(p["link_local"], seq, LINK_CAP) and h["sig"][i] == arena_flag(p["link_local"], seq)
            else:             # no blocks / no arena of its own mapped: left null
                assert h["buf"][i] == 0 and h["sig"][i] == 0
        assert np.all(h["buf"][4:] == 0) and np.all(h["sig"][4:] == 0)


GHOSTS = ((0, 0, 0, 0), (1, 0, 0, 2), (255, 256, 1, 0), (256, 1, 1, 256), (0, 300, 257, 0), (1000, 0, 0, 0))


@pytest.mark.parametrize("wide", (0, 1), ids=("DistPeer", "derived"))
def test_ghost_tables(lib, wide):
    peers = [make_peer(i, ghosts=g) for i, g in enumerate(GHOSTS)]
    for send in (True, False):
        tb = ghost_tab(lib, peers, 0, send, wide)
        cnt = [(p["n_send_p"], p["n_send_e"]) if send else (p["n_recv_p"], p["n_recv_e"]) for p in peers]
        mine = [(p, c) for p, c in zip(peers, cnt) if sum(c)]
        check_offsets(tb, [sum(c) for _, c in mine])
        for k, (p, (n_p, n_e)) in enumerate(mine):
            assert tb["n_p"][k] == n_p and tb["n_e"][k] == n_e
            assert tb["ids_p"][k] == p["send_p" if send else "recv_p"] and tb["ids_e"][k] == p["send_e" if send else "recv_e"]
            assert tb["buf"][k] == p["ghost_send" if send else "ghost_recv"]
    # (n_send_p, n_recv_p, n_send_e, n_recv_e): peer 0 sends and receives nothing, peer 5 receives nothing
    assert ghost_tab(lib, peers, 0, True, wide)["n"] == 5 and ghost_tab(lib, peers, 0, False, wide)["n"] == 4


def test_more_peers_than_one_table_holds(lib):
    """nine peers: the tables of [0, 8) and [8, 16) together hold every non-empty peer exactly once"""
    nbs = (2, 0, 1, LINK_CAP + 1, 3, 0, 1, 4, 2)
    peers = [make_peer(i, n_blocks=nb, ghosts=(nb, 0, 0, nb)) for i, nb in enumerate(nbs)]
    seen, seen_g = [], []
    for i0 in (0, TAB):
        tb = halo_tab(lib, peers, i0, True, True, 3, True)
        check_halo_tab(tb, peers, i0, True, True, 3, True)
        seen += tb["blocks"][:tb["n"]].tolist()
        g = ghost_tab(lib, peers, i0, True)
        seen_g += g["ids_p"][:g["n"]].tolist()
    want = [p["blocks"] for p in peers if p["n_blocks"]]
    assert seen == want and len(set(seen)) == len(want) == 7
    assert seen_g == [p["send_p"] for p in peers if p["n_blocks"]]
    assert halo_tab(lib, peers, TAB, True, True, 3, True)["n"] == 1
    # ... and an empty list, or a window behind the list, is an empty table
    assert halo_tab(lib, [], 0, True, False, 0, True)["n"] == 0 and halo_tab(lib, peers, 2 * TAB, True, False, 0, True)["n"] == 0
    assert ghost_tab(lib, [], 0, True)["n"] == 0
