"""The optimiser step and the schedules without a GPU: appearance_param_groups, update_learning_rate and expon_lr against the
reference's own training_setup / update_learning_rate / get_expon_lr_func (tests/golden/optim.npz); the twin
(tests/adam_twin_torch.py) against the reference's recorded trajectory; the measurement of S32, the constants the bounds are built
on; mpmavatar_amd/csrc/adam_math.hpp compiled with g++ (tests/hostadam/hostadam.cpp: the launches and the kernel as serial loops,
table decode included) against the float64 twin; the decode over the shapes at which it can go wrong; lr == 0.  Every comparison
prints its figures before it asserts (run with -s)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import adam_cases as ac
import adam_twin_torch as tw
from mpmavatar_amd import optim

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim.npz")
SETS = (("default", ac.DEFAULT_OPT, 1.0), ("other", ac.OPT, ac.SCALE))


# ---- the schedules and the groups are the reference's --------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,args,scale", SETS, ids=[s[0] for s in SETS])
def test_param_groups_have_the_references_structure(tag, args, scale):
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < 512 * 1024
    groups = ac.groups(opt=args, scale=scale)
    assert [x["name"] for x in groups] == list(g[f"{tag}_names"]) == list(optim.GROUP_NAMES)
    assert [len(x["params"]) for x in groups] == list(g[f"{tag}_counts"])
    assert [",".join(x["params"]) for x in groups] == list(g[f"{tag}_members"])
    assert np.array_equal(np.array([x["lr"] for x in groups], np.float64), g[f"{tag}_lr_setup"])
    # what a torch.optim.Adam and a FusedAdam fill in: the reference's eps and betas
    assert (g[f"{tag}_eps"] == 1e-15).all() and (g[f"{tag}_betas"] == (0.9, 0.999)).all()
    leaves = [torch.nn.Parameter(torch.zeros(1)) for _ in range(13)]
    opt = optim.FusedAdam(optim.appearance_param_groups(*leaves[:7], leaves[7:9], leaves[9:], args, scale), lr=0.0, eps=1e-15)
    assert [x["eps"] for x in opt.param_groups] == list(g[f"{tag}_eps"])
    assert [list(x["betas"]) for x in opt.param_groups] == g[f"{tag}_betas"].tolist()


@pytest.mark.parametrize("tag,args,scale", SETS, ids=[s[0] for s in SETS])
def test_update_learning_rate_reproduces_every_recorded_rate(tag, args, scale):
    g = np.load(GOLD)
    fake = SimpleNamespace(param_groups=ac.groups(opt=args, scale=scale))
    for row, it in zip(g[f"{tag}_lr"], ac.ITERATIONS):
        set_now = optim.update_learning_rate(fake, it)
        assert set(set_now) == {"xyz", "verts"}
        for x, want in zip(fake.param_groups, row):
            got = float(x["lr"])
            print(tag, it, x["name"], "%.17g against %.17g" % (got, want))
            assert got == want if want == 0 else abs(got - want) <= 1e-15 * abs(want), (it, x["name"])
    if tag == "default":
        assert fake.param_groups[6]["lr"] == 0.0 and g["default_lr"][:, 6].max() == 0         # both zero -> 0.0: verts is switched off
    else:
        assert len(set(g["other_lr"][:, 0])) == 5                                               # xyz changes, and is held behind max_steps


def test_expon_lr_rules():
    assert optim.expon_lr(-1, 1e-2, 1e-4) == 0.0 and optim.expon_lr(5, 0.0, 0.0) == 0.0
    assert optim.expon_lr(0, 1e-2, 1e-4, max_steps=100) == pytest.approx(1e-2, rel=1e-15)
    assert optim.expon_lr(100, 1e-2, 1e-4, max_steps=100) == optim.expon_lr(1000, 1e-2, 1e-4, max_steps=100) == pytest.approx(1e-4, rel=1e-15)
    assert optim.expon_lr(50, 1e-2, 1e-4, max_steps=100) == pytest.approx(1e-3, rel=1e-14)
    # the eased-in factor: lr_delay_mult at step 0, 1 from lr_delay_steps on
    assert optim.expon_lr(0, 1e-2, 1e-2, lr_delay_steps=10, lr_delay_mult=0.01) == pytest.approx(1e-4, rel=1e-14)
    assert optim.expon_lr(10, 1e-2, 1e-2, lr_delay_steps=10, lr_delay_mult=0.01) == pytest.approx(1e-2, rel=1e-14)


def test_twin_reproduces_the_references_trajectory():
    """25 steps of the reference's own optimiser, set up and scheduled by its own methods, float64"""
    g, t = np.load(GOLD), ac.twin64(25)
    for k in sorted(t):
        err = ac.rel(t[k], g[k])
        print(k, "twin against the fixture %.3g" % err)
        assert g[k].dtype == np.float64 and err <= 1e-13, k
    assert np.array_equal(g["p__features_rest"], ac.params()["_features_rest"].astype(np.float64)) and g["m__features_rest"].any()     # lr == 0


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------

def test_s32_is_the_measurement():
    worst = {c: 0.0 for c in ac.CLASSES}
    for k_steps in ac.K_STEPS:
        e = ac.errors(ac.twin(k_steps, torch.float32), ac.twin64(k_steps))
        print("K = %d:" % k_steps, ", ".join("%s %.3g (%s)" % (c, *e[c]) for c in ac.CLASSES))
        for c in ac.CLASSES:
            worst[c] = max(worst[c], e[c][0])
    for c in ac.CLASSES:
        print("S32[%s] measured %.4g, committed %.4g" % (c, worst[c], ac.S32[c]))
        assert 0.5 * ac.S32[c] < worst[c] <= ac.S32[c]
        assert ac.BOUND[c] == 10 * ac.S32[c]


def test_cases_meet_their_conditions():
    p = ac.params()
    assert not p["_xyz"].any() and not p["verts_offset"].any() and ac.N % 4 and ac.N % 64
    assert sorted(v.size for k, v in p.items() if k.startswith("shadow")) == [1, 3, 18, 257]
    for k in (1, 2, 25):
        g = ac.grads(k)
        rows = ~g["_xyz"].any(1)
        assert 0.35 * ac.N < rows.sum() < 0.65 * ac.N
        for name in ac.GAUSS:
            flat = g[name].reshape(ac.N, -1)
            assert not flat[rows].any() and (flat[~rows] != 0).all()
        every = np.concatenate([np.abs(v[v != 0]) for v in g.values()])
        assert every.min() >= 0.99e-8 and every.max() <= 1.0 and (every.astype(np.float32) ** 2 > 1e-30).all()
        assert np.log10(every).std() > 2                                       # spread over the decades
    assert not np.array_equal(~ac.grads(1)["_xyz"].any(1), ~ac.grads(2)["_xyz"].any(1))
    assert ac.rates(1)["xyz"] != ac.rates(2)["xyz"] != ac.rates(3)["xyz"] and ac.rates(1)["verts"] != ac.rates(2)["verts"]
    assert ac.rates(1)["f_rest"] == 0.0


# ---- adam_math.hpp on the host ---------------------------------------------------------------------------------------------------------

def test_host_constants_are_the_headers():
    lib = ac.host_lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpmhip.h")).read()
    assert f"#define MPMHIP_ADAM_CHUNK {lib.ha_chunk()}\n" in header and f"#define MPMHIP_ADAM_MAX_TENSORS {lib.ha_max_tensors()}\n" in header
    assert (optim.ADAM_CHUNK, optim.MAX_TENSORS) == (lib.ha_chunk(), lib.ha_max_tensors())
    assert lib.ha_table_bytes() + 512 <= 4096                               # the table is a kernel argument


@pytest.mark.parametrize("k_steps", ac.K_STEPS)
def test_host_against_float64(k_steps):
    e = ac.errors(ac.host_run(k_steps), ac.twin64(k_steps))
    for c in ac.CLASSES:
        print("K = %d %s: %.3g (%s) of bound %.3g" % (k_steps, c, *e[c], ac.BOUND[c]))
        assert e[c][0] <= ac.BOUND[c], c


@pytest.mark.parametrize("name", list(ac.shape_lists(4096, 48)))
def test_host_decode_visits_every_element_exactly_once(name):
    lib = ac.host_lib()
    counts, offsets = ac.shape_lists(lib.ha_chunk(), lib.ha_max_tensors())[name]
    rng = np.random.default_rng(5)
    rows = ac.rows(counts, rng, offsets)
    want = [ac.expected(r) for r in rows]
    visits = [np.zeros(max(n, 1), np.int32) for n in counts]
    launches = ac.host_step(rows, visits)
    assert launches == -(-sum(n > 0 for n in counts) // lib.ha_max_tensors())
    for r, w, vis, n in zip(rows, want, visits, counts):
        assert (vis[:n] == 1).all(), (name, n, np.flatnonzero(vis[:n] != 1)[:5])
        for got, w64, c in zip((r[0], r[2], r[3]), w, ac.CLASSES):
            assert ac.rel(got, w64) <= ac.BOUND[c], (name, n, c)


def test_host_strides_over_more_chunks_than_the_grid():
    """one tensor of more chunks than GRID_CAP workgroups, not a multiple of the chunk: the stride takes every chunk once"""
    lib = ac.host_lib()
    n = (lib.ha_grid_cap() + 37) * lib.ha_chunk() + 2
    rng = np.random.default_rng(6)
    rows = ac.rows([n, 5], rng)
    visits = [np.zeros(n, np.int32), np.zeros(5, np.int32)]
    assert ac.host_step(rows, visits) == 1
    assert (visits[0] == 1).all() and (visits[1] == 1).all()


def test_host_lr_zero_leaves_the_parameters_bits_alone():
    rng = np.random.default_rng(7)
    rows = ac.rows([5000, 3], rng, update=[False, True])
    p0 = rows[0][0].copy()
    p0.view(np.uint32)[::7] = 0x7FC00001                                       # NaN payloads: any read-modify-write would lose them
    rows[0][0][:] = p0
    before = [a.copy() for r in rows for a in r[:4]]
    ac.host_step(rows)
    assert np.array_equal(rows[0][0].view(np.uint32), p0.view(np.uint32))
    assert not np.array_equal(rows[0][2], before[2]) and not np.array_equal(rows[0][3], before[3])
    assert (rows[1][0] != before[4]).all()                                     # the other tensor of the same launch does move
    # and through the twin's case: f_rest of the base case has lr == 0
    got = ac.host_run(2)
    assert np.array_equal(got["p__features_rest"], ac.params()["_features_rest"]) and got["m__features_rest"].any()
