"""plan_search_launch (duckdb-vss_amd/csrc/host_logic.h): the one function that decides a launch of the search engine.

On the CPU: every launch of a recording session is replayed through it.  The session ran the library of the commit BEFORE the
planner existed, built with profiles/r11_record_search_plans.patch (which appends the inputs and every decided value of each
launch to a file), over indexes of 3 000 and 20 000 rows at 100, 128, 768 and 1536 dims, launches of 1-5 000 queries through the
host- and device-pointer entries, limits of 10-5 000, a predicate, deleted rows, and each search option away from its default
(profiles/README.md, r11).  tests/golden/search_plans.npz holds its de-duplicated rows: the planner must decide what that
library decided, field by field.

On the GPU (-m gpu): vss_last_search_shape of real launches, word for word against the planner called for the same inputs."""
import ctypes as C
import os

import numpy as np
import pytest

import datagen
from test_host_logic import hl  # noqa: F401  (the probe library, built from the engine's own headers)

HERE = os.path.dirname(os.path.abspath(__file__))

# the cells of hl_plan_search_launch's flat arrays, in its order (tests/host_logic_probe.cpp)
CFG = ("solo_mode solo_max_queries solo_max_bytes team n_cus touch_rows touch_lists touch_max_queries force_looping crew "
       "engine_walkers M0 V G list_cap_max nodes hash_max_log2 search_waves search_walkers_cap search_wgs_per_cu search_spec_active "
       "search_pipelined search_wide_lists search_list_lds search_prescore search_prescore_descent retry_in_place visited_per_limit "
       "hash_lds_max_log2 hash_lds_max_override visited_compact_on search_crew_tune").split()
IN = "n limit bump min_hash_log2 list_cap cand_cap tomb direct_io".split()
OUT = ("solo team threads walkers grid lds_bytes regs nch hash_log2 hash_in_lds visited_compact stage_cap retry_log2 roomy list_place "
       "list_lds pipelined crew touch_lines spec_active wants_prescore prescore_descent global_hash retry_hash list_buf cand_buf "
       "shape0 shape1 shape2 shape3 shape4 shape5 shape6 shape7").split()
# the two options the recorded engine kept twice (as a member and inside its shape policy): one cell each here
ALIASES = {"search_walkers": "engine_walkers", "search_touch_lists": "touch_lists", "o_S": "o_walkers"}


def plan(hl, cfg, launch):  # noqa: F811
    c = np.array([cfg[k] for k in CFG], dtype=np.uint64)
    i = np.array([launch[k] for k in IN], dtype=np.uint64)
    o = np.zeros(len(OUT), dtype=np.uint64)
    hl.hl_plan_search_launch(c.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p))
    return dict(zip(OUT, (int(v) for v in o)))


@pytest.fixture(scope="module")
def recorded():
    z = np.load(os.path.join(HERE, "golden", "search_plans.npz"))
    names, rows = [str(s) for s in z["names"]], z["rows"]
    rows.setflags(write=False)
    return names, rows


def test_fixture_of_recorded_launches_reaches_every_branch(recorded):
    names, rows = recorded
    col = {n: rows[:, i] for i, n in enumerate(names)}
    assert set(names) == set(CFG) | set(IN) | {"o_" + k for k in OUT} | set(ALIASES), "every input and every plan field is recorded"
    for a, b in ALIASES.items():
        assert np.array_equal(col[a], col[b]), (a, b)
    assert len(np.unique(rows, axis=0)) == len(rows) > 1000
    solo, team = col["o_solo"] == 1, col["o_team"] == 1
    assert (solo & ~team).any() and team.any() and (~solo).any(), "solo, team and workgroup engine"
    assert not (team & ~solo).any()
    assert set(col["o_list_place"].tolist()) == {0, 1, 2}, "list in registers, LDS, HBM"
    assert set(col["o_shape5"].tolist()) == {0, 1, 2}, "visited set in LDS plain, LDS compact, HBM"
    assert (col["bump"] > 0).any() and (col["min_hash_log2"] > 0).any(), "retry passes"
    assert (col["o_retry_log2"] > 0).any(), "in-place retry wanted"
    assert (col["tomb"] == 1).any() and (col["tomb"] == 2).any()
    assert (col["o_threads"] == 768).any(), "a 12-wave launch"
    assert (col["direct_io"] == 1).any() and (col["direct_io"] == 0).any()
    for k in OUT:
        if k != "shape7":  # (the eighth word of vss_last_search_shape is reserved: always 0)
            assert len(np.unique(col["o_" + k])) >= 2, k
    assert not col["o_shape7"].any()


def test_planner_decides_what_the_engine_decided_before_it_existed(hl, recorded):  # noqa: F811
    names, rows = recorded
    bad = []
    for r in rows:
        rec = dict(zip(names, (int(v) for v in r)))
        got = plan(hl, rec, rec)
        diff = {k: (got[k], rec["o_" + k]) for k in OUT if got[k] != rec["o_" + k]}
        if diff:
            bad.append(({k: rec[k] for k in CFG + IN}, diff))
    assert not bad, "%d of %d recorded launches planned differently (got, recorded); first: %s" % (len(bad), len(rows), bad[0])


# ---------------------------------------------------------------------------------------------------------------------------
ROWS = 3000
DEFAULTS = dict(solo_mode=1, solo_max_queries=32, solo_max_bytes=32 * 1024, team=1, touch_rows=1, touch_lists=1, touch_max_queries=256,
                force_looping=0, crew=1, engine_walkers=0, search_waves=16, search_walkers_cap=4, search_wgs_per_cu=1,
                search_spec_active=0, search_pipelined=1, search_wide_lists=1, search_list_lds=1, search_prescore=1,
                search_prescore_descent=1, retry_in_place=1, visited_per_limit=0, hash_lds_max_log2=13, hash_lds_max_override=0,
                visited_compact_on=1, search_crew_tune=0)
# (dim, queries, limit, entry, options of the engine = cells of the config, what the launch must be)
LAUNCHES = [
    (64, 8, 64, "host", {"search.team": ("team", 0)}, "solo"),
    (64, 64, 64, "host", {}, "team"),
    (64, 1000, 64, "host", {}, "engine"),
    (768, 1, 64, "host", {}, "one walker"),
    (768, 200, 64, "device", {}, "one walker"),
    (768, 1000, 64, "host", {}, "four walkers"),
    (768, 1000, 400, "host", {}, "twelve waves"),
    (768, 300, 513, "host", {"search.list_lds": ("search_list_lds", 2)}, "list in LDS"),
    (768, 300, 5000, "host", {}, "engine"),
    (768, 300, 100, "filtered", {}, "engine"),
]


@pytest.fixture(scope="module")
def indexes():
    import gpu_common as gc
    out = {}
    for dim in (64, 768):
        g = gc.gpu_index(dim, "l2sq")
        g.reserve(ROWS)
        g.add(np.arange(ROWS), datagen.mixture(ROWS, dim, 1234 + dim))
        out[dim] = (g, datagen.mixture(1000, dim, 4321 + dim))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dim,nq,limit,entry,options,what", LAUNCHES, ids=["%d-%d-%d-%s" % c[:4] for c in LAUNCHES])
def test_launched_shape_is_the_planned_shape(hl, indexes, dim, nq, limit, entry, options, what):  # noqa: F811
    import torch
    g, Q = indexes[dim]
    V = (dim + 3) // 4
    G = 1
    while G < min(64, V):
        G *= 2
    M0 = g.M0
    cfg = dict(DEFAULTS, n_cus=torch.cuda.get_device_properties(0).multi_processor_count, M0=M0, V=V, G=G,
               list_cap_max=(max(g.M, M0) + 63) // 64 * 64, nodes=ROWS,
               hash_max_log2=max(10, int(np.ceil(np.log2((ROWS + 2) * 8 // 7 + 64)))))
    k = min(10, limit)
    launch = dict(n=nq, limit=limit, bump=0, min_hash_log2=0, list_cap=min(limit, ROWS) if limit > 512 else 0,
                  cand_cap=min(ROWS + 1, max(1024, 4 * limit)), tomb=0, direct_io=int(entry == "host" and nq <= 256))
    for name, (cell, value) in options.items():
        g.set_option(name, value)
        cfg[cell] = value
    try:
        if entry == "host":
            g.search_batch(Q[:nq], k, limit)
        elif entry == "filtered":
            launch["tomb"] = 1 if limit <= 512 else 2
            g.search_batch_filtered(Q[:nq], k, limit, np.full((ROWS + 63) // 64, 0x5555555555555555, dtype=np.uint64), ROWS)
        else:
            dQ = torch.from_numpy(Q[:nq]).cuda()
            keys = torch.empty((nq, k), dtype=torch.int64, device="cuda")
            dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
            cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
            g.search_batch_device(dQ.data_ptr(), nq, k, limit, keys.data_ptr(), dist.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
        shape = g.last_search_shape().tolist()
    finally:
        for name, (cell, _) in options.items():
            g.set_option(name, DEFAULTS[cell])
    want = plan(hl, cfg, launch)
    print(what, shape, want)
    assert shape == [want["shape%d" % i] for i in range(8)], (what, want)
    # ... and the case is the one it is meant to be
    threads, walkers, solo = shape[0], shape[1], shape[6]
    assert {"solo": solo and threads == 64, "team": solo and threads == 512, "engine": not solo,
            "one walker": not solo and walkers == 1 and threads == 1024, "four walkers": not solo and walkers == 4,
            "twelve waves": not solo and threads == 768, "list in LDS": not solo and shape[4] == 1}[what], (what, shape)
