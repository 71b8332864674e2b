"""The flat stencil kernel of unpartitioned stream-state sequences (k_seq_flat_<n>_<NW>) and the select list projected
inside the stencil kernels, against the general kernel (SG_NO_SEQ=1) and the CPU oracle, bit-exact: matches on every
poll, the work counters, the state documents, the projected value words and null flags, the runtime's callback events.
One stream of one key at 3 events per ms; pushes of 700 events span three tiles and cut chains at every boundary.
"""
import importlib
import re

import numpy as np
import pytest

import test_gpu_seq_window as sw
from test_gpu_parity import _same
from test_gpu_seq_window import (RISE, SHAPES, STOCK, _compile, _counters_equal, _docs_equal, _drive, _engine, _oracle,
                                 _push, _stream)

sa = importlib.import_module("siddhi-1_amd")
cp = importlib.import_module("siddhi-1_amd.compiler")
sd = importlib.import_module("siddhi-1_amd.state_doc")

pytestmark = pytest.mark.gpu

SEED = 7   # (picked with the oracle alone: every shape below, nulls on and off, matches on this stream)


def flat(q):
    """the unpartitioned version of a query of test_gpu_seq_window"""
    return q.replace("partition with (symbol of S) begin ", "").replace(" end;", "")


def _trio(q, batch, monkeypatch, kernel="k_seq_flat_"):
    fast = _engine(q, 1, batch, False, monkeypatch)
    assert kernel in fast.describe(), fast.describe()
    gen = _engine(q, 1, batch, True, monkeypatch)
    assert "k_seq_" not in gen.describe(), gen.describe()
    return [fast, gen, _oracle(q, 1)]


@pytest.mark.parametrize("nulls", [False, True], ids=["full", "nulls"])
@pytest.mark.parametrize("shape", ["s2", "s3", "s4", "s3_short_within", "s3_two_refs", "s3_wide"])
def test_flat_equals_general_and_oracle(shape, nulls, monkeypatch):
    q = flat(SHAPES[shape])
    d, cols, nul = _stream(2100, 1, seed=SEED, nulls=nulls, wide="double" in q)
    engines = _trio(q, 1024, monkeypatch)
    assert _drive(engines, d, cols, nul, 700, docs=True) > 0
    _counters_equal(*engines)
    assert engines[0].stats()["keys_touched"] == 3 and engines[0].stats()["window_spills"] == 0


def test_flat_carry_shorter_than_the_halo(monkeypatch):
    """pushes of 1, 2 and 3 events: the window comes from the carry record and the tile in every mix; then 600 at once"""
    q = flat(SHAPES["s4"])
    d, cols, nul = _stream(720, 1, seed=SEED)
    engines = _trio(q, 1024, monkeypatch)
    cuts = [0]
    while cuts[-1] < 120:
        cuts.append(cuts[-1] + 1 + len(cuts) % 3)
    assert sum(len(_push(engines, d, cols, nul, lo, hi, docs=True)) for lo, hi in zip(cuts, cuts[1:] + [720])) > 0
    _counters_equal(*engines)


@pytest.mark.parametrize("case", ["import", "restore", "foreign"])
def test_flat_adopts_or_hands_over_a_state_that_arrives_in_the_block(case, monkeypatch):
    """500 events, then the state moved into a fresh engine: the oracle's document (adopted), a snapshot (adopted), and
    a document whose clone carries another timestamp than its partials (not the canonical form: key 0 goes to the
    general kernel for one push, window_spills counts it).  All go on as the engine that ran straight through."""
    q = flat(SHAPES["s3"])
    d, cols, nul = _stream(2100, 1, seed=SEED)
    straight, ora = _engine(q, 1, 1024, False, monkeypatch), _oracle(q, 1)
    _drive([straight, ora], d, cols, nul, 500, hi=500)
    fresh = _engine(q, 1, 1024, False, monkeypatch)
    if case == "restore":
        fresh.restore(straight.snapshot())
    else:
        doc = sd.parse(ora.state_export())
        if case == "foreign":
            clone = doc.keys[0].procs[0].newev
            assert clone, "no clone staged at the cut: the test does not test"
            doc.keys[0].states[clone[0]].ts += 1
        fresh.state_import(sd.write(doc))
    assert _drive([straight, fresh, ora], d, cols, nul, 400, lo=500, docs=True) > 0
    assert fresh.stats()["window_spills"] == (1 if case == "foreign" else 0)


def _select(q, n, having):
    return q.replace("select e1.price as a", f"select e1.price as a, e{n}.price - e1.price as d, e2.volume as v"
                     + (" having d > 1" if having else ""))


@pytest.mark.parametrize("having", [False, True], ids=["select", "having"])
@pytest.mark.parametrize("shape", ["s2", "s4", "s3_wide"])
@pytest.mark.parametrize("part", [True, False], ids=["partitioned", "flat"])
def test_select_list_projected_in_the_stencil_kernels(part, shape, having, monkeypatch):
    n, keys = {"s2": 2, "s4": 4, "s3_wide": 3}[shape], 5 if part else 1
    q = _select(SHAPES[shape] if part else flat(SHAPES[shape]), n, having)
    d, cols, nul = _stream(2100, keys, seed=SEED, nulls=True, wide="double" in q)
    app, strings = sa.parse_app(q), sa.StringDictionary()
    prog = cp.projection_program(sa.compile_query(app, app.queries[0], strings), strings)
    engines = [_engine(q, keys, 1024, general, monkeypatch) for general in (False, True)]
    for e in engines:
        e.set_projection(*prog)
    assert re.search("k_seq_batch_._._p" if part else "k_seq_flat_._._p", engines[0].describe()), engines[0].describe()
    assert "k_seq_" not in engines[1].describe()
    total = nulls = 0
    for lo in range(0, 2100, 700):
        sl = slice(lo, lo + 700)
        for e in engines:
            e.push(0, lo, d["ts"][sl], [c[sl] for c in cols], [x if x is None else x[sl] for x in nul], d["key"][sl])
        mf, mg = [e.poll() for e in engines]
        _same(mf, mg)
        assert np.array_equal(mf.proj_value, mg.proj_value) and np.array_equal(mf.proj_null, mg.proj_null)
        total, nulls = total + len(mf), nulls + int(mf.proj_null.sum())
    assert total > 0 and nulls > 0   # (a null operand gives a null item)
    _counters_equal(*engines)


@pytest.mark.parametrize("part", [True, False], ids=["partitioned", "flat"])
def test_sequence_through_the_runtime(part, monkeypatch):
    body = ("from every e1=S[price>20], e2=S[price>e1.price], e3=S[price>e2.price] "
            "select e1.price as a, e3.price - e1.price as d insert into O;")
    app = STOCK + (f"partition with (symbol of S) begin {body} end;" if part else body)
    keys = 5 if part else 1
    d = sw.synth.stock_ticks(0, 2100, keys, seed=SEED, rate_per_ms=3)
    out = {}
    for general in (False, True):
        if general:
            monkeypatch.setenv("SG_NO_SEQ", "1")
        rt = sa.SiddhiManager(n_keys=64, max_batch=1024).createSiddhiAppRuntime(app)
        monkeypatch.delenv("SG_NO_SEQ", raising=False)
        eng = rt.queries[0]
        assert eng.device_projection
        assert (("k_seq_batch_3_3_p" if part else "k_seq_flat_3_3_p") in eng.engine.describe()) != general, eng.engine.describe()
        rows = out[general] = []
        rt.addCallback("O", lambda events, rows=rows: rows.extend((e.timestamp, tuple(e.data)) for e in events))
        rt.start()
        for lo in range(0, 2100, 700):
            sl = slice(lo, lo + 700)
            rt.getInputHandler("S").send_columns(d["ts"][sl], [np.array([f"K{k}" for k in d["key"][sl]]), d["price"][sl],
                                                               d["volume"][sl]])
        rt.shutdown()
    assert len(out[False]) > 0 and out[False] == out[True]


@pytest.mark.parametrize("case", ["count", "ifThenElse", "no_every"])
def test_out_of_shape_stays_on_the_general_kernel(case, monkeypatch):
    """an aggregator and an ifThenElse item keep the projecting query on k_gen_batch (the host selector's rows are
    the reference there: the runtime compares them in test_selector); the sequence without `every` is no stencil"""
    q = flat(SHAPES["s3"] if case != "no_every" else sw.seq(RISE[:3], every=False))
    q = q.replace("e1.price as a", {"count": "count() as c", "ifThenElse": "ifThenElse(e1.price > 30, 1, 0) as a",
                                    "no_every": "e1.price as a"}[case])
    d, cols, nul = _stream(2100, 1, seed=SEED)
    e, ora = _engine(q, 1, 1024, False, monkeypatch), _oracle(q, 1)
    prog = cp.projection_program(_compile(q), sa.StringDictionary())
    if prog is not None:
        e.set_projection(*prog)
    assert "k_seq_" not in e.describe() and "k_gen_batch" in e.describe(), e.describe()
    p = d["price"]   # (without `every` the one key's only attempt starts at the first event: start where it matches)
    lo = next(i for i in range(2000) if 20 < p[i] < p[i + 1] < p[i + 2]) if case == "no_every" else 0
    assert _drive([e, ora], d, cols, nul, 700, lo=lo) > 0
    _docs_equal(e, ora)
