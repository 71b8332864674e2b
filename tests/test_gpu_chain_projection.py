"""The select list of a chained pattern evaluated by the chain kernels (csrc/chn_kernels.hip k_chn_*_p): bit
for bit against the general kernel with the same select list (SG_NO_CHN=1) and against numpy at the per-slot event seqs
of each poll, for every place a match's event can be (payload, pool entry, batch columns, either side of a hand-over)."""
import importlib
import re

import numpy as np
import pytest

from test_gpu_chain_window import ALL, SHAPES, _chunks, _docs_equal, _engine, _oracle, _stream, chain
from test_gpu_parity import _same

sa = importlib.import_module("siddhi-1_amd")
cp = importlib.import_module("siddhi-1_amd.compiler")
pytestmark = pytest.mark.gpu

PILE = chain(["price>10", "price>39.5", "price>e2.price"], within="within 300 milliseconds")   # (outgrows the windows)
PILE_AT = {"cap": 64, "keys": 16, "rate": 2, "size": 1000}
BATCH_P = "push: k_chn_batch_2_1_p (chained states, register window, lane per key, select list projected) + "
WIDE_P = "k_chn_wide_2_1_p (the keys handed over, wide window, select list projected) + "
SELECTS = {"attrs": "e1.price as a, e2.volume as v, e{n}.price as c", "arith": "e1.price + e2.price as s, e{n}.volume as v",
           "having": "e1.price as a, e{n}.price - e1.price as d having d > 1"}
# name: (query, select list, nulls, environment, push size and engine parameters / what happens before the pushes)
CASES = {
    "p3_attrs": (SHAPES["p3"], "attrs", False, {}, {}),
    "p3_one_push": (SHAPES["p3"], "arith", True, {}, {"size": 4000}),                 # (whole matches in the payload)
    "p3_having": (SHAPES["p3"], "having", True, {}, {}),
    "p3_no_every": (SHAPES["p3_no_every"], "attrs", False, {}, {}),
    "p3_two_words_nulls": (SHAPES["p3_two_words"], "attrs", True, {}, {}),            # (kept words != projected words)
    "p3_wide": (SHAPES["p3_wide"], "arith", False, {}, {}),                           # (double: two-word values)
    "p4_nulls": (SHAPES["p4"], "arith", True, {}, {}),
    "p2": (SHAPES["p2"], "attrs", True, {"SG_FORCE_GENERAL": "1"}, {}),
    "p3_single_events": (SHAPES["p3"], "arith", True, {}, {"size": 1, "n": 1200}),    # (every captured event a pool entry)
    "p3_single_events_sorted": (SHAPES["p3"], "attrs", True, {"SG_NO_FUSED": "1"}, {"size": 1, "n": 1200}),
    "p3_import": (SHAPES["p3"], "arith", True, {}, {"size": 500, "imported": True}),  # (a block that is not canonical)
    "p3_wide_import": (SHAPES["p3_wide"], "attrs", True, {}, {"size": 500, "imported": True}),   # (and no payload: 5 words)
    "pile_wide": (PILE, "arith", False, {}, dict(PILE_AT, route=BATCH_P + WIDE_P + "k_gen_batch (keys handed over)")),
    "pile_general": (PILE, "attrs", False, {"SG_NO_CHN_WIDE": "1"}, dict(PILE_AT, route=BATCH_P + "k_gen_batch (keys handed over)")),
}


def _reference(sel, n, cols, nul, ix):
    """"attrs" and "arith" from the input columns at ix[s], the positions of state s + 1's events, in the columns' own
    types (float32 + float32 is a float32 sum, as Java's), with their null flags (a = 1 price, 2 volume)"""
    null = lambda a, s: nul[a][ix[s]] != 0 if nul else np.zeros(len(ix[s]), bool)
    if sel == "attrs":
        return [(cols[1][ix[0]], null(1, 0)), (cols[2][ix[1]], null(2, 1)), (cols[1][ix[n - 1]], null(1, n - 1))]
    return [(cols[1][ix[0]] + cols[1][ix[1]], null(1, 0) | null(1, 1)), (cols[2][ix[n - 1]], null(2, n - 1))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_select_list_projected_in_the_chain_kernels(name, monkeypatch):
    q, sel, nulls, env, o = CASES[name]
    n, keys, total_n, lo0 = q.count("=S["), o.get("keys", 40), o.get("n", 4000), o.get("n", 4000) if o.get("imported") else 0
    q = q.replace("select e1.price as a", "select " + SELECTS[sel].format(n=n))
    d, cols, nul = _stream(lo0 + total_n, keys, seed=7, nulls=nulls, wide="double" in q, rate=o.get("rate", 3))
    cut = lambda lo, hi: (lo, d["ts"][lo:hi], [c[lo:hi] for c in cols], nul and [x if x is None else x[lo:hi] for x in nul],
                          d["key"][lo:hi])
    [monkeypatch.setenv(k, v) for k, v in env.items()]
    app, strings = sa.parse_app(q), sa.StringDictionary()
    prog = cp.projection_program(sa.compile_query(app, app.queries[0], strings), strings)
    fast, gen = [_engine(q, keys, 4096, general, monkeypatch, cap=o.get("cap", 32)) for general in (False, True)]
    if lo0:   # (an oracle document: pool entries in the oracle's order, read back through the checked path)
        ora = _oracle(q, keys)
        for lo, hi in _chunks(lo0, 600):
            ora.push(0, *cut(lo, hi))
    for e in (fast, gen):
        e.set_projection(*prog)
        if lo0:
            e.state_import(ora.state_export())
    assert re.search("k_chn_batch_._._p", fast.describe()) and fast.describe() == o.get("route", fast.describe()), fast.describe()
    assert "k_chn_" not in gen.describe() and "k_gen_batch" in gen.describe()
    total = 0
    for lo, hi in _chunks(total_n, o.get("size", 900)):
        for e in (fast, gen):
            e.push(0, *cut(lo0 + lo, lo0 + hi))
        mf, mg = fast.poll(), gen.poll()
        _same(mf, mg)
        assert np.array_equal(mf.proj_value, mg.proj_value) and np.array_equal(mf.proj_null, mg.proj_null)
        ix = [mf.slot_seq[:, s, 0].astype(np.int64) for s in range(n)]
        for i, (want, isnull) in enumerate(_reference(sel, n, cols, nul, ix) if sel != "having" and len(mf) else []):
            bits = want.view(np.uint32 if want.dtype.itemsize == 4 else np.uint64).astype(np.uint64)
            assert np.array_equal(mf.proj_null[i] != 0, isnull), (name, i)
            assert np.array_equal(mf.proj_value[i][~isnull], bits[~isnull]), (name, i)
        total += len(mf)
    sf, sg = fast.stats(), gen.stats()
    assert total > 0 and all(sf[k] == sg[k] for k in ALL), (total, sf, sg)
    assert sf["window_spills"] > 0 or "route" not in o, "no key outgrew the window: the case does not test"
    _docs_equal(fast, gen)


README3 = ("define stream S (symbol string, price float, volume int); partition with (symbol of S) begin "
           "from every e1=S[price>20] -> e2=S[price>e1.price] -> e3=S[price>e2.price] within 10 sec "
           "select {} insert into O; end;")


@pytest.mark.parametrize("select,kernel", [("e1.symbol, e1.price as p1, e2.price as p2, e3.price as p3", "k_chn_batch_2_1_p"),
                                           ("e1.price as p1, count() as c", "push: k_gen_batch (general"),
                                           ("ifThenElse(e1.price > 30, e2.price, e3.price) as p", "push: k_gen_batch (general")])
def test_chain_select_list_through_the_runtime(select, kernel, monkeypatch):
    """the README's example with a third state; count() / ifThenElse stay on k_gen_batch; rows == the host selector's"""
    d, out = _stream(3000, 40, seed=9)[0], []
    for host in (False, True):
        if host:
            monkeypatch.setattr(cp, "projection_program", lambda *a: None)
        rt = sa.SiddhiManager(n_keys=64, max_batch=1024).createSiddhiAppRuntime(README3.format(select))
        desc = rt.queries[0].engine.describe()
        assert rt.queries[0].device_projection != host and ("k_chn_batch_2_1 (" if host else kernel) in desc, desc
        rows = []
        rt.addCallback("O", lambda events, rows=rows: rows.extend((e.timestamp, tuple(e.data)) for e in events))
        rt.start()
        for lo, hi in _chunks(3000, 1000):
            rt.getInputHandler("S").send_columns(d["ts"][lo:hi], [np.array([f"K{k}" for k in d["key"][lo:hi]]),
                                                                  d["price"][lo:hi], d["volume"][lo:hi]])
        rt.shutdown()
        out.append(rows)
    assert len(out[0]) > 0 and out[0] == out[1]
