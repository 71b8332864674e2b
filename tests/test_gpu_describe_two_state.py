"""describe() of the two-state engine (csrc/p2_host.hip), compared for exact equality with the strings the engine
printed while it still lived in the C-ABI file: either grouping, the hot-key pipeline's batch count, the projection and
the aggregators.  The strings were recorded on an MI355X, as those of test_gpu_describe_routes.py were.

The grouping follows the batch's density (fused_density_ok): 256 events on 4 keys put 16,384 events into the one
256-key tile, above what the fused split holds in registers, so that batch is sorted; 64 events on 64 keys are fused.
`every e1 -> e2` on one stream runs the hot-key pipeline on its first batch whatever the keys; the other shapes never.
"""
import importlib

import pytest
import torch

from test_gpu_parity import SHAPES
from test_gpu_projection import AGG_APPS

sa = importlib.import_module("siddhi-1_amd")
cp = importlib.import_module("siddhi-1_amd.compiler")
synth = importlib.import_module("siddhi-1_amd.synth")

pytestmark = pytest.mark.gpu

# name: (query, n_keys, events per batch, batches pushed, select list set)
CASES = {
    "sorted": (SHAPES["no_every"], 4, 256, 1, False),
    "fused": (SHAPES["no_every"], 64, 64, 1, False),
    "hot_pipeline": (SHAPES["c2_every_within"], 64, 64, 2, False),
    "projection": (SHAPES["no_every"], 64, 64, 1, True),
    "projection_aggregator": (AGG_APPS["agg_c2"], 64, 64, 1, True),
}

SORTED = ("push: k_part_hist + k_part_scan + k_part_scatter per 8-bit digit + k_part_bounds (grouping, stream 2); "
          "k_adv_m (NFA advance, LDS-staged, lane per key)")
FUSED = ("push: k_part_hist + k_part_scan + k_part_scatter x2 + k_tile_bounds (grouping by key tile, stream 2); "
         "k_adv_m (key split in LDS + NFA advance, LDS-staged, lane per key)")
HOT = " + k_hot_prep..k_hot_final (hot keys, partials in parallel, 1 batches)"
REST = (" + k_adv_m_h / k_adv_m_k (NFA advance, HBM pass: the waves left whole / the keys stopped) + k_stats_reduce; "
        "k_order_sums + scan + k_order_scatter (ordering)")

# describe() after the engine was created (and the select list set), and after the pushes: an engine that has not
# pushed yet names the sorted grouping; the pipeline ran on the first of the two batches only
EXPECTED = {
    "sorted": [SORTED + REST, SORTED + REST],
    "fused": [SORTED + REST, FUSED + REST],
    "hot_pipeline": [SORTED + REST, FUSED + HOT + REST],
    "projection": [SORTED + REST + " + k_project", FUSED + REST + " + k_project"],
    "projection_aggregator": [SORTED + REST + " + k_project + k_agg", FUSED + HOT + REST + " + k_project + k_agg"],
}


def described(name, devices=None):
    q, n_keys, n, batches, select = CASES[name]
    app, strings = sa.parse_app(q), sa.StringDictionary()
    cq = sa.compile_query(app, app.queries[0], strings)
    e = sa.NativeEngine(sa.load_hip_library(), "sg_", cq.ir, n_keys=n_keys, max_batch=n, partial_capacity=32,
                        match_capacity=1 << 12, devices=devices)
    if select:
        e.set_projection(*cp.projection_program(cq, strings))
    out = [e.describe()]
    for b in range(batches):
        d = synth.stock_ticks(b * n, n, n_keys, seed=1, rate_per_ms=3)
        e.push(0, b * n, d["ts"], [d["symbol"], d["price"], d["volume"]], None, d["key"])
        e.poll()
    out.append(e.describe())
    e.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_describe_is_the_recorded_string(name):
    got = described(name)
    print(name, got)
    assert got == EXPECTED[name]


def test_describe_of_two_shards():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    got = described("fused", devices=[0, 1])
    print(got)
    assert got == ["2 shards, each " + s for s in EXPECTED["fused"]]
