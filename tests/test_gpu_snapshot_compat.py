"""Snapshots taken before the two-state engine moved out of the C-ABI file still restore, and new ones carry the
same header.  tests/golden/snapshot_{two_state,general}.bin were written on an MI355X by the library as it was then:
K = 4, partial_capacity = 4, after twelve events that leave live partials on every key; snapshot_compat.json holds
the matches that library emitted for the eight events pushed after the snapshot.

Only the header and the total length of a fresh image are compared: slab rows above a key's live count are not
initialised, so the bodies may differ.
"""
import importlib
import json
import os

import numpy as np
import pytest

from test_gpu_general import GENERAL
from test_gpu_parity import SHAPES

sa = importlib.import_module("siddhi-1_amd")

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QUERY = {"two_state": SHAPES["c2_every_within"], "general": GENERAL["sequence"]}
K, CAP = 4, 4
HEADER_BYTES = 88   # SnapHeader (csrc/sg_engine.hip)


def events(seq, n):
    i = np.arange(seq, seq + n)
    key = (i % K).astype(np.uint32)
    return dict(key=key, ts=(1_000_000 + i).astype(np.int64), symbol=key.copy(),
                price=(21.0 + i).astype(np.float32), volume=(100 + i).astype(np.int32))


def engine(kind):
    app = sa.parse_app(QUERY[kind])
    cq = sa.compile_query(app, app.queries[0], sa.StringDictionary())
    return sa.NativeEngine(sa.load_hip_library(), "sg_", cq.ir, n_keys=K, max_batch=16, partial_capacity=CAP,
                           match_capacity=256)


def push(e, seq, n):
    d = events(seq, n)
    e.push(0, seq, d["ts"], [d["symbol"], d["price"], d["volume"]], None, d["key"])
    m = e.poll()
    return dict(trigger_seq=m.trigger_seq.tolist(), key=m.key.tolist(), ts=m.ts.tolist(),
                slot_seq=m.slot_seq.reshape(len(m), -1).tolist(), chain_len=m.chain_len.tolist())


def snapshot_after_a_dozen(kind):
    e = engine(kind)
    push(e, 0, 12)
    image, live = e.snapshot(), e.stats()["partials_live"]
    e.close()
    return image, live


@pytest.mark.parametrize("kind", sorted(QUERY))
def test_recorded_snapshot_restores_and_matches_follow(kind):
    with open(os.path.join(GOLDEN, f"snapshot_{kind}.bin"), "rb") as f:
        image = f.read()
    with open(os.path.join(GOLDEN, "snapshot_compat.json")) as f:
        want = json.load(f)[kind]
    e = engine(kind)
    e.restore(image)
    assert e.stats()["partials_live"] == want["partials_live"] > 0
    got = push(e, 12, 8)
    e.close()
    assert len(want["matches"]["trigger_seq"]) > 0
    assert got == want["matches"]


@pytest.mark.parametrize("kind", sorted(QUERY))
def test_fresh_snapshot_has_the_recorded_header(kind):
    with open(os.path.join(GOLDEN, f"snapshot_{kind}.bin"), "rb") as f:
        image = f.read()
    fresh, _ = snapshot_after_a_dozen(kind)
    assert fresh[:HEADER_BYTES] == image[:HEADER_BYTES]
    assert len(fresh) == len(image)
