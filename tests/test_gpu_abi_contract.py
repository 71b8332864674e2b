"""The C-ABI's error contract: call sequence -> (return code, exact sg_last_error text), on the two-state engine and on
the general engine, at K = 4 with batches of 8 events.  The expected values were recorded on an MI355X from the
library as it was before the two-state engine moved out of the C-ABI file (csrc/p2_host.hip); every path must keep
its code and its text.
"""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from test_gpu_general import GENERAL
from test_gpu_parity import SHAPES

sa = importlib.import_module("siddhi-1_amd")
cp = importlib.import_module("siddhi-1_amd.compiler")
native = importlib.import_module("siddhi-1_amd.native")

pytestmark = pytest.mark.gpu

K, N = 4, 8
QUERY = {"two_state": SHAPES["c2_every_within"], "general": GENERAL["sequence"]}
OK = (0, "")


def batch(seq, bad_key=False):
    """8 events, two per key, prices rising: every key's second event completes a match"""
    key = np.arange(N, dtype=np.uint32) % K
    if bad_key:
        key[5] = K
    i = np.arange(seq, seq + N)
    return dict(key=key, ts=(1_000_000 + i).astype(np.int64), symbol=key.copy(),
                price=(21.0 + i).astype(np.float32), volume=(100 + i).astype(np.int32))


class Engine:
    """one engine and the (code, text) of each call: (0, "") or the EngineError's pair"""

    def __init__(self, kind, n_keys=K, force_general=False, monkeypatch=None):
        app, self.strings = sa.parse_app(QUERY[kind]), sa.StringDictionary()
        self.cq = sa.compile_query(app, app.queries[0], self.strings)
        if force_general:
            monkeypatch.setenv("SG_FORCE_GENERAL", "1")
        self.e = sa.NativeEngine(sa.load_hip_library(), "sg_", self.cq.ir, n_keys=n_keys, max_batch=N,
                                 partial_capacity=4, match_capacity=64)
        if force_general:
            monkeypatch.delenv("SG_FORCE_GENERAL")
        self.value = None

    def call(self, f, *a):
        try:
            self.value = f(*a)
            return OK
        except sa.EngineError as ex:
            return (ex.code, str(ex).split(": ", 1)[1])

    def push(self, seq, n=N, bad_key=False):
        d = batch(seq, bad_key)
        if n != N:
            d = {k: np.resize(v, n) for k, v in d.items()}
        return self.call(self.e.push, 0, seq, d["ts"], [d["symbol"], d["price"], d["volume"]], None, d["key"])

    def hold(self):
        return self.call(self.e.poll_device)

    def set_projection(self):
        return self.call(self.e.set_projection, *cp.projection_program(self.cq, self.strings))

    def get_projection(self):
        pr = native.sg_projection()
        g = self.e.lib.sg_get_projection
        g.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(native.sg_projection)]
        return self.call(lambda: self.e._check(g(self.e.h, native.SG_MEM_HOST, C.byref(pr))))

    def reset_device_ids(self, ids):
        t = torch.tensor(ids, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        f = self.e.lib.sg_reset_keys
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        return self.call(lambda: self.e._check(f(self.e.h, C.c_void_p(t.data_ptr()), len(ids), native.SG_MEM_DEVICE)))


def push_while_held(x, mp):
    assert x.push(0) == OK and x.hold() == OK
    return [x.push(N)]


def second_poll_without_release(x, mp):
    assert x.push(0) == OK and x.hold() == OK
    return [x.hold()]


def set_projection_after_push(x, mp):
    assert x.push(0) == OK
    return [x.set_projection()]


def set_projection_twice(x, mp):
    assert x.set_projection() == OK
    return [x.set_projection()]


def get_projection_before_poll(x, mp):
    assert x.set_projection() == OK and x.push(0) == OK
    return [x.get_projection()]


def get_projection_without_projection(x, mp):
    assert x.push(0) == OK and x.hold() == OK
    return [x.get_projection()]


def seq_base_not_increasing(x, mp):
    assert x.push(0) == OK and x.call(x.e.poll) == OK
    return [x.push(0)]


def batch_above_max_batch(x, mp):
    return [x.push(0, n=N + 1)]


def host_key_out_of_range_then_corrected(x, mp):
    """the rejected batch leaves the engine as it was: the corrected one goes in at the same seq_base"""
    out = [x.push(0, bad_key=True), x.push(0), x.call(x.e.poll)]
    return out + [len(x.value)]


def snapshot_and_export_with_matches_held(x, mp):
    assert x.push(0) == OK and x.hold() == OK
    return [x.call(x.e.snapshot), x.call(x.e.state_export)]


def snapshot_and_export_with_matches_pending(x, mp):
    assert x.push(0) == OK
    return [x.call(x.e.snapshot), x.call(x.e.state_export)]


def restore_truncated(x, mp):
    assert x.call(x.e.snapshot) == OK
    return [x.call(x.e.restore, x.value[:-8]), x.call(x.e.restore, x.value[:16])]


def restore_other_kind(x, mp):
    """the same query (the same IR hash) on the other engine kind"""
    other = Engine("two_state", force_general=x.kind == "two_state", monkeypatch=mp)
    assert other.call(other.e.snapshot) == OK
    if x.kind == "general":
        x.e.close()
        x = Engine("two_state", force_general=True, monkeypatch=mp)
    return [x.call(x.e.restore, other.value)]


def restore_other_n_keys(x, mp):
    other = Engine(x.kind, n_keys=2 * K)
    assert other.call(other.e.snapshot) == OK
    return [x.call(x.e.restore, other.value)]


def reset_keys_out_of_range(x, mp):
    return [x.call(x.e.reset_keys, [1, K]), x.reset_device_ids([1, K]), x.call(x.e.reset_keys, [1]),
            x.reset_device_ids([2])]


CASES = [push_while_held, second_poll_without_release, set_projection_after_push, set_projection_twice,
         get_projection_before_poll, get_projection_without_projection, seq_base_not_increasing,
         batch_above_max_batch, host_key_out_of_range_then_corrected, snapshot_and_export_with_matches_held,
         snapshot_and_export_with_matches_pending, restore_truncated, restore_other_kind, restore_other_n_keys,
         reset_keys_out_of_range]


def observed(case, kind, monkeypatch):
    x = Engine(kind)
    x.kind = kind
    return [list(r) if isinstance(r, tuple) else r for r in case(x, monkeypatch)]


KEY_RANGE = [-1, "key id outside [0, n_keys)"]
# case: what each call after the set-up returned, per engine kind (one entry where both kinds agree)
EXPECTED = {
    "push_while_held": [[-5, "release the polled matches before pushing"]],
    "second_poll_without_release": [[-5, "previous matches not released"]],
    "set_projection_after_push": [[-5, "set the projection before the first push"]],
    "set_projection_twice": [[-5, "the projection is already set"]],
    "get_projection_before_poll": [[-5, "poll the matches first"]],
    "get_projection_without_projection": [[-5, "no projection set"]],
    # (the general engine does not look at seq_base)
    "seq_base_not_increasing": {"general": [[0, ""]], "two_state": [[-1, "sequence numbers must increase"]]},
    "batch_above_max_batch": [[-1, "batch larger than max_batch"]],
    "host_key_out_of_range_then_corrected": [KEY_RANGE, [0, ""], [0, ""], 4],
    "snapshot_and_export_with_matches_held": {
        "general": [[-5, "release the polled matches before a snapshot"]] * 2,
        "two_state": [[-5, "release the polled matches before a snapshot"],
                      [-5, "release the polled matches before exporting the state"]],
    },
    "snapshot_and_export_with_matches_pending": {
        "general": [[-5, "poll the emitted matches before a snapshot"]] * 2,
        "two_state": [[-5, "poll the emitted matches before a snapshot"],
                      [-5, "poll the emitted matches before exporting the state"]],
    },
    "restore_truncated": [[-1, "snapshot length does not match its header"], [-1, "snapshot too short"]],
    "restore_other_kind": [[-1, "snapshot of a different engine kind"]],
    "restore_other_n_keys": {
        "general": [[-1, "snapshot taken with a different n_keys / partial_capacity"]],
        "two_state": [[-1, "snapshot taken with a different n_keys"]],
    },
    "reset_keys_out_of_range": [KEY_RANGE, KEY_RANGE, [0, ""], [0, ""]],
}


@pytest.mark.parametrize("kind", sorted(QUERY))
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_call_sequence_gives_the_recorded_code_and_text(case, kind, monkeypatch):
    got = observed(case, kind, monkeypatch)
    print(case.__name__, kind, got)
    want = EXPECTED[case.__name__]
    assert got == (want[kind] if isinstance(want, dict) else want)
