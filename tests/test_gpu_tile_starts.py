"""The fused grouping's two-pass branch (part_kernels.hip sgd_group_tiles_fused, more than 256 key tiles): the
second pass's scatter computes the tile starts itself and reads the high tile digit pass 1 wrote as one byte.

A tile start is the end of the events before one of pass 1's digit boundaries, counted inside the chunk of pass 2 the
boundary falls into, so the cases are about where those boundaries fall: all of them in one or two chunks (sparse
batches), on a chunk's first or last event, on top of each other (a low digit without events), past the last event
(the last low digits empty), with a tile count that is no multiple of pass 1's digit count, with events dropped
before pass 2 (null and out-of-range ids), and the general engine's caller (64-key tiles, C3).  Every case is
compared with the CPU oracle and with the sorted grouping (SG_NO_FUSED), bit-exact, over three batches with state
carried across them, and asserts that describe() names the fused grouping."""
import importlib

import numpy as np
import pytest
import torch

import test_gpu_count_window as nw
from test_gpu_grouping import COLS, STATS, _engine_env
from test_gpu_parity import SHAPES, _engines, _same

sa = importlib.import_module("siddhi-1_amd")
synth = importlib.import_module("siddhi-1_amd.synth")

pytestmark = pytest.mark.gpu

CHUNK = 512 * 4          # events of one scatter chunk (SGD_PT_THREADS x 4, elements of 12 B)
TILE = 256               # keys of one tile of the two-state engine
K20 = 1 << 20            # 4096 tiles: two 6-bit passes
K17 = 1 << 17            # 512 tiles: a 4-bit and a 5-bit pass


def fused_route_ok(n, K, stride_words=3):
    """sgd_fused_ok and fused_density_ok (p2_host.hip) for a payload of one word, and the two-pass branch"""
    mean = n * 256.0 / K
    dense_ok = mean + 3.0 * np.sqrt(mean) <= (80 // (stride_words + 1)) * 256
    return 1 <= K <= 4096 * TILE and n <= 1 << 24 and dense_ok and (K + TILE - 1) // TILE > 256


def _pool(rng, tiles, per_tile=3):
    """a few keys in each of the given tiles (each key then gets several events of a batch)"""
    tiles = np.asarray(tiles, dtype=np.int64)
    return (np.repeat(tiles, per_tile) * TILE + rng.integers(0, TILE, len(tiles) * per_tile)).astype(np.uint32)


def _cases():
    rng = np.random.default_rng(20)
    c = {}
    # almost every tile empty; the 64 boundaries of pass 1 fall into one or two chunks of pass 2
    c["sparse"] = (K20, 3000, _pool(rng, rng.choice(4096, 150, replace=False)))
    c["sparse_three_chunks"] = (K20, 2 * CHUNK + 905, _pool(rng, rng.choice(4096, 400, replace=False)))
    # 257 tiles: b1 = 4, b2 = 5, 17 high digits, the last one holds one tile
    K = 65536 + 256
    c["tiles_257"] = (K, 4096, np.concatenate([_pool(rng, rng.choice(256, 100, replace=False)),
                                                 np.array([65536, K - 1], dtype=np.uint32)]))
    # 4096 tiles, the last one holds one key
    K = K20 - 256 + 1
    c["partial_last_tile"] = (K, 3000, np.concatenate([_pool(rng, rng.choice(4095, 150, replace=False)),
                                                       np.array([K - 1], dtype=np.uint32)]))
    c["first_tile_only"] = (K20, 700, np.arange(0, 256, 5, dtype=np.uint32))
    c["last_tile_only"] = (K20, 700, np.arange(K20 - 256, K20, 5, dtype=np.uint32))
    # low digit 5 never occurs (two equal boundaries), low digits 60..63 never occur (boundaries at the valid count)
    t = np.arange(4096)
    t = t[((t & 63) != 5) & ((t & 63) < 60)]
    c["empty_low_digits"] = (K20, 5000, _pool(rng, rng.choice(t, 300, replace=False)))
    for name, n in (("one_chunk", CHUNK), ("one_chunk_plus_one", CHUNK + 1), ("one_chunk_minus_one", CHUNK - 1),
                    ("two_chunks", 2 * CHUNK)):
        c[name] = (K17, n, _pool(rng, np.arange(512), 2))
    return c


CASES = _cases()


def test_every_case_qualifies_for_the_two_pass_fused_route():
    for name, (K, n, pool) in CASES.items():
        assert fused_route_ok(n, K), name
        assert pool.max() < K, name
    assert fused_route_ok(6000, K17)


@pytest.mark.parametrize("name", sorted(CASES))
def test_tile_starts_vs_sorted_vs_oracle(name):
    K, n, pool = CASES[name]
    q = SHAPES["c2_every_within"]
    cq, gpu, ora = _engines(q, K, n)
    srt = _engine_env(q, K, n, {"SG_NO_FUSED": "1"})
    rng = np.random.default_rng(len(name) + n)
    seq, total = 0, 0
    for b in range(3):
        d = synth.stock_ticks(seq, n, K, seed=700 + b, rate_per_ms=64)
        d["key"] = pool[rng.integers(0, len(pool), n)]
        d["symbol"] = d["key"].copy()
        for e in (gpu, ora, srt):
            e.push(0, seq, d["ts"], [d[c] for c in COLS], None, d["key"])
        mg, mo, ms = gpu.poll(), ora.poll(), srt.poll()
        _same(mg, mo)
        _same(mg, ms)
        total += len(mg)
        seq += n
    assert total > 0
    assert "grouping by key tile" in gpu.describe(), gpu.describe()
    assert "grouping by key tile" not in srt.describe()
    sg, so, ss = gpu.stats(), ora.stats(), srt.stats()
    for f in ("partials_live", "matches"):
        assert sg[f] == so[f], f
    for f in STATS:
        assert sg.get(f) == ss.get(f), f
    for e in (gpu, ora, srt):
        e.close()


def test_tile_starts_with_dropped_keys():
    """device batches with SG_KEY_NULL ids (dropped, SG_CFG_NULL_KEYS) and one id == n_keys (reported at the next
    poll, the other events processed): pass 2 runs on the valid count pass 1 left on the device, and the boundaries
    are positions among the valid events"""
    dev = torch.device("cuda", 0)
    K, n = K17, 6000
    flags = sa.native.SG_CFG_NULL_KEYS
    q = SHAPES["c2_every_within"]
    gpu = _engine_env(q, K, n, {}, flags)
    ref = _engine_env(q, K, n, {"SG_NO_FUSED": "1"}, flags)
    rng = np.random.default_rng(12)
    pool = _pool(rng, np.arange(512), 1)
    seq, total = 0, 0
    for b in range(3):
        d = synth.stock_ticks(seq, n, K, seed=800 + b, rate_per_ms=64)
        d["key"] = pool[rng.integers(0, len(pool), n)]
        d["key"][rng.random(n) < 0.2] = sa.native.SG_KEY_NULL
        if b == 1:
            d["key"][123] = K
            d["key"][n - 1] = K + 5
        d["symbol"] = d["key"].copy()
        t = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).to(dev) for k, v in d.items()}
        torch.cuda.synchronize()
        res = []
        for e in (gpu, ref):
            e.push(0, seq, (n, t["ts"].data_ptr(), [t["symbol"].data_ptr(), t["price"].data_ptr(),
                                                    t["volume"].data_ptr()], t["key"].data_ptr()),
                   [0, 1, 2], mem=sa.native.SG_MEM_DEVICE)
            e.synchronize()
            if b == 1:
                with pytest.raises(sa.EngineError, match="n_keys"):
                    e.poll()
                res.append(None)
            else:
                res.append(e.poll())
        if b != 1:
            _same(res[0], res[1])
            total += len(res[0])
        seq += n
    assert total > 0
    assert "grouping by key tile" in gpu.describe(), gpu.describe()
    sg, sr = gpu.stats(), ref.stats()
    for f in STATS:
        assert sg.get(f) == sr.get(f), f
    gpu.close()
    ref.close()


def test_tile_starts_general_engine_caller(monkeypatch):
    """C3 on 20,000 keys: the count kernel's grouping by 64-key tile takes the two-pass branch (313 tiles, the last
    one partial: a 4-bit and a 5-bit pass)"""
    q = nw.SHAPES["c3_min1"]
    K, n = 20000, 3 * CHUNK + 77
    fused = nw._engine(q, K, n, False, monkeypatch)
    srt = nw._engine(q, K, n, True, monkeypatch, env="SG_NO_FUSED")
    ora = nw._oracle(q, K)
    rng = np.random.default_rng(19)
    pool = np.concatenate([rng.choice(K, 400, replace=False), [0, K - 1]]).astype(np.uint32)
    total = 0
    for b in range(3):
        d = synth.stock_ticks(b * n, n, K, seed=60 + b, rate_per_ms=256)
        d["key"] = pool[rng.integers(0, len(pool), n)]
        d["symbol"] = d["key"].copy()
        for e in (fused, srt, ora):
            e.push(0, b * n, d["ts"], [d["symbol"], d["price"], d["volume"]], None, d["key"])
        ms = [e.poll() for e in (fused, srt, ora)]
        _same(ms[0], ms[1])
        _same(ms[0], ms[2])
        total += len(ms[0])
    assert total > 0
    sf, ss, so = fused.stats(), srt.stats(), ora.stats()
    for k in nw.ALL:
        assert sf[k] == ss[k], (k, sf[k], ss[k])
    for k in ("matches", "partials_live"):
        assert sf[k] == so[k], (k, sf[k], so[k])
    assert "k_cnt_split" in fused.describe(), fused.describe()
    assert "k_cnt_split" not in srt.describe()
    nw._docs_equal(fused, ora)
    for e in (fused, srt, ora):
        e.close()
