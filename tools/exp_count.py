"""C3_min1 (the counting sequence) at bench size through the engine: 2^20 keys, 2^22-event batches resident in HBM, steady
state (the first pushes fill the 10-second `within` window — 2.1 s of stream time each — and are not timed), step time
per push and events/s with the spread over the timed pushes, the count kernel's hand-overs (window_spills) and the work
counters.  SG_NO_CNT=1 runs the same query on the general kernel; rocprofv3 wraps this script for kernel traces.

    python tools/exp_count.py [steps] [warmup] [--projection] [--tail] [--lib PATH]

--projection  the query's select list set on the device (sg_set_projection), as the runtime does: k_cnt_batch_*_p
--tail        the single-tail form `every e1=S[f0]<1:5>, e2=S[price > e1[last].price] within 10 sec` (no `or e3=...`)
--lib PATH    another build of the engine library (a checkout of the parent commit: the baseline of a comparison)
Only the public engine API is used, so the same script drives either library.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("steps", nargs="?", type=int, default=10)
    ap.add_argument("warmup", nargs="?", type=int, default=5)
    ap.add_argument("--projection", action="store_true")
    ap.add_argument("--tail", action="store_true")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    import torch
    sa = importlib.import_module("siddhi-1_amd")
    synth = importlib.import_module("siddhi-1_amd.synth")
    cp = importlib.import_module("siddhi-1_amd.compiler")
    K, B = 1 << 20, 1 << 22
    q = synth.C3_MIN1_QUERY
    if args.tail:
        q = q.replace(" or e3=StockStream[volume > 1000]", "").replace(", e3.volume as v3", "")
        assert "e3" not in q
    app, strings = sa.parse_app(q), sa.StringDictionary()
    cq = sa.compile_query(app, app.queries[0], strings)
    dev = torch.device("cuda", 0)
    bats = [synth.stock_ticks_torch(torch, s * B, B, K, dev) for s in range(args.warmup + args.steps)]
    torch.cuda.synchronize()
    lib = sa.native.load_library(args.lib) if args.lib else sa.load_hip_library()
    eng = sa.NativeEngine(lib, "sg_", cq.ir, n_keys=K, max_batch=B, partial_capacity=32, match_capacity=2 * B, device=0)
    if args.projection:
        eng.set_projection(*cp.projection_program(cq, strings))
    times = []
    for s, t in enumerate(bats):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.push(0, s * B, (B, t["ts"].data_ptr(), [t["symbol"].data_ptr(), t["price"].data_ptr(), t["volume"].data_ptr()],
                            t["key"].data_ptr()), [0, 1, 2], mem=sa.native.SG_MEM_DEVICE)
        m = eng.poll_device()
        eng.release(m)
        eng.synchronize()
        if s >= args.warmup:
            times.append(time.perf_counter() - t0)
    print(eng.describe(), flush=True)
    med = statistics.median(times)
    what = ("single tail" if args.tail else "C3_min1") + (", select list on the device" if args.projection else ", no projection")
    print(f"{what} ({args.lib or 'this build'}): {med * 1e3:.3f} ms per step (median of {len(times)}; "
          f"min {min(times) * 1e3:.3f}, max {max(times) * 1e3:.3f}), {B / med:.3e} events/s; stats {eng.stats()}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
