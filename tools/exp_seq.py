"""The P3 workload as a SEQUENCE (`->` replaced by `,`) at bench size through the engine: 2^20 keys, 2^22-event
batches resident in HBM, steady state (the first pushes fill the `within` window and are not timed), step time per
push and events/s with the spread over the timed pushes.  SG_NO_SEQ=1 runs the same query on the general kernel;
rocprofv3 wraps this script for kernel traces.

    python tools/exp_seq.py [steps] [warmup] [--flat] [--projection] [--batch-log2 N] [--keys-log2 N] [--lib PATH]

--flat        the unpartitioned query (one key, the flat stencil kernel k_seq_flat_*)
--projection  the query's select list set on the device (sg_set_projection), as the runtime does
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
    ap.add_argument("warmup", nargs="?", type=int, default=3)
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--projection", action="store_true")
    ap.add_argument("--batch-log2", type=int, default=22)
    ap.add_argument("--keys-log2", type=int, default=20)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    import torch
    sa = importlib.import_module("siddhi-1_amd")
    synth = importlib.import_module("siddhi-1_amd.synth")
    cp = importlib.import_module("siddhi-1_amd.compiler")
    K, B = 1 if args.flat else 1 << args.keys_log2, 1 << args.batch_log2
    text = synth.P3_QUERY.replace(" -> ", ", ")
    if args.flat:
        text = text.replace("partition with (symbol of StockStream)\nbegin", "").replace("end;", "")
    app, strings = sa.parse_app(text), sa.StringDictionary()
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
                            None if args.flat else t["key"].data_ptr()), [0, 1, 2], mem=sa.native.SG_MEM_DEVICE)
        m = eng.poll_device()
        eng.release(m)
        eng.synchronize()
        if s >= args.warmup:
            times.append(time.perf_counter() - t0)
    print(eng.describe(), flush=True)
    med = statistics.median(times)
    what = ("unpartitioned" if args.flat else f"2^{args.keys_log2} keys") + (", select list on the device" if args.projection else "")
    print(f"P3 as a sequence ({what}, 2^{args.batch_log2}-event pushes, {args.lib or 'this build'}): {med * 1e3:.3f} ms per step "
          f"(median of {len(times)}; min {min(times) * 1e3:.3f}, max {max(times) * 1e3:.3f}), {B / med:.3e} events/s; "
          f"stats {eng.stats()}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
