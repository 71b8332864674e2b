"""The P3 workload as a SEQUENCE (`->` replaced by `,`) at bench size through the engine: 2^20 keys, 2^22-event
batches resident in HBM, steady state (the first pushes fill the `within` window and are not timed), step time per
push and events/s with the spread over the timed pushes.  SG_NO_SEQ=1 runs the same query on the general kernel
(what the engine did before the stencil kernel of seq_kernels.hip); rocprofv3 wraps this script for kernel traces.

    python tools/exp_seq.py [steps] [warmup]
"""
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    sa = importlib.import_module("siddhi-1_amd")
    synth = importlib.import_module("siddhi-1_amd.synth")
    K, B = 1 << 20, 1 << 22
    app = sa.parse_app(synth.P3_QUERY.replace(" -> ", ", "))
    cq = sa.compile_query(app, app.queries[0], sa.StringDictionary())
    dev = torch.device("cuda", 0)
    bats = [synth.stock_ticks_torch(torch, s * B, B, K, dev) for s in range(warmup + steps)]
    torch.cuda.synchronize()
    eng = sa.NativeEngine(sa.load_hip_library(), "sg_", cq.ir, n_keys=K, max_batch=B, partial_capacity=32,
                          match_capacity=2 * B, device=0)
    times = []
    for s, t in enumerate(bats):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.push(0, s * B, (B, t["ts"].data_ptr(), [t["symbol"].data_ptr(), t["price"].data_ptr(), t["volume"].data_ptr()],
                            t["key"].data_ptr()), [0, 1, 2], mem=sa.native.SG_MEM_DEVICE)
        m = eng.poll_device()
        eng.release(m)
        eng.synchronize()
        if s >= warmup:
            times.append(time.perf_counter() - t0)
    print(eng.describe(), flush=True)
    med = statistics.median(times)
    print(f"P3 as a sequence: {med * 1e3:.3f} ms per step (median of {len(times)}; min {min(times) * 1e3:.3f}, "
          f"max {max(times) * 1e3:.3f}), {B / med:.3e} events/s; stats {eng.stats()}", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
