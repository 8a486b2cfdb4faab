#!/usr/bin/env python3
"""Interrupted repeats (prf_scan_interrupted_chunked) on a chromosome-sized stand-in: one JSON line with the device time (walk and
emission + sort apart), the lanes launched and dropped, the walk's steps per position and the memo hit rate.

    python3 tools/interrupted_timing.py [--length 50818468] [--kmin 1 --kmax 6 --min-repeats 3 --min-span 9 --max-interruptions 1]
    python3 tools/interrupted_timing.py --chunk 262144              # landing positions per lane (default: the library's; 0: one
                                                                    # lane per motif size, the engine before chunks)
    python3 tools/interrupted_timing.py --by-k 0,0,1,1,1,1          # a budget per motif size kmin .. kmax
    python3 tools/interrupted_timing.py --model [--length ...]      # the CPU model (tests/interrupted_model.py) instead, no GPU
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "colab-repeat-finder_amd"), os.path.join(ROOT, "tests")]

import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=synth.CHR22_LEN)
    ap.add_argument("--seed", type=int, default=22)
    ap.add_argument("--kmin", type=int, default=1)
    ap.add_argument("--kmax", type=int, default=6)
    ap.add_argument("--min-repeats", type=int, default=3)
    ap.add_argument("--min-span", type=int, default=9)
    ap.add_argument("--max-interruptions", type=int, default=1)
    ap.add_argument("--by-k", default=None, metavar="M,M,...", help="max interruptions of every motif size kmin .. kmax, in place of "
                    "--max-interruptions (prf_scan_interrupted_by_k)")
    ap.add_argument("--memo-stride", type=int, default=8)
    ap.add_argument("--memo-slots", type=int, default=1 << 22)
    ap.add_argument("--chunk", type=int, default=None, help="landing positions per GPU lane (default: PRF_INT_CHUNK; 0: one lane per k)")
    ap.add_argument("--repeat", type=int, default=2, help="GPU: calls (the first one warms up)")
    ap.add_argument("--model", action="store_true", help="time the CPU model instead of the GPU")
    args = ap.parse_args()
    n_head = min(10_510_000, args.length // 5)
    seq = synth.chr_standin(length=args.length, seed=args.seed, n_head=n_head, n_tail=min(10_000, args.length // 100)).tobytes()
    by_k = None if args.by_k is None else [int(m) for m in args.by_k.split(",")]
    p = (args.kmin, args.kmax, args.min_repeats, args.min_span, 0 if by_k else args.max_interruptions)
    res = {"length": args.length, "kmin": args.kmin, "kmax": args.kmax, "min_repeats": args.min_repeats, "min_span": args.min_span,
           "max_interruptions": by_k or args.max_interruptions, "memo_stride": args.memo_stride, "memo_slots": args.memo_slots}
    if args.model:
        import interrupted_model as M
        ctr = {}
        t = time.perf_counter()
        if by_k:
            import interrupted_by_k_model as K
            rows = K.detect(seq, *p[:4], by_k, stride=args.memo_stride, slots=args.memo_slots, counters=ctr)
        else:
            rows = M.detect(seq, *p, stride=args.memo_stride, slots=args.memo_slots, counters=ctr)
        res.update(engine="cpu_model", seconds=round(time.perf_counter() - t, 2), rows=len(rows))
    else:
        import prf_native
        chunk = prf_native.INT_CHUNK if args.chunk is None else args.chunk
        ctx = prf_native.Context(0)
        extra = {} if by_k is None else {"max_interruptions_by_k": by_k}
        for _ in range(args.repeat):
            t = time.perf_counter()
            rows, stats, ctr = ctx.scan_interrupted([seq], *p, memo_stride=args.memo_stride, memo_slots=args.memo_slots, counters=True,
                                                    chunk=chunk, **extra)
            wall = time.perf_counter() - t
        ctx.close()
        res.update(engine="gpu", chunk=chunk, lanes=int(ctr["lanes"]), dropped_lanes=int(ctr["dropped_lanes"]), rows=len(rows), wall_s=round(wall, 3), scan_ms=round(stats.scan_ms, 2), walk_ms=round(stats.phase1_ms, 2),
                   emit_sort_ms=round(stats.phase2_ms, 2), candidates=int(stats.n_candidates), launches=int(stats.n_launches),
                   episodes_recorded=int(ctr["episodes"]))
    body = args.length - n_head - min(10_000, args.length // 100)
    nk = args.kmax - args.kmin + 1
    res.update(steps=int(ctr["steps"]), steps_per_position=round(ctr["steps"] / max(1, body) / nk, 3),
               memo_lookups=int(ctr["lookups"]), memo_hits=int(ctr["hits"]),
               memo_hit_rate=round(ctr["hits"] / ctr["lookups"], 4) if ctr["lookups"] else None)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
