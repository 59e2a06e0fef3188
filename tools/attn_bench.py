#!/usr/bin/env python3
"""Attention forward / backward micro-benchmark (random bf16 data, ragged right padding as the synthetic workload).

    python tools/attn_bench.py [--seqs 256] [--heads 16] [--S 128] [--causal 1] [--drop 0.1]

--split 1 also times the split backward (pgca_attention_bwd_split, S <= 1024); where S <= 512 the one-pass backward is
timed in the same process.  The forward and the backward variants take turns, --repeats windows each (median, min and
max reported).  --json appends the figures as one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pgca_amd import hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--S", type=int, default=128)
    ap.add_argument("--causal", type=int, default=1)
    ap.add_argument("--drop", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--packed", type=int, default=0, help="1: packed rows (cu offsets, the training layout), lengths 16..S")
    ap.add_argument("--split", type=int, default=0, choices=[0, 1], help="1: time pgca_attention_bwd_split as well")
    ap.add_argument("--repeats", type=int, default=1, help="timed windows per kernel (the median is reported)")
    ap.add_argument("--json", type=str, default=None, help="append the figures to this file as one JSON line")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hip.load()
    B, S, heads = args.seqs, args.S, args.heads
    H = heads * 64
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * S, 3 * H, generator=g).to(dev).bfloat16()
    dout = torch.randn(B * S, H, generator=g).to(dev).bfloat16()
    lens = torch.randint(16, S + 1, (B,), generator=g)
    mask = (torch.arange(S)[None] < lens[:, None]).int().to(dev) if args.causal else None
    out = torch.empty(B * S, H, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B, heads, S, device=dev)
    dqkv = torch.empty(B * S, 3 * H, dtype=torch.bfloat16, device=dev)
    d = hip.drop_args(77, args.drop)
    cu = None
    if args.packed:
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = torch.cumsum(lens, 0)
        cu = cu.to(dev)
        mask = None

    def timeit(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    # the kernels are timed alternately, --repeats times each, so that drift of a shared machine hits all alike
    variants = {}
    if S <= 512:
        variants["onepass"] = hip.attention_bwd
    if args.split:
        variants["split"] = hip.attention_bwd_split
    tfs, times = [], {k: [] for k in variants}
    for _ in range(args.repeats):
        tfs.append(timeit(lambda: hip.attention_fwd(qkv, mask, B, S, heads, bool(args.causal), out, lse, drop=d, cu=cu)))
        for k, fn in variants.items():
            times[k].append(timeit(lambda: fn(qkv, out, dout, lse, mask, B, S, heads, bool(args.causal), dqkv, drop=d,
                                              cu=cu)))
    tfs.sort()
    tf = tfs[len(tfs) // 2]
    rows = int(lens.sum()) if args.packed else B * S
    # algorithmic flop: 4 S^2 64 per head forward, 10 S^2 64 backward (five matmuls), whichever kernel runs them
    fl = 4.0 * heads * 64 * (float((lens.double() ** 2).sum()) if args.packed else B * S * S)
    byt_f = rows * H * 2 * 4 + rows * heads * 4
    byt_b = rows * H * 2 * (3 + 1 + 1 + 3)
    line = (f"packed={args.packed} B={B} heads={heads} S={S} causal={args.causal} drop={args.drop}: "
            f"fwd {tf:7.1f} us ({fl / tf / 1e6:6.1f} TF/s, {byt_f / tf / 1e6:5.2f} TB/s; "
            f"min {tfs[0]:.1f} max {tfs[-1]:.1f})")
    rec = {"seqs": B, "heads": heads, "S": S, "causal": args.causal, "drop": args.drop, "packed": args.packed,
           "iters": args.iters, "repeats": args.repeats, "fwd_us": round(tf, 1),
           "fwd": {"median_us": round(tf, 1), "min_us": round(tfs[0], 1), "max_us": round(tfs[-1], 1),
                   "windows_us": [round(x, 1) for x in tfs], "tflops": round(fl / tf / 1e6, 1)},
           "bwd": {}}
    for k, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        line += (f"   bwd[{k}] {med:7.1f} us ({2.5 * fl / med / 1e6:6.1f} TF/s, {byt_b / med / 1e6:5.2f} TB/s; "
                 f"min {ts[0]:.1f} max {ts[-1]:.1f})")
        rec["bwd"][k] = {"median_us": round(med, 1), "min_us": round(ts[0], 1), "max_us": round(ts[-1], 1),
                         "windows_us": [round(x, 1) for x in ts], "tflops": round(2.5 * fl / med / 1e6, 1)}
    print(line)
    if args.json:
        with open(args.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
