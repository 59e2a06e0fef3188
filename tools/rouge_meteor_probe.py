#!/usr/bin/env python3
"""Time ``pgca_rouge_stats`` and ``pgca_meteor_stats`` at the workload of tools/eval_probe.py: 5000 images, K = 5
references, S = 50 columns, the same seeded Zipf-distributed ids over the GPT-2 vocabulary.

    python tools/rouge_meteor_probe.py [--out profiles/eval_rouge_meteor.json]

Recorded: device time of each kernel over all images (device events, median of 10 after a warm-up) and the time of the
tests/rouge_meteor_refs.py restatement (full LCS table, list-popping METEOR matching) of the same integers on this host,
which is what the kernels are measured against; and whether the integers agree.  A sibling of eval_probe.py so that
profiles/eval_metrics.json keeps its content.  No threshold: the figures are written down, nothing is asserted.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import rouge_meteor_refs as R  # noqa: E402
from eval_probe import DEV, K, N, S, VOCAB, make_input, timed  # noqa: E402
from pgca_amd import hip  # noqa: E402
from pgca_amd.evaluation import meteor_from_stats, rouge_from_stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_rouge_meteor.json"))
    args = ap.parse_args()
    hip.load()
    pred_ids, pred_len, ref_ids, ref_len = make_input()
    p_ids, p_len = torch.from_numpy(pred_ids).to(DEV), torch.from_numpy(pred_len).to(DEV)
    r_ids, r_len = torch.from_numpy(ref_ids).to(DEV), torch.from_numpy(ref_len).to(DEV)
    rouge = torch.empty(N, 6, dtype=torch.int32, device=DEV)
    meteor = torch.empty(N, K, 2, dtype=torch.int32, device=DEV)

    def rouge_kernel():
        hip.rouge_stats(p_ids, p_len, r_ids, r_len, N, K, S, VOCAB, rouge)

    def meteor_kernel():
        hip.meteor_stats(p_ids, p_len, r_ids, r_len, N, K, S, VOCAB, meteor)

    def both():
        rouge_kernel()
        meteor_kernel()

    result = {"shape": {"images": N, "references": K, "columns": S, "vocab": VOCAB, "ids": "zipf(1.2), seed 2026"},
              "device": torch.cuda.get_device_name(0),
              "device_ms": {name: dict(zip(("median", "min", "max"), timed(fn)))
                            for name, fn in (("rouge_stats", rouge_kernel), ("meteor_stats", meteor_kernel),
                                             ("both", both))}}
    both()
    got_rouge, got_meteor = rouge.cpu().tolist(), meteor.cpu().tolist()

    preds = [pred_ids[i, :pred_len[i]].tolist() for i in range(N)]
    refs = [[ref_ids[i, k, :ref_len[i, k]].tolist() for k in range(K)] for i in range(N)]
    t0 = time.perf_counter()
    want_rouge = [R.rouge_stats(p, r) for p, r in zip(preds, refs)]
    t1 = time.perf_counter()
    want_meteor = [R.meteor_stats(p, r) for p, r in zip(preds, refs)]
    t2 = time.perf_counter()
    result["measured_against"] = "tests/rouge_meteor_refs.py (plain Python, one thread) on the host of the same machine"
    result["host_restatement_ms"] = {"rouge_stats": (t1 - t0) * 1e3, "meteor_stats": (t2 - t1) * 1e3}
    result["agreement"] = {"rouge_stats_equal": got_rouge == want_rouge, "meteor_stats_equal": got_meteor == want_meteor}
    result["both_us_per_image"] = result["device_ms"]["both"]["median"] * 1e3 / N
    result["scores"] = dict(rouge_from_stats(got_rouge),
                            meteor=meteor_from_stats(got_meteor, pred_len.tolist(), ref_len.tolist()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
