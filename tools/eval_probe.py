#!/usr/bin/env python3
"""Time the caption metrics at the workload's own size: 5000 images, K = 5 references, S = 50 columns, seeded
Zipf-distributed ids over the GPT-2 vocabulary.

    python tools/eval_probe.py [--out profiles/eval_metrics.json] [--no-generation]

Recorded: corpus build time (wall, after a warm-up, ending in a synchronise); device scoring time of all images
(pgca_cider_rows + pgca_bleu_stats + two pgca_token_overlap, device events, median of 10 after a warm-up); the time of
the tests/eval_refs.py restatement of CIDEr and the BLEU integers on this host for the same input; and the scoring
time per image as a share of the generation time per image at ``evaluation.generate_config`` of configs/default.yaml
(one batch of 8 images through the full-size model with freshly initialised weights, after a warm-up batch).
No threshold: the figures are written down, nothing is asserted.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_refs as E  # noqa: E402
from pgca_amd import hip  # noqa: E402
from pgca_amd.config import Config, generate_kwargs  # noqa: E402
from pgca_amd.evaluation import ReferenceCorpus  # noqa: E402

N, K, S, VOCAB, DEV = 5000, 5, 50, 50257, "cuda:0"
I32, I64, F64 = torch.int32, torch.int64, torch.float64


def make_input(seed=2026):
    rng = np.random.default_rng(seed)
    ref_ids = np.minimum(rng.zipf(1.2, (N, K, S)) - 1, VOCAB - 1).astype(np.int64)
    ref_len = rng.integers(8, S + 1, (N, K)).astype(np.int32)
    pred_len = rng.integers(4, S + 1, N).astype(np.int32)
    pred_ids = ref_ids[:, 0].copy()
    redraw = rng.random((N, S)) < 0.3
    pred_ids[redraw] = np.minimum(rng.zipf(1.2, int(redraw.sum())) - 1, VOCAB - 1)
    cols = np.arange(S)
    ref_ids[cols[None, None] >= ref_len[..., None]] = VOCAB
    pred_ids[cols[None] >= pred_len[:, None]] = VOCAB
    return pred_ids, pred_len, ref_ids, ref_len


def timed(fn, repeats=10):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics.json"))
    ap.add_argument("--no-generation", action="store_true")
    args = ap.parse_args()
    hip.load()
    pred_ids, pred_len, ref_ids, ref_len = make_input()
    arch = types.SimpleNamespace(gpt=types.SimpleNamespace(base_vocab=VOCAB))
    p_ids, p_len = torch.from_numpy(pred_ids).to(DEV), torch.from_numpy(pred_len).to(DEV)
    r_ids, r_len = torch.from_numpy(ref_ids).to(DEV), torch.from_numpy(ref_len).to(DEV)
    zero = torch.zeros((), dtype=I64, device=DEV)

    corpus = ReferenceCorpus(arch, r_ids, r_len, zero)          # warm-up
    torch.cuda.synchronize()
    builds = []
    for _ in range(3):
        t0 = time.perf_counter()
        corpus = ReferenceCorpus(arch, r_ids, r_len, zero)
        torch.cuda.synchronize()
        builds.append((time.perf_counter() - t0) * 1e3)

    score, flag = torch.empty(N, dtype=F64, device=DEV), torch.empty(N, dtype=I32, device=DEV)
    stats = torch.empty(N, 10, dtype=I64, device=DEV)
    over = torch.empty(2, N, 2, dtype=I32, device=DEV)
    b0, b1 = r_ids[:, 0].contiguous(), r_ids[:, 1].contiguous()
    l0, l1 = r_len[:, 0].contiguous(), r_len[:, 1].contiguous()

    def cider():
        hip.cider_rows(p_ids, p_len, r_ids, r_len, N, K, S, VOCAB, corpus.table_keys, corpus.table_df, corpus.table_off,
                       corpus.n_docs, 6.0, score, flag)

    def bleu():
        hip.bleu_stats(p_ids, p_len, r_ids, r_len, N, K, S, VOCAB, stats)

    def overlap():
        hip.token_overlap(p_ids, p_len, b0, l0, N, S, over[0])
        hip.token_overlap(p_ids, p_len, b1, l1, N, S, over[1])

    def scoring():
        cider()
        bleu()
        overlap()

    result = {"shape": {"images": N, "references": K, "columns": S, "vocab": VOCAB, "ids": "zipf(1.2), seed 2026"},
              "device": torch.cuda.get_device_name(0),
              "table_sizes": corpus.table_sizes,
              "corpus_build_ms": {"median": float(np.median(builds)), "runs": builds},
              "device_ms": {name: dict(zip(("median", "min", "max"), timed(fn)))
                            for name, fn in (("cider_rows", cider), ("bleu_stats", bleu), ("token_overlap_x2", overlap),
                                             ("scoring", scoring))}}
    scoring()
    got_score, got_stats = score.cpu().numpy(), stats.cpu().tolist()

    preds = [pred_ids[i, :pred_len[i]].tolist() for i in range(N)]
    refs = [[ref_ids[i, k, :ref_len[i, k]].tolist() for k in range(K)] for i in range(N)]
    t0 = time.perf_counter()
    want_score, _ = E.cider_rows(preds, refs)
    t1 = time.perf_counter()
    want_stats = [E.bleu_stats(p, r) for p, r in zip(preds, refs)]
    t2 = time.perf_counter()
    result["host_restatement_ms"] = {"cider_rows": (t1 - t0) * 1e3, "bleu_stats": (t2 - t1) * 1e3}
    result["agreement"] = {"cider_max_abs_err": float(np.abs(got_score - np.array(want_score)).max()),
                           "bleu_stats_equal": got_stats == want_stats}
    result["scoring_us_per_image"] = result["device_ms"]["scoring"]["median"] * 1e3 / N

    if not args.no_generation:
        from pgca_amd.model import PreferenceGuidedCaptioningModel
        cfg = Config(os.path.join(ROOT, "configs", "default.yaml"))
        mc, kw = cfg.get_model_config(), generate_kwargs(cfg)
        model = PreferenceGuidedCaptioningModel(vision_model=mc["vision_model"], text_model=mc["text_model"],
                                                projection_dim=mc["projection_dim"], freeze_vision_backbone=True,
                                                seed=0, device=DEV)
        B = 8
        images = torch.randn(B, 3, model.arch.vit.image, model.arch.vit.image, generator=torch.Generator().manual_seed(1))
        g = torch.Generator(device=DEV).manual_seed(1)
        model.generate_token_ids(images, generator=g, **kw)     # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ids = model.generate_token_ids(images, generator=g, **kw)
        torch.cuda.synchronize()
        gen_ms = (time.perf_counter() - t0) * 1e3 / B
        result["generation"] = {"generate_config": kw, "batch": B, "tokens_returned": int(ids.shape[1]),
                                "ms_per_image": gen_ms, "weights": "freshly initialised"}
        result["scoring_share_of_generation"] = result["scoring_us_per_image"] * 1e-3 / gen_ms
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
