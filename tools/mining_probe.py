#!/usr/bin/env python3
"""Measure preference mining on the GPU and write profiles/mining.json.

    python tools/mining_probe.py [--commit <hash>] [--out profiles/mining.json]

Two measurements:

* throughput: images/s of one ``PreferenceMiner.mine`` call at ViT-B/32 + GPT-2-medium, 4 candidates per image, 16
  images (random weights: the token statistics, hence the caption lengths, are those of an untrained decoder), and where
  the time goes - generation, the scorer's text tower and each of the four kernels of csrc/mine.hip (HIP events around
  the same calls ``mine`` makes).  No target: the file records what was measured.
* score agreement: how far the public surface ``model(images, ids, mask, mode="contrastive")`` moves when the same rows
  are computed in another batch composition (all B*n rows at once against n calls of B rows), at the geometry of
  tests/test_mining_gpu.py.  The miner's alignment scores are compared with that surface under 4 x this value (the
  factor covers the ViT seeing another batch as well); a batch-invariant surface leaves the summation bound
  4 * P * 2^-24.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps


def throughput():
    from pgca_amd import hip
    from pgca_amd.mining import PreferenceMiner
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    model = PreferenceGuidedCaptioningModel("openai/clip-vit-base-patch32", "gpt2-medium", 512, freeze_vision_backbone=True,
                                            device=DEV, seed=1)
    arch = model.arch
    B, n = 16, 4
    images = torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=torch.Generator().manual_seed(0)).to(DEV)
    miner = PreferenceMiner(model, num_candidates=n)
    gen = torch.Generator(device=DEV).manual_seed(7)
    miner.mine(images, generator=gen)                       # sizes the workspace, captures the decode graphs
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mined = miner.mine(images, generator=gen)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    wall = sorted(walls)[1]
    # the pieces, on the calls mine() makes
    S, base, R = miner.max_length - 1, arch.gpt.base_vocab, B * n
    model.eval()
    with torch.no_grad():
        emb, t_vit = timed(lambda: model.vision_encoder(images)["embeddings"].clone())
        (ids, logp, lens), t_gen = timed(lambda: model.generate_candidates(images, n, max_length=miner.max_length,
                                                                           generator=gen, image_embeddings=emb,
                                                                           **miner.sampling))
        cand = torch.full((R, S), base, dtype=torch.int64, device=DEV)
        cand[:, :ids.shape[2]] = ids.view(R, -1)
        lengths = lens.reshape(-1).contiguous()
        i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=DEV)   # noqa: E731
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)   # noqa: E731
        dec_ids, dec_mask, text_ids, text_mask, text_len, out_len = i64(R, S), i64(R, S), i64(R, S), i32(R, S), i32(R), i32(R)
        _, t_rows = timed(lambda: hip.candidate_rows(cand, lengths, R, S, base, arch.dec_vocab, base, base, dec_ids,
                                                     dec_mask, text_ids, text_mask, text_len, out_len), 20)
        temb, t_text = timed(lambda: model.text_encoder.engine.forward(text_ids, text_mask, save=False)[2], 3)
        scores = torch.empty(B, n, device=DEV)
        _, t_cos = timed(lambda: hip.group_cosine(emb, temb, B, n, arch.proj_dim, scores), 20)
        rank, pw, pl, cnt = i32(B, n), i32(B, n), i32(B, n), i32(B)
        pm = torch.empty(B, n, device=DEV)
        _, t_mine = timed(lambda: hip.mine_pairs(scores, dec_ids, out_len, None, B, n, S, 2, "adjacent", 0.0, rank, pw, pl,
                                                 pm, cnt), 20)
        cap = B * (n - 1)
        o = [i64(cap, S) for _ in range(4)]
        pi, ps, npairs = i32(cap), torch.empty(cap, device=DEV), i32(1)
        _, t_pair = timed(lambda: hip.pair_rows(pw, pl, pm, cnt, dec_ids, dec_mask, B, n, S, cap, base, o[0], o[1], o[2],
                                                o[3], pi, ps, npairs), 20)
    return {"model": "openai/clip-vit-base-patch32 + gpt2-medium (random weights), ViT frozen",
            "images": B, "num_candidates": n, "max_length": miner.max_length, "scorer": "alignment",
            "mine_wall_ms": 1e3 * wall, "mine_wall_ms_runs": [1e3 * w for w in walls], "images_per_s": B / wall,
            "pairs": int(mined["n_pairs"]), "mean_generated_tokens": float(mined["lengths"].float().mean()),
            "breakdown_gpu_ms": {"vit_and_head": t_vit, "generation": t_gen, "scorer_text_tower": t_text,
                                 "pgca_candidate_rows": t_rows, "pgca_group_cosine": t_cos, "pgca_mine_pairs": t_mine,
                                 "pgca_pair_rows": t_pair}}


def agreement():
    """The geometry of tests/test_mining_gpu.py: tiny_arch, 4 images, n = 4, max_length 12."""
    from pgca_amd.arch import tiny_arch
    from pgca_amd.mining import PreferenceMiner
    from pgca_amd.model import PreferenceGuidedCaptioningModel
    arch = tiny_arch()
    worst, worst_vs_miner = 0.0, 0.0
    for seed in (3, 4, 5):
        model = PreferenceGuidedCaptioningModel(freeze_vision_backbone=True, arch=arch, seed=seed, device=DEV)
        model.eval()
        B, n, L = 4, 4, 12
        images = torch.randn(B, 3, arch.vit.image, arch.vit.image, generator=torch.Generator().manual_seed(seed)).to(DEV)
        miner = PreferenceMiner(model, num_candidates=n, max_length=L)
        mined = miner.mine(images, generator=torch.Generator(device=DEV).manual_seed(11))
        S, base = L - 1, arch.gpt.base_vocab
        cand, lens = mined["candidates"].view(B * n, S), mined["lengths"].view(-1)
        live = torch.arange(S, device=DEV)[None] < lens[:, None]
        keep = live & (cand < base)
        # scorer rows: the ordinary tokens, compacted to the left (a stable sort of the keep flags)
        order = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices
        text_ids = torch.where(torch.gather(keep, 1, order), torch.gather(cand, 1, order), torch.full_like(cand, base))
        text_mask = torch.gather(keep, 1, order).long()
        rep = images.repeat_interleave(n, dim=0)

        def cosine(rows):
            out = model(rep[rows], text_ids[rows], text_mask[rows], mode="contrastive")
            return (out["image_embeddings"].double() * out["text_embeddings"].double()).sum(1)

        with torch.no_grad():
            every = torch.arange(B * n, device=DEV)
            whole = cosine(every)
            parts = torch.empty_like(whole)
            for j in range(n):
                parts[j::n] = cosine(every[j::n])
        worst = max(worst, float((whole - parts).abs().max()))
        worst_vs_miner = max(worst_vs_miner, float((mined["scores"].view(-1).double() - whole).abs().max()))
    P = arch.proj_dim
    floor = 4 * P * 2.0 ** -24
    return {"geometry": "tiny_arch, 4 images x 4 candidates, max_length 12, 3 seeds",
            "surface_batch_composition_max_abs_diff": worst, "summation_bound_4P_2^-24": floor,
            "bound": 4 * worst if worst > 0 else floor,
            "bound_rule": "4 x the surface's own batch-composition difference; 4*P*2^-24 when that is zero",
            "miner_vs_surface_max_abs_diff_observed": worst_vs_miner}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mining.json"))
    args = ap.parse_args()
    result = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "score_agreement": agreement(),
              "throughput": throughput()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
