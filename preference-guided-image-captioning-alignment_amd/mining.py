"""Stage-2 preference data from the model's own captions, on the device.

``PreferenceMiner.mine`` closes the loop the pipeline leaves open after Stage 1: sample ``num_candidates`` captions per
image (``generate_candidates``), score each one, apply the reference's pairing rule
(``UltraFeedbackDataset._process_scored_captions``, data/loader.py:416-451: sort by score, pair neighbours whose score
difference reaches ``preference_threshold``) and hand back the reference's Stage-2 batch dict, which
``steps.DPOStep.prepare`` takes unchanged.  Everything between the sampled ids and the finished batch is HIP
(csrc/mine.hip): id conversion, scoring, ranking, de-duplication, pairing and batch assembly.  The host reads back four
bytes per mined batch, the pair count.

``MinedPreferenceData`` collects mined batches (every image once, in pinned host memory) and serves them as an ordinary
Stage-2 loader.
"""
from __future__ import annotations

import math
from typing import Any, Callable, Dict, Iterator, List, Optional, Union

import torch

from . import hip

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8
SCORERS = ("alignment", "logprob")
BATCH_KEYS = ("preferred_ids", "preferred_mask", "rejected_ids", "rejected_mask", "preference_score")


class PreferenceMiner:
    """``scorer``: ``"alignment"`` (cosine of the Stage-1 image and text towers), ``"logprob"`` (the decoder's own
    length-normalised log-probability) or a callable ``scorer(images, dec_ids [B, n, S], dec_mask [B, n, S]) -> [B, n]``
    float32 on the device.  ``rule``: ``"adjacent"`` (the reference's) or ``"best_worst"``.  ``num_candidates`` <= 64
    (one wave ranks one image).  ``min_tokens``: shorter captions are left out - with fewer than two tokens no position
    is scored, the mean log-probability is 0/0 and ``DPOStep`` would drop the whole batch.  ``decode_rows``: captions
    decoded (and scored) at once; images are taken ``decode_rows // num_candidates`` at a time."""

    def __init__(self, model, num_candidates: int = 4, rule: str = "adjacent", threshold: float = 0.0,
                 scorer: Union[str, Callable] = "alignment", max_length: int = 50, min_tokens: int = 2,
                 temperature: float = 1.0, top_p: float = 0.9, top_k: int = 0, repetition_penalty: float = 1.1,
                 no_repeat_ngram_size: int = 0, decode_rows: int = 64):
        n = int(num_candidates)
        if not 1 <= n <= 64:
            raise ValueError(f"num_candidates={num_candidates}: expected 1 .. 64 (one 64-lane wave ranks one image)")
        if rule not in hip.MINE_RULES:
            raise ValueError(f"rule={rule!r}: expected one of {sorted(hip.MINE_RULES)}")
        if not callable(scorer) and scorer not in SCORERS:
            raise ValueError(f"scorer={scorer!r}: expected one of {SCORERS} or a callable")
        if int(max_length) < 3:
            raise ValueError(f"max_length={max_length}: a scored caption needs two tokens after the prefix")
        if math.isnan(float(threshold)):
            raise ValueError("threshold is NaN")
        self.model, self.n, self.rule, self.threshold, self.scorer = model, n, rule, float(threshold), scorer
        self.max_length, self.min_tokens = int(max_length), int(min_tokens)
        self.sampling = dict(temperature=float(temperature), top_p=float(top_p), top_k=int(top_k),
                             repetition_penalty=float(repetition_penalty),
                             no_repeat_ngram_size=int(no_repeat_ngram_size))
        self.chunk = max(1, int(decode_rows) // n)

    @torch.no_grad()
    def mine(self, images: torch.Tensor, generator: Optional[torch.Generator] = None) -> Dict[str, Any]:
        """images [B, 3, I, I] -> the Stage-2 batch dict of the mined pairs (``image``, ``preferred_ids``,
        ``preferred_mask``, ``rejected_ids``, ``rejected_mask``, ``preference_score``: ``n_pairs`` rows on the device)
        plus ``pair_image`` [n_pairs] (the image of each pair), ``scores`` / ``rank`` [B, n], ``candidates`` [B, n, S]
        (the sampled ids, [PAD] after them), ``lengths`` [B, n], ``n_pairs`` and ``source_images`` (the B images
        on the device, which ``MinedPreferenceData.add`` stores once each)."""
        m = self.model
        was = m.training
        m.eval()
        try:
            return self._mine(images.to(m.device, F32).contiguous(), generator)
        finally:
            m.train(was)

    def _mine(self, images: torch.Tensor, generator) -> Dict[str, Any]:
        m, n, dev = self.model, self.n, self.model.device
        arch = m.arch
        base, S, B = arch.gpt.base_vocab, self.max_length - 1, images.shape[0]
        R = B * n
        dec_pad, text_pad = base, base          # [PAD] is the first added id of both tokenizers
        cand = torch.full((R, S), dec_pad, dtype=I64, device=dev)
        lengths = torch.empty(R, dtype=I64, device=dev)
        dec_ids, dec_mask = torch.empty(R, S, dtype=I64, device=dev), torch.empty(R, S, dtype=I64, device=dev)
        text_ids, text_mask = torch.empty(R, S, dtype=I64, device=dev), torch.empty(R, S, dtype=I32, device=dev)
        text_len, out_len = torch.empty(R, dtype=I32, device=dev), torch.empty(R, dtype=I32, device=dev)
        scores = torch.empty(B, n, dtype=F32, device=dev)
        bad_id = torch.zeros((), dtype=torch.bool, device=dev)
        for b0 in range(0, B, self.chunk):
            b1 = min(B, b0 + self.chunk)
            Bc, rows = b1 - b0, slice(b0 * n, b1 * n)
            # the ViT runs once per image: the same embedding conditions the decoder and meets the captions in the scorer
            emb = m.vision_encoder(images[b0:b1])["embeddings"].clone()
            ids, logp, lens = m.generate_candidates(images[b0:b1], n, max_length=self.max_length, generator=generator,
                                                    image_embeddings=emb, **self.sampling)
            cand[rows, :ids.shape[2]] = ids.view(Bc * n, -1)
            lengths[rows] = lens.reshape(-1)
            hip.candidate_rows(cand[rows], lengths[rows], Bc * n, S, base, arch.dec_vocab, dec_pad, text_pad,
                               dec_ids[rows], dec_mask[rows], text_ids[rows], text_mask[rows], text_len[rows],
                               out_len[rows])
            if self.scorer == "alignment":
                # checked on the device before the gather: an id past the text tower's table never reaches it (it is
                # replaced by [PAD]) and the flag travels with the one read-back below
                t_ids = text_ids[rows]
                wrong = (t_ids < 0) | (t_ids >= arch.text_vocab)
                bad_id |= wrong.any()
                t_ids.masked_fill_(wrong, text_pad)
                _, _, temb = m.text_encoder.engine.forward(t_ids, text_mask[rows], save=False)
                hip.group_cosine(emb, temb, Bc, n, arch.proj_dim, scores[b0:b1])
            elif self.scorer == "logprob":
                scores[b0:b1] = logp / lens.to(F32)
            else:
                s = self.scorer(images[b0:b1], dec_ids[rows].view(Bc, n, S), dec_mask[rows].view(Bc, n, S))
                scores[b0:b1] = s.to(dev, F32).reshape(Bc, n)
        ok = (text_len >= 0).to(U8)
        rank = torch.empty(B, n, dtype=I32, device=dev)
        pair_win, pair_lose = torch.empty(B, n, dtype=I32, device=dev), torch.empty(B, n, dtype=I32, device=dev)
        pair_margin, pair_count = torch.empty(B, n, dtype=F32, device=dev), torch.empty(B, dtype=I32, device=dev)
        hip.mine_pairs(scores, dec_ids, out_len, ok, B, n, S, self.min_tokens, self.rule, self.threshold, rank, pair_win,
                       pair_lose, pair_margin, pair_count)
        cap = max(1, B * (n - 1))
        out = {k: torch.empty(cap, S, dtype=I64, device=dev) for k in BATCH_KEYS[:4]}
        out["preference_score"] = torch.empty(cap, dtype=F32, device=dev)
        pair_image, n_dev = torch.empty(cap, dtype=I32, device=dev), torch.empty(1, dtype=I32, device=dev)
        hip.pair_rows(pair_win, pair_lose, pair_margin, pair_count, dec_ids, dec_mask, B, n, S, cap, dec_pad,
                      out["preferred_ids"], out["preferred_mask"], out["rejected_ids"], out["rejected_mask"], pair_image,
                      out["preference_score"], n_dev)
        n_pairs = int(torch.where(bad_id, torch.full_like(n_dev, -1), n_dev))      # the one read-back: 4 bytes
        if n_pairs < 0:
            raise RuntimeError(f"a scorer row holds an id outside the text tower's vocabulary [0, {arch.text_vocab})")
        out = {k: v[:n_pairs] for k, v in out.items()}
        pair_image = pair_image[:n_pairs]
        out.update(image=images[pair_image.long()], pair_image=pair_image, scores=scores, rank=rank,
                   candidates=cand.view(B, n, S), lengths=lengths.view(B, n), out_len=out_len.view(B, n),
                   pair_count=pair_count, n_pairs=n_pairs, source_images=images)
        return out


class MinedPreferenceData:
    """Mined batches as a Stage-2 dataset: ``add`` keeps the images of a mined batch once (pinned host memory) next to
    its pair rows; ``loader`` yields the reference's batch dicts (loader.py:487-497)."""

    def __init__(self) -> None:
        self._images: List[torch.Tensor] = []
        self._rows: List[Dict[str, torch.Tensor]] = []
        self._n_images = 0
        self.stats = {"images": 0, "candidates": 0, "left_out": 0, "pairs": 0}
        self._frozen: Optional[Dict[str, torch.Tensor]] = None

    @staticmethod
    def _host(t: torch.Tensor) -> torch.Tensor:
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=t.is_cuda)
        h.copy_(t)
        return h

    def add(self, mined: Dict[str, Any]) -> None:
        """``mined``: what ``PreferenceMiner.mine`` returned."""
        rank, images = mined["rank"], mined["source_images"]
        self.stats["images"] += int(rank.shape[0])
        self.stats["candidates"] += int(rank.numel())
        self.stats["left_out"] += int((rank < 0).sum())
        self.stats["pairs"] += int(mined["n_pairs"])
        self._images.append(self._host(images.detach().to(F32)))
        rows = {k: self._host(mined[k]) for k in BATCH_KEYS}
        rows["pair_image"] = self._host(mined["pair_image"]).long() + self._n_images
        self._rows.append(rows)
        self._n_images += int(images.shape[0])
        self._frozen = None

    def __len__(self) -> int:
        return self.stats["pairs"]

    def _tables(self) -> Dict[str, torch.Tensor]:
        if self._frozen is None:
            t = {k: torch.cat([r[k] for r in self._rows]) for k in BATCH_KEYS + ("pair_image",)}
            t["image"] = torch.cat(self._images)
            self._frozen = t
        return self._frozen

    def loader(self, batch_size: int, shuffle: bool = False, seed: int = 0, drop_last: bool = True,
               max_batches: Optional[int] = None) -> "_MinedLoader":
        return _MinedLoader(self._tables() if len(self) else None, len(self), int(batch_size), shuffle, int(seed),
                            drop_last, max_batches)


class _MinedLoader:
    """``len()`` batches per pass; a shuffled loader draws a new order every pass from its own seeded generator."""

    def __init__(self, tables, n, batch_size, shuffle, seed, drop_last, max_batches):
        self.t, self.n, self.bs, self.shuffle, self.drop_last = tables, n, batch_size, shuffle, drop_last
        self.g = torch.Generator().manual_seed(seed)
        full = n // batch_size if drop_last else (n + batch_size - 1) // batch_size
        self.batches = full if max_batches is None else min(full, int(max_batches))

    def __len__(self) -> int:
        return self.batches

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        order = torch.randperm(self.n, generator=self.g) if self.shuffle else torch.arange(self.n)
        for i in range(self.batches):
            idx = order[i * self.bs:(i + 1) * self.bs]
            batch = {k: self.t[k][idx] for k in BATCH_KEYS}
            batch["image"] = self.t["image"][self.t["pair_image"][idx]]
            yield batch
