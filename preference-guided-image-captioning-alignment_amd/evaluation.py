"""Caption evaluation where the generated ids are: BLEU, CIDEr, ROUGE, METEOR, diversity, preference win rate, alignment,
latency.

The reference scores decoded text on the host (evaluation/metrics.py: ``CaptioningMetrics``, ``EvaluationRunner``).  Here
the same formulas run over TOKEN IDS in HIP (csrc/eval.hip), next to the ids ``generate_token_ids`` leaves on the device.

A "word" is a base-vocabulary token id.  The decoder's specials ([PAD], [BOS], [EOS]: ids >= ``arch.gpt.base_vocab``) are
stripped first, by ``pgca_candidate_rows``, the conversion the mining scorer already uses.  The numbers are therefore the
reference's formulas applied to BPE tokens: they track a model inside this project and are NOT comparable with the
word-level BLEU / CIDEr / ROUGE / METEOR of papers (a word is often several tokens, which raises n-gram precision and
shortens the reach of a 4-gram).  ROUGE-1 / 2 / L and METEOR (exact-match stage: the stemmer and WordNet stages are the
identity on ids) are the order-sensitive scores of the set: the longest common subsequence and METEOR's chunk penalty see
word order beyond four tokens.  BERTScore and ``human_preference_correlation`` are not computed.

``ReferenceCorpus``  the stripped references of a loader and, per n-gram order, the sorted keys with their document
                     frequencies: built once, reused for every checkpoint or epoch; no generation runs.
``CaptionEvaluator`` generates, scores each batch on the device into per-image buffers and reads them back once.

Torch does the plumbing (sorting keys, counting runs, padding); key emission, per-image de-duplication, the idf lookup
and every score are kernels.
"""
from __future__ import annotations

import math
import time
from typing import Any, Dict, Iterable, List, Optional

import torch

from . import hip
from .config import generate_kwargs as config_generate_kwargs

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
CIDER_SIGMA = 6.0   # the reference's default (metrics.py:445)


def strip_rows(arch, ids: torch.Tensor, lengths: torch.Tensor, S: int):
    """Decoder rows ``ids`` int64 [R, W] with ``lengths`` [R] live columns -> ``(text_ids int64 [R, S], text_mask int32
    [R, S], text_len int32 [R])``: the base-vocabulary ids in order, [PAD] after them (``pgca_candidate_rows``).
    ``text_len`` is -1 for a row with an id outside the decoder's vocabulary."""
    dev, R, base = ids.device, ids.shape[0], arch.gpt.base_vocab
    ids = ids.to(I64).contiguous()
    lengths = lengths.to(I64).contiguous()
    scratch = torch.empty(2, R, S, dtype=I64, device=dev)
    text_ids, text_mask = torch.empty(R, S, dtype=I64, device=dev), torch.empty(R, S, dtype=I32, device=dev)
    text_len, out_len = torch.empty(R, dtype=I32, device=dev), torch.empty(R, dtype=I32, device=dev)
    hip.candidate_rows(ids, lengths, R, S, base, arch.dec_vocab, base, base, scratch[0], scratch[1], text_ids, text_mask,
                       text_len, out_len)
    return text_ids, text_mask, text_len


def batch_references(batch: Dict[str, Any]):
    """The references a batch carries, as ``(ids [B, K, W], mask [B, K, W], present [B, K] bool or None)``:
    ``reference_ids`` / ``reference_mask`` (optionally ``reference_present``), else ``caption_ids`` / ``caption_mask``
    (Stage 1, K = 1), else ``preferred_ids`` / ``preferred_mask`` (Stage 2 and mined batches, K = 1)."""
    if "reference_ids" in batch:
        ids, mask = batch["reference_ids"], batch["reference_mask"]
        if ids.dim() != 3:
            raise ValueError(f"reference_ids must be [B, K, S], got {tuple(ids.shape)}")
        return ids, mask, batch.get("reference_present")
    for name in ("caption", "preferred"):
        if name + "_ids" in batch:
            return batch[name + "_ids"][:, None], batch[name + "_mask"][:, None], None
    raise KeyError("the batch carries no references: expected reference_ids, caption_ids or preferred_ids")


class FirstBatches:
    """The first ``n`` batches of a loader, as often as asked."""

    def __init__(self, loader, n: Optional[int]):
        self.loader, self.n = loader, n

    def __iter__(self):
        for i, batch in enumerate(self.loader):
            if self.n is not None and i >= self.n:
                return
            yield batch


class ReferenceCorpus:
    """``ref_ids`` int64 [N, K, S] / ``ref_len`` int32 [N, K] (-1: absent, 0: present and empty) in loader order, and the
    document-frequency tables of orders 1..4: ``table_keys`` (sorted, signed), ``table_df``, ``table_off`` [5]."""

    def __init__(self, arch, ref_ids, ref_len, bad_rows):
        self.arch, self.ref_ids, self.ref_len, self.bad_rows = arch, ref_ids, ref_len, bad_rows
        self.N, self.K, self.S = ref_ids.shape
        self.n_docs = self.N
        dev, base = ref_ids.device, arch.gpt.base_vocab
        keys, dfs, off = [], [], [0]
        buf = torch.empty(self.N, self.K, self.S, dtype=I64, device=dev)
        for order in range(1, 5):
            hip.ngram_keys(ref_ids, ref_len, self.N, self.K, self.S, order, base, True, buf)
            k = torch.sort(buf.view(-1)).values
            uk, cnt = torch.unique_consecutive(k, return_counts=True)   # once per image: the run length is the df
            keep = uk != -1
            keys.append(uk[keep])
            dfs.append(cnt[keep])
            off.append(off[-1] + int(keys[-1].numel()))
        self.table_keys = torch.cat(keys + [torch.zeros(1, dtype=I64, device=dev)])   # never empty: one spare entry
        self.table_df = torch.cat(dfs + [torch.ones(1, dtype=I64, device=dev)])
        self.table_off = torch.tensor(off, dtype=I64, device=dev)
        self.table_sizes = [off[i + 1] - off[i] for i in range(4)]

    @classmethod
    def build(cls, loader: Iterable[Dict[str, Any]], arch, device, min_width: int = 1) -> "ReferenceCorpus":
        """One pass over ``loader`` (the images are not touched).  ``min_width``: columns the rows must at least have
        (the evaluator asks for the longest caption it can generate); ``rejected_ids`` count too, so that one width
        serves every row of the evaluation."""
        rows, lens, S, K, bad = [], [], int(min_width), 1, torch.zeros((), dtype=I64, device=device)
        for batch in loader:
            ids, mask, present = batch_references(batch)
            B, k, W = ids.shape
            t_ids, _, t_len = strip_rows(arch, ids.to(device).reshape(B * k, W),
                                         mask.to(device).reshape(B * k, W).sum(1), W)
            t_len = t_len.view(B, k)
            if present is not None:
                absent = ~present.to(device).bool()
                bad += ((t_len < 0) & ~absent).sum()
                t_len = t_len.masked_fill(absent, -1)
            else:
                bad += (t_len < 0).sum()
            rows.append(t_ids.view(B, k, W))
            lens.append(t_len)
            S, K = max(S, W, batch["rejected_ids"].shape[-1] if "rejected_ids" in batch else 0), max(K, k)
        if not rows:
            raise ValueError("the loader gave no batch")
        if S > hip.EVAL_MAX_S or K > hip.EVAL_MAX_K or arch.gpt.base_vocab > hip.EVAL_MAX_VOCAB:
            raise ValueError(f"caption metrics take at most {hip.EVAL_MAX_S} token columns, {hip.EVAL_MAX_K} references "
                             f"per image and a base vocabulary of {hip.EVAL_MAX_VOCAB}; got {S}, {K} and "
                             f"{arch.gpt.base_vocab}")
        pad = arch.gpt.base_vocab
        N = sum(r.shape[0] for r in rows)
        ref_ids = torch.full((N, K, S), pad, dtype=I64, device=device)
        ref_len = torch.full((N, K), -1, dtype=I32, device=device)
        i = 0
        for r, l in zip(rows, lens):
            B, k, W = r.shape
            ref_ids[i:i + B, :k, :W], ref_len[i:i + B, :k] = r, l
            i += B
        return cls(arch, ref_ids, ref_len, bad)

    def rows(self, S: int) -> torch.Tensor:
        """``ref_ids`` at a width of ``S`` >= its own ([PAD] in the new columns; lengths and tables are unchanged)."""
        if S == self.S:
            return self.ref_ids
        if S < self.S:
            raise ValueError(f"the corpus rows are {self.S} columns wide, {S} asked for")
        wide = torch.full((self.N, self.K, S), self.arch.gpt.base_vocab, dtype=I64, device=self.ref_ids.device)
        wide[:, :, :self.S] = self.ref_ids
        return wide


def bleu_from_stats(stats: List[int], order: int) -> float:
    """Corpus BLEU of ``order`` from the ten summed integers of ``pgca_bleu_stats``, as the ``bleu`` metric the reference
    loads defines it: geometric mean of the clipped precisions 1..order (0 if any is 0, no smoothing) times the
    brevity penalty (1 if pred_len / ref_len > 1 else exp(1 - ref_len / pred_len)); 0 when either length is 0."""
    pred_len, ref_len = int(stats[8]), int(stats[9])
    if pred_len == 0 or ref_len == 0:
        return 0.0
    prec = [int(stats[m]) / int(stats[4 + m]) if int(stats[4 + m]) > 0 else 0.0 for m in range(order)]
    if min(prec) <= 0.0:
        return 0.0
    geo = math.exp(sum(math.log(p) for p in prec) / order)
    return geo * (1.0 if pred_len / ref_len > 1.0 else math.exp(1.0 - ref_len / pred_len))


METEOR_ALPHA, METEOR_BETA, METEOR_GAMMA = 0.9, 3.0, 0.5   # HF ``meteor``'s defaults, which the reference takes


def _harmonic(p: float, r: float) -> float:
    return 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0


def rouge_from_stats(stats: List[List[int]]) -> Dict[str, float]:
    """``rouge1`` / ``rouge2`` / ``rougeL`` from the six integers per image of ``pgca_rouge_stats`` (overlap_1, overlap_2,
    lcs, pred_len, ref_len, k_used): per image F = 2PR / (P + R) with P = overlap_n / max(pred_len - n + 1, 1) and
    R = overlap_n / max(ref_len - n + 1, 1), for ROUGE-L P = lcs / pred_len and R = lcs / ref_len (F = 0 when either
    length is 0); then the mean over all images, one with no reference (k_used = -1) counting as 0."""
    f1 = f2 = fl = 0.0
    for o1, o2, lcs, pred_len, ref_len, k_used in ([int(v) for v in row] for row in stats):
        if k_used < 0:
            continue
        f1 += _harmonic(o1 / max(pred_len, 1), o1 / max(ref_len, 1))
        f2 += _harmonic(o2 / max(pred_len - 1, 1), o2 / max(ref_len - 1, 1))
        if pred_len > 0 and ref_len > 0:
            fl += _harmonic(lcs / pred_len, lcs / ref_len)
    n = max(len(stats), 1)
    return {"rouge1": f1 / n, "rouge2": f2 / n, "rougeL": fl / n}


def meteor_from_stats(stats: List[List[List[int]]], pred_len: List[int], ref_len: List[List[int]]) -> float:
    """``meteor`` from the [m, chunks] per reference of ``pgca_meteor_stats`` and the lengths: per reference
    P = m / pred_len, R = m / ref_len, F = PR / (0.9 P + 0.1 R), score = (1 - 0.5 (chunks / m)^3) F (0 when m or a length
    is 0); per image the best present reference (``ref_len`` >= 0); then the mean over all images."""
    total = 0.0
    for rows, plen, rlens in zip(stats, pred_len, ref_len):
        best = 0.0
        for (m, chunks), rlen in zip(rows, rlens):
            m, chunks, plen, rlen = int(m), int(chunks), int(plen), int(rlen)
            if rlen <= 0 or plen <= 0 or m <= 0:
                continue
            p, r = m / plen, m / rlen
            f = p * r / (METEOR_ALPHA * p + (1.0 - METEOR_ALPHA) * r)
            best = max(best, (1.0 - METEOR_GAMMA * (chunks / m) ** METEOR_BETA) * f)
        total += best
    return total / max(len(stats), 1)


def _percentile(sorted_values: List[float], q: float) -> float:
    """numpy's default (linear) percentile of an ascending list."""
    pos = (len(sorted_values) - 1) * q / 100.0
    lo = int(math.floor(pos))
    hi = min(lo + 1, len(sorted_values) - 1)
    return sorted_values[lo] + (sorted_values[hi] - sorted_values[lo]) * (pos - lo)


class CaptionEvaluator:
    """``generate_kwargs``: keywords of ``generate_token_ids``; ``None`` takes ``evaluation.generate_config`` of
    ``config`` when it has that section, else ``generate``'s own defaults.  ``measure_latency``: the reference's
    per-image latency (batch wall time ending in a device synchronise, over the batch size; metrics.py:873-889); with
    ``False`` no synchronise is added and no latency key is returned.

    Result keys - the reference's names where the quantity is the reference's: ``bleu_1`` .. ``bleu_4``, ``cider``
    (mean per-image score x 10), ``rouge1``, ``rouge2``, ``rougeL`` (mean per-image F against the image's first present
    reference, as the reference scores them), ``meteor`` (mean per-image best score over the present references, exact
    matches only) - like BLEU and CIDEr over BPE ids, not comparable with word-level ROUGE / METEOR;
    ``diversity_1``, ``diversity_2``, ``unique_caption_ratio``; with ``rejected_ids`` in the
    batches ``preference_win_rate``, ``avg_preferred_similarity``, ``avg_rejected_similarity``, ``preference_margin``;
    ``alignment_score`` / ``alignment_score_std`` (population std): the cosine of the model's own Stage-1 towers between
    image and generated caption - this project's stand-in for CLIP-Score, not CLIP-Score; ``latency_mean_ms``,
    ``latency_median_ms``, ``latency_p95_ms``, ``latency_p99_ms``; ``num_samples``, ``mean_length``."""

    def __init__(self, model, generate_kwargs: Optional[Dict[str, Any]] = None, measure_latency: bool = True,
                 config=None, sigma: float = CIDER_SIGMA):
        if generate_kwargs is None:
            try:
                generate_kwargs = config_generate_kwargs(config) if config is not None else {}
            except (KeyError, TypeError):
                generate_kwargs = {}
        self.model, self.generate_kwargs = model, dict(generate_kwargs)
        self.measure_latency, self.sigma = bool(measure_latency), float(sigma)
        self.last: Dict[str, torch.Tensor] = {}     # per-image results of the last evaluate(), on the host

    def max_new_tokens(self) -> int:
        """The most tokens ``generate`` can return under ``generate_kwargs`` (the prefix is one of ``max_length``)."""
        kw = self.generate_kwargs
        if kw.get("max_new_tokens") is not None:
            return int(kw["max_new_tokens"])
        return int(kw.get("max_length", 50)) - 1

    def build_corpus(self, loader) -> ReferenceCorpus:
        return ReferenceCorpus.build(loader, self.model.arch, self.model.device, min_width=max(1, self.max_new_tokens()))

    @torch.no_grad()
    def evaluate(self, loader, corpus: Optional[ReferenceCorpus] = None) -> Dict[str, float]:
        m = self.model
        was = m.training
        m.eval()
        try:
            return self._evaluate(loader, corpus)
        finally:
            m.train(was)

    def _evaluate(self, loader, corpus: Optional[ReferenceCorpus]) -> Dict[str, float]:
        m, dev = self.model, self.model.device
        arch = m.arch
        base, P = arch.gpt.base_vocab, arch.proj_dim
        if corpus is None:
            corpus = self.build_corpus(loader)                    # pass one
        N, K = corpus.N, corpus.K
        S = max(corpus.S, self.max_new_tokens())
        if S > hip.EVAL_MAX_S:
            raise ValueError(f"generation may return {S} tokens; caption metrics take at most {hip.EVAL_MAX_S} columns")
        ref_ids, ref_len = corpus.rows(S), corpus.ref_len
        pred_ids = torch.full((N, S), base, dtype=I64, device=dev)
        pred_len = torch.zeros(N, dtype=I32, device=dev)
        score, flag = torch.zeros(N, dtype=F64, device=dev), torch.zeros(N, dtype=I32, device=dev)
        stats = torch.zeros(N, 10, dtype=I64, device=dev)
        rouge = torch.zeros(N, 6, dtype=I32, device=dev)          # overlap_1, overlap_2, lcs, pred_len, ref_len, k_used
        meteor = torch.zeros(N, K, 2, dtype=I32, device=dev)      # per reference: matches, chunks
        over = torch.zeros(2, N, 2, dtype=I32, device=dev)        # [preferred | rejected], image, [both, either]
        side_len = torch.zeros(2, N, dtype=I32, device=dev)
        align = torch.zeros(N, dtype=F32, device=dev)
        bad = corpus.bad_rows.clone()                             # rows with an id no vocabulary holds
        latencies: List[float] = []
        has_pairs, i0 = None, 0
        for batch in loader:                                      # pass two
            images = batch["image"]
            B = images.shape[0]
            if i0 + B > N:
                raise ValueError(f"the loader gave more than the {N} images of the reference corpus")
            if self.measure_latency:
                torch.cuda.synchronize(dev)
                t0 = time.time()
            ids = m.generate_token_ids(images, **self.generate_kwargs)
            if self.measure_latency:
                torch.cuda.synchronize(dev)
                latencies += [(time.time() - t0) / B] * B
            W = ids.shape[1]
            rows = slice(i0, i0 + B)
            # every generated column is handed over: [PAD] after [EOS] is a special and is stripped like [EOS] itself
            t_ids, t_mask, t_len = strip_rows(arch, ids, torch.full((B,), W, dtype=I64, device=dev), S)
            bad += (t_len < 0).sum()
            pred_ids[rows], pred_len[rows] = t_ids, t_len.clamp_min(0)
            hip.cider_rows(pred_ids[rows], pred_len[rows], ref_ids[rows], ref_len[rows], B, K, S, base,
                           corpus.table_keys, corpus.table_df, corpus.table_off, corpus.n_docs, self.sigma, score[rows],
                           flag[rows])
            hip.bleu_stats(pred_ids[rows], pred_len[rows], ref_ids[rows], ref_len[rows], B, K, S, base, stats[rows])
            hip.rouge_stats(pred_ids[rows], pred_len[rows], ref_ids[rows], ref_len[rows], B, K, S, base, rouge[rows])
            hip.meteor_stats(pred_ids[rows], pred_len[rows], ref_ids[rows], ref_len[rows], B, K, S, base, meteor[rows])
            pairs = "rejected_ids" in batch and "preferred_ids" in batch
            if has_pairs is not None and pairs != has_pairs:
                raise ValueError("some batches carry preferred / rejected captions and some do not")
            has_pairs = pairs
            if pairs:
                for side, name in enumerate(("preferred", "rejected")):
                    c_ids, c_mask = batch[name + "_ids"].to(dev), batch[name + "_mask"].to(dev)
                    s_ids, _, s_len = strip_rows(arch, c_ids, c_mask.sum(1), S)
                    bad += (s_len < 0).sum()
                    side_len[side, rows] = s_len.clamp_min(0)
                    hip.token_overlap(pred_ids[rows], pred_len[rows], s_ids, side_len[side, rows], B, S,
                                      over[side, rows])
            # alignment: the Stage-1 towers on the image and on the stripped caption (the scorer of mining.py, n = 1)
            emb = m.vision_encoder(images.to(dev, F32).contiguous())["embeddings"].clone()
            a_ids, a_mask = t_ids[:, :W].contiguous(), t_mask[:, :W].contiguous()
            wrong = (a_ids < 0) | (a_ids >= arch.text_vocab)
            bad += wrong.any(1).sum()
            a_ids.masked_fill_(wrong, base)
            _, _, temb = m.text_encoder.engine.forward(a_ids, a_mask, save=False)
            hip.group_cosine(emb, temb, B, 1, P, align[rows])
            i0 += B
        if i0 != N:
            raise ValueError(f"the loader gave {i0} images, the reference corpus holds {N}")
        # diversity over all predictions: every n-gram key, ordered and counted by torch
        div = []
        keys = torch.empty(N, S, dtype=I64, device=dev)
        for order in (1, 2):
            hip.ngram_keys(pred_ids, pred_len, N, 1, S, order, base, False, keys)
            k = torch.sort(keys.view(-1)).values
            valid = k != -1
            starts = torch.cat([valid[:1], (k[1:] != k[:-1]) & valid[1:]])   # first element of every run of a real key
            div += [starts.sum(), valid.sum()]
        # distinct captions: rows are [PAD] after their length, so one caption has one form; stable sorts from the last
        # column to the first order the rows, and a row that differs from the one before it starts a new caption
        perm = torch.arange(N, device=dev)
        for c in range(S - 1, -1, -1):
            perm = perm[torch.sort(pred_ids[perm, c], stable=True).indices]
        ordered = pred_ids[perm]
        div.append((ordered[1:] != ordered[:-1]).any(1).sum() + 1)
        # the one read-back
        packed = torch.cat([score, flag.to(F64), stats.to(F64).view(-1), over.to(F64).view(-1),
                            side_len.to(F64).view(-1), align.to(F64), pred_len.to(F64),
                            torch.stack(div + [bad]).to(F64), rouge.to(F64).view(-1), meteor.to(F64).view(-1),
                            ref_len.to(F64).view(-1)]).cpu()
        parts = torch.split(packed, [N, N, 10 * N, 4 * N, 2 * N, N, N, 6, 6 * N, 2 * K * N, K * N])
        score_h, flag_h, align_h, len_h = parts[0], parts[1].long(), parts[5], parts[6].long()
        stats_h, over_h, side_h = parts[2].long().view(N, 10), parts[3].long().view(2, N, 2), parts[4].long().view(2, N)
        d1u, d1t, d2u, d2t, unique, n_bad = (int(v) for v in parts[7])
        rouge_h, meteor_h = parts[8].long().view(N, 6), parts[9].long().view(N, K, 2)
        ref_len_h = parts[10].long().view(N, K)
        if n_bad:
            raise ValueError(f"{n_bad} caption rows hold an id outside the decoder's or the text tower's vocabulary")
        if int(flag_h.sum()):
            raise ValueError(f"{int(flag_h.sum())} of {N} images have no reference")
        self.last = {"cider": score_h, "bleu_stats": stats_h, "overlap": over_h, "alignment": align_h, "length": len_h,
                     "pred_ids": pred_ids.cpu(), "rouge_stats": rouge_h, "meteor_stats": meteor_h}
        total = [int(v) for v in stats_h.sum(0)]
        out: Dict[str, float] = {f"bleu_{n}": bleu_from_stats(total, n) for n in range(1, 5)}
        out["cider"] = float(score_h.sum() / N * 10.0)
        out.update(rouge_from_stats(rouge_h.tolist()))
        out["meteor"] = meteor_from_stats(meteor_h.tolist(), len_h.tolist(), ref_len_h.tolist())
        out["diversity_1"] = d1u / d1t if d1t else 0.0
        out["diversity_2"] = d2u / d2t if d2t else 0.0
        out["unique_caption_ratio"] = unique / N
        if has_pairs:
            sims = []
            for side in range(2):
                both, either = over_h[side, :, 0].to(F64), over_h[side, :, 1].to(F64)
                usable = (len_h > 0) & (side_h[side] > 0) & (either > 0)
                sims.append(torch.where(usable, both / either.clamp_min(1.0), torch.zeros_like(both)))
            out["preference_win_rate"] = float((sims[0] > sims[1]).sum()) / N
            out["avg_preferred_similarity"] = float(sims[0].sum() / N)
            out["avg_rejected_similarity"] = float(sims[1].sum() / N)
            out["preference_margin"] = out["avg_preferred_similarity"] - out["avg_rejected_similarity"]
        out["alignment_score"] = float(align_h.mean())
        out["alignment_score_std"] = float(align_h.std(unbiased=False))
        if self.measure_latency:
            lat = sorted(latencies)
            out["latency_mean_ms"] = sum(lat) / len(lat) * 1000.0
            out["latency_median_ms"] = _percentile(lat, 50.0) * 1000.0
            out["latency_p95_ms"] = _percentile(lat, 95.0) * 1000.0
            out["latency_p99_ms"] = _percentile(lat, 99.0) * 1000.0
        out["num_samples"] = N
        out["mean_length"] = float(len_h.sum()) / N
        return out
