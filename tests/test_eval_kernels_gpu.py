"""csrc/eval.hip against the plain-Python restatements of tests/eval_refs.py: keys, document-frequency tables, BLEU
integers and overlap integers exactly, per-image CIDEr within 1e-9 absolute.

The CIDEr bound is derived, not tuned: kernel and restatement evaluate the same float64 formula and differ only in the
order of sums of at most 128 * (K + 1) terms (about 1e-12 on the 0..1 per-image scale) and possibly in the last place
of the device's ``log``.  Measured on an MI355X: see profiles/eval_metrics.json.

Shapes are the smallest at which these kernels can go wrong: one image and several workgroups; one reference and the
most; S below, at and above one 64-lane sweep and at the limit; a 3-id vocabulary (heavy repeats: clipping, document
frequencies equal to the corpus size), 509 and 65535 (leading ids >= 32768: negative order-4 keys)."""
import types

import numpy as np
import pytest
import torch

import eval_refs as E
from pgca_amd import hip
from pgca_amd.evaluation import ReferenceCorpus

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, I64, F64 = torch.int32, torch.int64, torch.float64

# every N of {1, 2, 37}, K of {1, 5, 8}, S of {1, 3, 63, 64, 65, 128} and vocabulary of {3, 509, 65535} occurs
CASES = [(1, 1, 1, 3), (1, 5, 3, 3), (2, 8, 3, 509), (2, 1, 63, 65535), (37, 5, 64, 3), (37, 8, 65, 509),
         (2, 5, 128, 65535), (37, 8, 128, 3), (37, 1, 65, 65535), (1, 8, 64, 509), (2, 5, 63, 3), (37, 5, 1, 3)]


def arch_of(vocab):
    return types.SimpleNamespace(gpt=types.SimpleNamespace(base_vocab=vocab))


def make_case(N, K, S, vocab, seed):
    """Stripped rows ([PAD] = vocab after the length).  References: absent (-1) and empty (0) ones mixed in; image 5
    (when there is one) has no present reference.  Predictions: a reference of the image with a third of its ids
    redrawn, cut to a random length; prediction 0 is empty and prediction 1 shorter than four ids when N allows."""
    rng = np.random.default_rng(seed)
    ref_ids = np.full((N, K, S), vocab, np.int64)
    ref_len = rng.integers(0, S + 1, (N, K)).astype(np.int32)
    kind = rng.random((N, K))
    ref_len[kind < 0.1] = 0
    ref_len[(kind >= 0.1) & (kind < 0.3)] = -1
    if N > 5:
        ref_len[5] = -1
    if N == 1 and (ref_len < 0).all():
        ref_len[0, 0] = S
    pred_ids = np.full((N, S), vocab, np.int64)
    pred_len = rng.integers(0, S + 1, N).astype(np.int32)
    if N > 1:
        pred_len[0] = 0
    if N > 2:
        pred_len[1] = min(S, 3)
    if N == 1:
        pred_len[0] = S
    for i in range(N):
        for k in range(K):
            n = max(int(ref_len[i, k]), 0)
            ref_ids[i, k, :n] = rng.integers(0, vocab, n)
        src = ref_ids[i, rng.integers(0, K)].copy()
        src[src >= vocab] = rng.integers(0, vocab, int((src >= vocab).sum()))
        redraw = rng.random(S) < 1 / 3
        src[redraw] = rng.integers(0, vocab, int(redraw.sum()))
        pred_ids[i, :pred_len[i]] = src[:pred_len[i]]
    return pred_ids, pred_len, ref_ids, ref_len


def as_lists(pred_ids, pred_len, ref_ids, ref_len):
    preds = [pred_ids[i, :pred_len[i]].tolist() for i in range(len(pred_len))]
    refs = [[None if ref_len[i, k] < 0 else ref_ids[i, k, :ref_len[i, k]].tolist() for k in range(ref_len.shape[1])]
            for i in range(len(pred_len))]
    return preds, refs


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def run_cider(corpus, p_ids, p_len, vocab, sigma=6.0):
    N, K, S = corpus.ref_ids.shape
    score = torch.full((N,), -7.0, dtype=F64, device=DEV)
    flag = torch.full((N,), -7, dtype=I32, device=DEV)
    hip.cider_rows(p_ids, p_len, corpus.ref_ids, corpus.ref_len, N, K, S, vocab, corpus.table_keys, corpus.table_df,
                   corpus.table_off, corpus.n_docs, sigma, score, flag)
    return score, flag


@pytest.fixture(scope="module")
def measured():
    worst = {"cider_max_abs_err": 0.0}
    yield worst
    print(f"\ncider_rows against the float64 restatement: max |err| over all cases = {worst['cider_max_abs_err']:.3e}")


@pytest.mark.parametrize("N,K,S,vocab", CASES)
def test_kernels_against_the_restatements(N, K, S, vocab, measured):
    pred_ids, pred_len, ref_ids, ref_len = make_case(N, K, S, vocab, seed=N * 1000 + K * 100 + S + vocab)
    preds, refs = as_lists(pred_ids, pred_len, ref_ids, ref_len)
    p_ids, p_len, r_ids, r_len = dev(pred_ids), dev(pred_len), dev(ref_ids), dev(ref_len)

    # keys of every order, every occurrence and once per image
    negative = False
    for order in (1, 2, 3, 4):
        for distinct in (False, True):
            got = torch.full((N, K, S), 12345, dtype=I64, device=DEV)
            hip.ngram_keys(r_ids, r_len, N, K, S, order, vocab, distinct, got)
            want = np.array(E.ngram_keys(ref_ids.tolist(), ref_len.tolist(), order, S, distinct), np.int64)
            assert np.array_equal(got.cpu().numpy(), want), (order, distinct)
            negative |= bool((want < -1).any())
    if vocab == 65535 and S >= 4:
        assert negative, "the case must hold order-4 keys with a leading id >= 32768"

    # the corpus tables: sorted in signed order, the reference's once-per-image document frequency
    corpus = ReferenceCorpus(arch_of(vocab), r_ids, r_len, torch.zeros((), dtype=I64, device=DEV))
    df = E.doc_freq(refs)
    keys_h, df_h, off = corpus.table_keys.cpu().tolist(), corpus.table_df.cpu().tolist(), corpus.table_off.cpu().tolist()
    for order in (1, 2, 3, 4):
        want = sorted((E.key(g), c) for g, c in df.items() if len(g) == order)
        assert list(zip(keys_h[off[order - 1]:off[order]], df_h[off[order - 1]:off[order]])) == want, order

    # CIDEr per image
    want_score, want_flag = E.cider_rows(preds, refs)
    score, flag = run_cider(corpus, p_ids, p_len, vocab)
    assert flag.cpu().tolist() == want_flag
    err = float(np.abs(score.cpu().numpy() - np.array(want_score)).max())
    print(f"cider_rows N={N} K={K} S={S} vocab={vocab}: max |err| = {err:.3e}")
    measured["cider_max_abs_err"] = max(measured["cider_max_abs_err"], err)
    assert err <= 1e-9
    if N > 5:
        assert want_flag[5] == 1 and float(score[5]) == 0.0
    again, flag2 = run_cider(corpus, p_ids, p_len, vocab)
    assert torch.equal(score.view(I64), again.view(I64)) and torch.equal(flag, flag2)      # bitwise

    # BLEU integers
    stats = torch.full((N, 10), -7, dtype=I64, device=DEV)
    hip.bleu_stats(p_ids, p_len, r_ids, r_len, N, K, S, vocab, stats)
    assert stats.cpu().tolist() == [E.bleu_stats(p, r) for p, r in zip(preds, refs)]

    # overlap integers: the prediction against the image's first reference (an absent one counts as empty)
    b_len = r_len[:, 0].clamp_min(0).contiguous()
    out = torch.full((N, 2), -7, dtype=I32, device=DEV)
    hip.token_overlap(p_ids, p_len, r_ids[:, 0].contiguous(), b_len, N, S, out)
    assert out.cpu().tolist() == [list(E.overlap(p, r[0] or [])) for p, r in zip(preds, refs)]


def test_sigma_and_a_corpus_larger_than_the_batch():
    """A batch is scored against the tables and n_docs of the whole corpus; sigma is honoured."""
    N, K, S, vocab = 9, 3, 12, 6
    pred_ids, pred_len, ref_ids, ref_len = make_case(N, K, S, vocab, seed=77)
    ref_len[5] = 4
    ref_ids[5, :, :4] = 2
    preds, refs = as_lists(pred_ids, pred_len, ref_ids, ref_len)
    corpus = ReferenceCorpus(arch_of(vocab), dev(ref_ids), dev(ref_len), torch.zeros((), dtype=I64, device=DEV))
    want, _ = E.cider_rows(preds, refs, sigma=2.5)
    rows = slice(3, 7)
    score = torch.empty(4, dtype=F64, device=DEV)
    flag = torch.empty(4, dtype=I32, device=DEV)
    hip.cider_rows(dev(pred_ids)[rows], dev(pred_len)[rows], corpus.ref_ids[rows], corpus.ref_len[rows], 4, K, S, vocab,
                   corpus.table_keys, corpus.table_df, corpus.table_off, corpus.n_docs, 2.5, score, flag)
    assert np.abs(score.cpu().numpy() - np.array(want[rows])).max() <= 1e-9 and flag.cpu().tolist() == [0] * 4


def test_identical_three_token_image_scores_7_5_on_the_device():
    """df == n_docs: the idf is about -1e-8 and the float64 cosine over it is 1 for the three orders that exist."""
    ids = torch.tensor([[[5, 6, 7]]], dtype=I64, device=DEV)
    length = torch.tensor([[3]], dtype=I32, device=DEV)
    corpus = ReferenceCorpus(arch_of(509), ids, length, torch.zeros((), dtype=I64, device=DEV))
    score, flag = run_cider(corpus, ids[0].contiguous(), length[0].contiguous(), 509)
    assert abs(float(score[0]) * 10.0 - 7.5) <= 1e-9 and int(flag[0]) == 0


def test_the_fixture_corpora_through_the_kernels(golden):
    """tests/golden/caption_metrics.npz: the reference's own CIDEr, diversity and preference numbers."""
    z = golden("caption_metrics")
    worst = 0.0
    for c in range(len(z["N"])):
        N, K, vocab, S = int(z["N"][c]), int(z["K"][c]), int(z["vocab"][c]), z["pred_ids"].shape[2]
        p_ids, p_len = dev(z["pred_ids"][c, :N]), dev(z["pred_len"][c, :N])
        r_ids, r_len = dev(z["ref_ids"][c, :N, :K]), dev(z["ref_len"][c, :N, :K])
        j_ids, j_len = dev(z["rej_ids"][c, :N]), dev(z["rej_len"][c, :N])
        corpus = ReferenceCorpus(arch_of(vocab), r_ids, r_len, torch.zeros((), dtype=I64, device=DEV))
        score, flag = run_cider(corpus, p_ids, p_len, vocab)
        assert int(flag.sum()) == 0
        worst = max(worst, abs(float(score.sum()) / N * 10.0 - float(z["cider"][c])))
        # diversity: distinct over total keys of all predictions
        for order, want in ((1, z["diversity"][c, 0]), (2, z["diversity"][c, 1])):
            keys = torch.empty(N, 1, S, dtype=I64, device=DEV)
            hip.ngram_keys(p_ids, p_len, N, 1, S, order, vocab, False, keys)
            k = keys[keys != -1].cpu().tolist()
            assert (len(set(k)) / len(k) if k else 0.0) == float(want)
        # preference: preferred = the first reference
        sims = []
        for b_ids, b_len in ((r_ids[:, 0].contiguous(), r_len[:, 0].contiguous()), (j_ids, j_len)):
            out = torch.empty(N, 2, dtype=I32, device=DEV)
            hip.token_overlap(p_ids, p_len, b_ids, b_len, N, S, out)
            sims.append([b / e if pl > 0 and bl > 0 and e > 0 else 0.0
                         for (b, e), pl, bl in zip(out.cpu().tolist(), p_len.cpu().tolist(), b_len.cpu().tolist())])
        assert sum(1 for p, r in zip(*sims) if p > r) / N == float(z["preference"][c, 0])
        assert abs(sum(sims[0]) / N - float(z["preference"][c, 1])) <= 1e-12
        assert abs(sum(sims[1]) / N - float(z["preference"][c, 2])) <= 1e-12
    print(f"fixture corpora through cider_rows: max |cider - reference| = {worst:.3e}")
    assert worst <= 1e-9 * 10.0     # the per-image bound on the x10 scale of the corpus value
