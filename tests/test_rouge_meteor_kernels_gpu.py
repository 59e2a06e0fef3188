"""``pgca_rouge_stats`` and ``pgca_meteor_stats`` against the plain-Python restatements of tests/rouge_meteor_refs.py:
every integer exactly, every output slot written, two launches bitwise equal.

The random cases are the grid and the input recipe of tests/test_eval_kernels_gpu.py (absent and empty references mixed
in, one image with no present reference, an empty prediction, a short one; S below, at and above one 64-lane word and at
the limit; a 3-id vocabulary for heavy repeats).  The crafted rows aim at what the grid may miss: the carry from word 0
into word 1 of the LCS recurrence, matches that cross the two words, and the last-to-first matching order."""
import numpy as np
import pytest
import torch

import rouge_meteor_refs as R
from pgca_amd import hip
from test_eval_kernels_gpu import CASES, as_lists, dev, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32
SENTINEL = -7


def run_both(pred_ids, pred_len, ref_ids, ref_len, vocab):
    """Both kernels twice on numpy rows -> (rouge [N, 6], meteor [N, K, 2]) as lists; asserts that no slot keeps the
    sentinel's place unwritten and that the second launch is bitwise the first."""
    N, K, S = ref_ids.shape
    p_ids, p_len, r_ids, r_len = dev(pred_ids), dev(pred_len), dev(ref_ids), dev(ref_len)
    outs = []
    for _ in range(2):
        rouge = torch.full((N, 6), SENTINEL, dtype=I32, device=DEV)
        meteor = torch.full((N, K, 2), SENTINEL, dtype=I32, device=DEV)
        hip.rouge_stats(p_ids, p_len, r_ids, r_len, N, K, S, vocab, rouge)
        hip.meteor_stats(p_ids, p_len, r_ids, r_len, N, K, S, vocab, meteor)
        outs.append((rouge.cpu(), meteor.cpu()))
    (rouge, meteor), (rouge2, meteor2) = outs
    assert torch.equal(rouge, rouge2) and torch.equal(meteor, meteor2)
    assert not (rouge == SENTINEL).any() and not (meteor == SENTINEL).any()
    return rouge.tolist(), meteor.tolist()


@pytest.mark.parametrize("N,K,S,vocab", CASES)
def test_kernels_against_the_restatements(N, K, S, vocab):
    pred_ids, pred_len, ref_ids, ref_len = make_case(N, K, S, vocab, seed=N * 1000 + K * 100 + S + vocab)
    preds, refs = as_lists(pred_ids, pred_len, ref_ids, ref_len)
    rouge, meteor = run_both(pred_ids, pred_len, ref_ids, ref_len, vocab)
    assert rouge == [R.rouge_stats(p, r) for p, r in zip(preds, refs)]
    assert meteor == [R.meteor_stats(p, r) for p, r in zip(preds, refs)]
    if N > 5:
        assert rouge[5] == [0, 0, 0, 0, 0, -1] and meteor[5] == [[-1, -1]] * K     # no present reference
    if N > 1:
        assert rouge[0][:4] == [0, 0, 0, 0] and all(m in ([0, 0], [-1, -1]) for m in meteor[0])   # empty prediction


def crafted_rows():
    """(prediction, [reference 0, reference 1]) per image, S = 128, ids below 509."""
    rng = np.random.default_rng(128)
    long_row = rng.integers(0, 509, 128).tolist()
    few = rng.integers(0, 4, 128).tolist()
    run = list(range(100, 140))                               # 40 distinct ids, used nowhere else in their rows
    return [
        (long_row, [list(long_row), long_row[::-1]]),         # identical at the limit: lcs 128, one chunk
        ([7] * 128, [[7] * 65, [7] * 128]),                   # one repeated id: every step carries
        ([7] * 65, [[7] * 128, [7] * 64]),
        ([1] * 64 + run, [run + [2] * 64, None]),             # common part in columns >= 64 of one row, < 64 of the other
        (run + [1] * 50, [[2] * 64 + run, []]),
        (few[::-1], [list(few), few[::-1]]),                  # the prediction reversed, many repeats
        (long_row[::-1], [list(long_row), None]),             # ... and nearly distinct ids
        (few[:70], [None, few[10:90]]),                       # the first reference absent, the second present
        ([1, 2], [[1, 2, 1], [1, 2]]),                        # the hand-worked matching order
        ([3] * 64 + [4], [[4] + [3] * 64, [3] * 63 + [4, 3]]),   # matches that cross the word boundary
    ]


def test_crafted_rows_carry_and_matching_order():
    rows = crafted_rows()
    N, K, S, vocab = len(rows), 2, 128, 509
    pred_ids, ref_ids = np.full((N, S), vocab, np.int64), np.full((N, K, S), vocab, np.int64)
    pred_len, ref_len = np.zeros(N, np.int32), np.full((N, K), -1, np.int32)
    for i, (p, refs) in enumerate(rows):
        pred_ids[i, :len(p)], pred_len[i] = p, len(p)
        for k, r in enumerate(refs):
            if r is not None:
                ref_ids[i, k, :len(r)], ref_len[i, k] = r, len(r)
    preds, refs = [p for p, _ in rows], [r for _, r in rows]
    rouge, meteor = run_both(pred_ids, pred_len, ref_ids, ref_len, vocab)
    assert rouge == [R.rouge_stats(p, r) for p, r in zip(preds, refs)]
    assert meteor == [R.meteor_stats(p, r) for p, r in zip(preds, refs)]
    # what the rows were made for, spelled out
    assert rouge[0] == [128, 127, 128, 128, 128, 0] and meteor[0][0] == [128, 1]
    assert rouge[1] == [65, 64, 65, 128, 65, 0] and meteor[1] == [[65, 1], [128, 1]]
    assert rouge[2] == [65, 64, 65, 65, 128, 0] and meteor[2] == [[65, 1], [64, 1]]
    assert rouge[3] == [40, 39, 40, 104, 104, 0] and meteor[3] == [[40, 1], [-1, -1]]
    assert rouge[4] == [40, 39, 40, 90, 104, 0] and meteor[4] == [[40, 1], [0, 0]]
    assert rouge[7][5] == 1 and rouge[7][3:5] == [70, 80] and meteor[7][0] == [-1, -1]
    assert meteor[8] == [[2, 2], [2, 1]]
    assert rouge[9][:3] == [65, 63, 64]
