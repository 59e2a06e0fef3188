"""The restatements of tests/rouge_meteor_refs.py on hand-worked values and properties, and the product's host formulas
(``rouge_from_stats`` / ``meteor_from_stats``) against them: the same float64 formula on the same integers, so they agree
to a few roundings (1e-15 relative)."""
import random

import pytest

import rouge_meteor_refs as R
from pgca_amd.evaluation import meteor_from_stats, rouge_from_stats

LENGTHS = (0, 1, 2, 3, 7, 20)


def close(a, b):
    return abs(a - b) <= 1e-15 * max(abs(a), abs(b))


def random_corpus(seed, n=40, K=3, vocab=5):
    """Predictions and references over a small vocabulary (many repeats); absent and empty references mixed in, image 3
    without its first reference, image 4 without any, prediction 0 empty."""
    rng = random.Random(seed)
    preds, refs = [], []
    for i in range(n):
        preds.append([rng.randrange(vocab) for _ in range(rng.choice(LENGTHS))])
        rows = []
        for k in range(K):
            u = rng.random()
            rows.append(None if u < 0.2 else [] if u < 0.3 else
                        [rng.randrange(vocab) for _ in range(rng.choice(LENGTHS))])
        refs.append(rows)
    preds[0] = []
    refs[3] = [None, [1, 2, 3, 1], [2, 2]]
    refs[4] = [None] * K
    return preds, refs


def test_the_hand_worked_meteor_values():
    six = [11, 12, 13, 14, 15, 16]
    assert R.meteor_stats(six, [six]) == [[6, 1]]
    assert close(R.meteor_single(six, six), 1.0 - 0.5 / 216.0) and round(R.meteor_single(six, six), 4) == 0.9977
    # last-to-first matching: a first-to-first rule would pair (0, 0), (1, 1) and count one chunk
    assert R.meteor_matches([1, 2], [1, 2, 1]) == [(0, 2), (1, 1)]
    assert R.meteor_stats([1, 2], [[1, 2, 1]]) == [[2, 2]]
    assert close(R.meteor_single([1, 2], [1, 2, 1]), 0.5 * (2.0 / 3.0) / (0.9 + 0.1 * 2.0 / 3.0))
    assert abs(R.meteor_single([1, 2], [1, 2, 1]) - 0.344827) < 1e-6


def test_the_hand_worked_rouge_values():
    pred, ref = [1, 2, 3, 4], [1, 3, 4, 5, 6]
    assert R.rouge_stats(pred, [ref]) == [3, 1, 3, 4, 5, 0]
    assert close(R.rouge_l(pred, ref), 2.0 / 3.0)
    assert close(R.rouge_n(pred, ref, 2), 2.0 * (1 / 3) * (1 / 4) / (1 / 3 + 1 / 4))
    assert close(R.rouge_n(pred, ref, 1), 2.0 * (3 / 4) * (3 / 5) / (3 / 4 + 3 / 5))


@pytest.mark.parametrize("n", [1, 2, 5, 64, 128])
def test_identical_rows(n):
    """F = 1 for every ROUGE that has an n-gram to count, and one chunk: METEOR = 1 - 0.5 (1 / n)^3 (the issue's table:
    1 - 0.5 / 216 at n = 6), with repeated ids as with distinct ones."""
    for row in (list(range(n)), [i % 3 for i in range(n)]):
        assert R.rouge_n(row, row, 1) == 1.0 and R.rouge_l(row, row) == 1.0
        assert R.rouge_n(row, row, 2) == (1.0 if n >= 2 else 0.0)
        assert R.meteor_stats(row, [row]) == [[n, 1]]
        assert close(R.meteor_single(row, row), 1.0 - 0.5 / n ** 3)


def test_disjoint_rows_score_zero():
    a, b = [1, 2, 3, 1], [4, 5, 6, 7, 4]
    assert R.rouge_stats(a, [b]) == [0, 0, 0, 4, 5, 0] and R.meteor_stats(a, [b]) == [[0, 0]]
    assert R.rouge(([a]), [[b]]) == {"rouge1": 0.0, "rouge2": 0.0, "rougeL": 0.0} and R.meteor([a], [[b]]) == 0.0


def test_empty_and_absent_rows():
    ref = [1, 2, 3]
    assert R.rouge_stats([], [ref]) == [0, 0, 0, 0, 3, 0] and R.rouge_stats(ref, [[]]) == [0, 0, 0, 3, 0, 0]
    for pred, refs in (([], [ref]), (ref, [[]])):
        assert R.rouge([pred], [refs]) == {"rouge1": 0.0, "rouge2": 0.0, "rougeL": 0.0}
        assert R.meteor([pred], [refs]) == 0.0
    # the first reference absent: ROUGE takes the second, METEOR the best of the present ones
    assert R.rouge_stats(ref, [None, ref, [9]]) == [3, 2, 3, 3, 3, 1]
    assert R.meteor_stats(ref, [None, ref, [9]]) == [[-1, -1], [3, 1], [0, 0]]
    assert R.rouge([ref], [[None, ref, [9]]])["rougeL"] == 1.0
    assert close(R.meteor([ref], [[None, ref, [9]]]), 1.0 - 0.5 / 27.0)
    # no reference at all: zeros, k_used -1, and the image still counts in the mean
    assert R.rouge_stats(ref, [None, None]) == [0, 0, 0, 0, 0, -1] and R.meteor_stats(ref, [None]) == [[-1, -1]]
    assert R.rouge([ref, ref], [[None], [ref]])["rouge1"] == 0.5
    assert close(R.meteor([ref, ref], [[None], [ref]]), 0.5 * (1.0 - 0.5 / 27.0))


def test_lcs_is_symmetric_and_the_match_counts_are_bounded():
    rng = random.Random(7)
    for _ in range(300):
        a = [rng.randrange(4) for _ in range(rng.choice(LENGTHS))]
        b = [rng.randrange(4) for _ in range(rng.choice(LENGTHS))]
        assert R.lcs(a, b) == R.lcs(b, a) <= min(len(a), len(b))
        assert R.overlap(a, b, 1) >= R.lcs(a, b)            # a common subsequence is a common bag
        (m, chunks), = R.meteor_stats(a, [b])
        assert 0 <= m <= min(len(a), len(b)) and m == R.overlap(a, b, 1)
        assert (1 <= chunks <= m) if m else chunks == 0
        assert 0.0 <= R.meteor_single(a, b) <= 1.0 and 0.0 <= R.rouge_l(a, b) <= 1.0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_host_formulas_equal_the_restatement(seed):
    preds, refs = random_corpus(seed)
    got = rouge_from_stats([R.rouge_stats(p, r) for p, r in zip(preds, refs)])
    want = R.rouge(preds, refs)
    assert set(got) == {"rouge1", "rouge2", "rougeL"}
    for name in want:
        assert close(got[name], want[name]), (name, got[name], want[name])
    ref_len = [[-1 if r is None else len(r) for r in rows] for rows in refs]
    got_m = meteor_from_stats([R.meteor_stats(p, r) for p, r in zip(preds, refs)], [len(p) for p in preds], ref_len)
    assert close(got_m, R.meteor(preds, refs)), (got_m, R.meteor(preds, refs))
    assert 0.0 < got_m < 1.0 and 0.0 < got["rouge2"] < got["rouge1"] < 1.0


def test_the_host_formulas_on_the_hand_worked_integers():
    assert close(rouge_from_stats([[3, 1, 3, 4, 5, 0]])["rougeL"], 2.0 / 3.0)
    assert close(rouge_from_stats([[3, 1, 3, 4, 5, 0], [0, 0, 0, 0, 0, -1]])["rouge2"], 0.5 * (2.0 / 7.0))
    assert close(meteor_from_stats([[[6, 1]]], [6], [[6]]), 1.0 - 0.5 / 216.0)
    assert close(meteor_from_stats([[[-1, -1], [2, 2]]], [2], [[-1, 3]]), 0.5 * (2.0 / 3.0) / (0.9 + 0.1 * 2.0 / 3.0))
    assert meteor_from_stats([[[0, 0]], [[-1, -1]]], [0, 4], [[3], [-1]]) == 0.0
