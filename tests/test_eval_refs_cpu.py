"""The restatements of tests/eval_refs.py against the reference's own outputs (tests/golden/caption_metrics.npz, recorded
by tools/make_eval_golden.py), BLEU against hand-worked cases, and the configuration surface of the evaluation."""
import math
import os

import pytest
import yaml

import eval_refs as E
from pgca_amd import evaluation  # noqa: F401  (the feature under test: absent before it)
from pgca_amd.evaluation import CaptionEvaluator, bleu_from_stats

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def corpora(golden):
    """[(preds, refs, rejected, recorded)] of the fixture, as id lists."""
    z = golden("caption_metrics")
    out = []
    for c in range(len(z["N"])):
        N, K = int(z["N"][c]), int(z["K"][c])
        preds = [z["pred_ids"][c, i, :z["pred_len"][c, i]].tolist() for i in range(N)]
        rej = [z["rej_ids"][c, i, :z["rej_len"][c, i]].tolist() for i in range(N)]
        refs = [[z["ref_ids"][c, i, k, :z["ref_len"][c, i, k]].tolist() for k in range(K)] for i in range(N)]
        out.append((preds, refs, rej, {"cider": float(z["cider"][c]), "diversity": z["diversity"][c].tolist(),
                                       "preference": z["preference"][c].tolist(), "vocab": int(z["vocab"][c])}))
    return out


def test_fixture_covers_the_edge_cases(golden):
    cs = corpora(golden)
    assert len(cs) >= 60 and os.path.getsize(os.path.join(GOLDEN, "caption_metrics.npz")) < 100 * 1024
    assert {len(p) for p, _, _, _ in cs} == set(range(1, 9)) and {len(r[0]) for _, r, _, _ in cs} == {1, 2, 3, 4}
    assert {w["vocab"] for *_, w in cs} == {3, 6, 40}
    assert any(len(p) == 1 for p, *_ in cs)
    assert any(len(x) == 0 for p, *_ in cs for x in p) and any(0 < len(x) < 4 for p, *_ in cs for x in p)
    assert any(len(x) == 0 for _, r, _, _ in cs for refs in r for x in refs)


def test_cider_restatement_equals_the_reference(golden):
    worst = 0.0
    for preds, refs, _, want in corpora(golden):
        worst = max(worst, abs(E.cider(preds, refs) - want["cider"]))
    print(f"cider restatement: max |diff| = {worst:.3e}")
    assert worst <= 1e-12


def test_diversity_and_preference_restatements_equal_the_reference(golden):
    for preds, refs, rej, want in corpora(golden):
        d = E.diversity(preds)
        assert [d["diversity_1"], d["diversity_2"], d["unique_caption_ratio"]] == want["diversity"]   # integer ratios
        p = E.preference(preds, [r[0] for r in refs], rej)
        assert p["preference_win_rate"] == want["preference"][0]
        for name, w in zip(("avg_preferred_similarity", "avg_rejected_similarity", "preference_margin"),
                           want["preference"][1:]):
            assert abs(p[name] - w) <= 1e-12, name


def test_identical_three_token_image_scores_7_5():
    """df == n_docs: idf = log(1 / (1 + 1e-8)) is about -1e-8, not 0, and the cosine over those weights is 1 for the
    orders that exist (1, 2, 3 of 4): 0.75 x 10."""
    assert abs(E.cider([[5, 6, 7]], [[[5, 6, 7]]]) - 7.5) <= 1e-12


# ------------------------------------------------------------------------------------------ BLEU, worked by hand
THE, CAT, IS, ON, MAT, SAT = 1, 2, 3, 4, 5, 6


def both(preds, refs):
    """The restatement's and the package's value of bleu_1..4 (they must agree exactly)."""
    total = [0] * 10
    for p, r in zip(preds, refs):
        total = [a + b for a, b in zip(total, E.bleu_stats(p, r))]
    got = [bleu_from_stats(total, n) for n in range(1, 5)]
    assert got == [E.bleu(total, n) for n in range(1, 5)] == list(E.corpus_bleu(preds, refs).values())
    return total, got


def test_bleu_identical_is_one():
    total, got = both([[THE, CAT, IS, ON, THE, MAT]], [[[THE, CAT, IS, ON, THE, MAT]]])
    assert total == [6, 5, 4, 3, 6, 5, 4, 3, 6, 6]
    assert all(abs(b - 1.0) <= 1e-15 for b in got)


def test_bleu_clipping():
    """Seven times "the" against "the cat is on the mat": the count is clipped at the reference's two."""
    total, got = both([[THE] * 7], [[[THE, CAT, IS, ON, THE, MAT]]])
    assert total[:4] == [2, 0, 0, 0] and total[4:8] == [7, 6, 5, 4] and total[8:] == [7, 6]
    assert got[0] == 2 / 7 and got[1:] == [0.0, 0.0, 0.0]
    # the maximum over references, not the sum: two references with two and one "the"
    assert E.bleu_stats([THE] * 7, [[THE, CAT, THE], [THE, MAT], None])[0] == 2


def test_bleu_prediction_shorter_than_the_order():
    total, got = both([[THE, CAT]], [[[THE, CAT, SAT]]])
    assert total == [2, 1, 0, 0, 2, 1, 0, 0, 2, 3]
    bp = math.exp(1 - 3 / 2)
    assert abs(got[0] - bp) <= 1e-15 and abs(got[1] - bp) <= 1e-15 and got[2:] == [0.0, 0.0]


def test_bleu_brevity_penalty_on_both_sides_of_one():
    ref = [THE, CAT, IS, ON]
    assert both([ref + [MAT]], [[ref]])[1][0] == 4 / 5                        # longer: ratio 1.25, bp 1
    assert both([ref], [[ref]])[1][0] == math.exp(0.0)                        # ratio exactly 1 is NOT > 1: exp(1 - 1)
    assert abs(both([ref[:3]], [[ref]])[1][0] - math.exp(1 - 4 / 3)) <= 1e-15  # shorter
    # the reference length is the shortest present reference
    assert E.bleu_stats(ref, [ref + [MAT, MAT], ref[:2], None])[9] == 2


def test_bleu_zero_lengths_are_zero():
    assert both([[]], [[[THE, CAT]]])[1] == [0.0] * 4
    assert both([[THE, CAT]], [[[]]])[1] == [0.0] * 4
    assert bleu_from_stats([0] * 10, 1) == 0.0


def test_overlap_and_keys():
    assert E.overlap([1, 1, 2, 3], [3, 3, 4]) == (1, 4) and E.similarity([], [1]) == 0.0
    assert E.key((1,)) == 1 and E.key((1, 2)) == (1 << 16) | 2
    assert E.key((32768, 0, 0, 0)) == -(1 << 63) and E.key((65534, 65534, 65534, 65534)) < -1
    keys = E.ngram_keys([[[7, 7, 7, 9], [7, 9, 0, 0]]], [[4, 2]], 1, 4, True)
    assert keys == [[[7, -1, -1, 9], [-1, -1, -1, -1]]]


# ------------------------------------------------------------------------------------------ configuration
def test_evaluation_defaults_and_off_by_default():
    from pgca_amd.config import MI355X_DEFAULTS, Config, select_evaluation
    assert MI355X_DEFAULTS["evaluation"] == {"every_epochs": 0, "max_batches": None}
    cfg = Config()
    assert cfg.get("mi355x.evaluation.every_epochs") == 0 and cfg.get("mi355x.evaluation.max_batches") is None
    assert select_evaluation(cfg) is None and select_evaluation({}) is None
    assert select_evaluation({"mi355x": {"evaluation": {"every_epochs": 0, "max_batches": 3}}}) is None
    cfg.set("mi355x.evaluation", {"every_epochs": 2})
    assert select_evaluation(cfg) == {"every_epochs": 2, "max_batches": None}
    with pytest.raises(ValueError, match="mi355x.evaluation"):
        select_evaluation({"mi355x": {"evaluation": {"every": 1}}})


def test_the_references_generate_config_reaches_the_evaluator():
    with open(os.path.join(GOLDEN, "reference_default.yaml"), "r", encoding="utf-8") as f:
        ref_cfg = yaml.safe_load(f)
    section = ref_cfg["evaluation"]["generate_config"]
    ev = CaptionEvaluator(model=None, config=ref_cfg)
    assert ev.generate_kwargs == section and ev.max_new_tokens() == section["max_length"] - 1
    assert {k: type(v) for k, v in ev.generate_kwargs.items()} == {k: type(v) for k, v in section.items()}
    # an explicit dict wins; no section and no dict: generate's own defaults
    assert CaptionEvaluator(None, {"num_beams": 1}, config=ref_cfg).generate_kwargs == {"num_beams": 1}
    assert CaptionEvaluator(None, config={"model": {}}).generate_kwargs == {}
    assert CaptionEvaluator(None).max_new_tokens() == 49 and CaptionEvaluator(None).measure_latency is True
