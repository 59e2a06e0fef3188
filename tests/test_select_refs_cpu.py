"""The float64 references of ``test_select_gpu.py`` (tests/select_refs.py) against what is already pinned: the oracle's
processors (themselves pinned to transformers' classes), a direct ``torch.topk`` threshold, and the dropout-mask hash."""
import torch

import row_kernel_refs as K
import select_refs as S
from oracle import restatement as R


def test_processors_equal_the_oracle_on_the_product_tests_inputs():
    """Same inputs as test_generation_gpu.test_product_score_processing_matches_the_oracle."""
    gen = torch.Generator().manual_seed(21)
    scores = torch.randn(6, 509, generator=gen) * 3
    ids = torch.randint(0, 509, (6, 7), generator=gen)
    got = S.process(scores, ids, 1.3, True, 0.7, 0, 0.8)
    want = R.process_scores(scores.clone(), ids, 1.3, True, 0.7, 0.8)
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    keep = ~torch.isinf(want)
    assert torch.allclose(got[keep], want[keep].double(), atol=1e-5)
    lp = torch.log_softmax(scores, dim=-1)
    got = S.process(lp, ids, 1.2, False)
    assert torch.allclose(got, R.process_scores(lp.clone(), ids, 1.2).double(), atol=1e-6)


def test_penalty_acts_once_per_distinct_id():
    s = torch.tensor([[2.0, -2.0, 1.0, -1.0]])
    prev = torch.tensor([[0, 1, 0, 1, 1]])
    got = S.process(s, prev, 2.0, False)
    assert torch.equal(got, torch.tensor([[1.0, -4.0, 1.0, -1.0]], dtype=torch.float64))


def test_top_k_rule_equals_a_topk_threshold():
    gen = torch.Generator().manual_seed(3)
    s = (torch.randn(5, 300, generator=gen) * 3).double()
    s[0, 10] = s[0, 20] = s[0].topk(4)[0][-1]          # ties with the k-th stay
    for k in (1, 4, 50, 299):
        kth = torch.topk(s, k, dim=-1)[0][:, -1:]
        assert torch.equal(S.top_k_filter(s, k), s.masked_fill(s < kth, float("-inf"))), k
    assert int((~torch.isinf(S.top_k_filter(s, 4)[0])).sum()) == 6
    assert torch.equal(S.top_k_filter(s, 0), s) and torch.equal(S.top_k_filter(s, 300), s)
    assert torch.equal(S.top_k_filter(s, 305), s)


def test_top_p_keeps_or_removes_equal_scores_together():
    s = torch.log(torch.tensor([[0.05, 0.05, 0.1, 0.1, 0.7]], dtype=torch.float64))
    assert S.top_p_removed(s, 0.85)[0].tolist() == [[True, True, False, False, False]]   # 0.1 class straddles 0.15
    assert S.top_p_removed(s, 0.95)[0].tolist() == [[False, False, False, False, False]]  # 0.05 class straddles 0.05
    assert S.top_p_removed(s, 1e-6)[0].tolist() == [[True, True, True, True, False]]


def test_hash32_equals_the_dropout_mask_function():
    idx = torch.tensor([0, 1, 2, 3, 77, 50259, 2 ** 31 + 5, 2 ** 32 - 1], dtype=torch.int64)
    for seed, p in ((0, 0.1), (12345, 0.5), (0xDEADBEEF, 0.25)):
        h = S.hash32(((idx >> 1) * 0x9E3779B1 + seed) & 0xFFFFFFFF)
        bits = torch.where((idx & 1) == 1, h >> 16, h & 0xFFFF)
        keep = bits >= (int(p * 4294967296.0) >> 16)
        scale = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
        assert torch.equal(keep.double() * scale, K.drop_mult_at(seed, p, idx)), seed
    g = S.gumbel(torch.arange(1000), 7)
    assert bool(torch.isfinite(g).all()) and -2.9 < float(g.min()) and float(g.max()) < 17.4
