"""The four entries of csrc/mine.hip against their restatements (tests/mining_refs.py): exact, except the cosine,
whose bound is the f32 summation error.  Every entry is also launched twice on one input: the outputs are bitwise equal."""
import numpy as np
import pytest
import torch

import mining_refs as M
from pgca_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BASE, DEC_VOCAB = 509, 512
PAD, BOS, EOS = BASE, BASE + 1, BASE + 2


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV).contiguous()


def run_candidate_rows(cand, lengths, S):
    R = cand.shape[0]
    o = dict(dec_ids=torch.empty(R, S, dtype=torch.int64, device=DEV), dec_mask=torch.empty(R, S, dtype=torch.int64, device=DEV),
             text_ids=torch.empty(R, S, dtype=torch.int64, device=DEV), text_mask=torch.empty(R, S, dtype=torch.int32, device=DEV),
             text_len=torch.empty(R, dtype=torch.int32, device=DEV), out_len=torch.empty(R, dtype=torch.int32, device=DEV))
    for t in o.values():
        t.fill_(-7)
    hip.candidate_rows(cand, lengths, R, S, BASE, DEC_VOCAB, PAD, PAD, o["dec_ids"], o["dec_mask"], o["text_ids"],
                       o["text_mask"], o["text_len"], o["out_len"])
    return o


def run_mine_pairs(scores, dec_ids, out_len, ok, min_tokens, rule, threshold):
    B, n = scores.shape
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)   # noqa: E731
    rank, pw, pl, cnt = i32(B, n), i32(B, n), i32(B, n), i32(B)
    pm = torch.full((B, n), -7.0, dtype=torch.float32, device=DEV)
    hip.mine_pairs(scores, dec_ids, out_len, ok, B, n, dec_ids.shape[1], min_tokens, rule, threshold, rank, pw, pl, pm, cnt)
    return rank, pw, pl, pm, cnt


def run_pair_rows(pw, pl, pm, cnt, dec_ids, dec_mask, cap):
    B, n = pw.shape
    S = dec_ids.shape[1]
    o = {k: torch.full((cap, S), -7, dtype=torch.int64, device=DEV)
         for k in ("preferred_ids", "preferred_mask", "rejected_ids", "rejected_mask")}
    o["pair_image"] = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    o["preference_score"] = torch.full((cap,), -7.0, dtype=torch.float32, device=DEV)
    o["n_pairs"] = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    hip.pair_rows(pw, pl, pm, cnt, dec_ids, dec_mask, B, n, S, cap, PAD, o["preferred_ids"], o["preferred_mask"],
                  o["rejected_ids"], o["rejected_mask"], o["pair_image"], o["preference_score"], o["n_pairs"])
    return o


def same(got, want):
    for k, w in want.items():
        g = got[k].cpu().numpy()
        assert g.dtype == np.asarray(w).dtype and np.array_equal(g.reshape(np.shape(w)), w), k


# ------------------------------------------------------------------------------------------ candidate_rows
CAND = np.array([                            # R = 6, ld_cand = 7
    [11, 22, 33, 44, 55, 66, 77],            # no [EOS], full length
    [EOS, PAD, PAD, PAD, PAD, PAD, PAD],     # [EOS] first
    [BOS, PAD, BOS, EOS, PAD, PAD, PAD],     # only specials
    [5, BOS, 6, PAD, 7, EOS, PAD],           # [BOS] in the middle, a live [PAD] before [EOS]
    [1, 2, DEC_VOCAB, 3, EOS, PAD, PAD],     # an id equal to dec_vocab: unusable
    [12, 13, 14, 15, 16, 17, 18],            # length 0
], np.int64)
LENGTHS = np.array([7, 1, 4, 6, 5, 0], np.int64)


@pytest.mark.parametrize("S", [8, 5])
def test_candidate_rows(S):
    got = run_candidate_rows(dev(CAND), dev(LENGTHS), S)
    want = M.candidate_rows(CAND, LENGTHS, S, BASE, DEC_VOCAB, PAD, PAD)
    same(got, want)
    assert want["out_len"].tolist() == [min(7, S), 1, 4, min(6, S), 0, 0]
    assert want["text_len"].tolist() == [min(7, S), 0, 0, 3, -1, 0]
    assert want["text_ids"][3].tolist()[:4] == [5, 6, 7, PAD] and want["dec_ids"][3, 1] == BOS
    assert int(got["text_ids"].max()) <= BASE          # the decoder's [BOS] / [EOS] never reach the text tower
    again = run_candidate_rows(dev(CAND), dev(LENGTHS), S)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_candidate_rows_bad_ids_count_only_inside_the_length():
    cand = np.array([[-1, 2, 3, EOS, PAD, PAD, PAD],          # a negative id: unusable
                     [1, 2, EOS, DEC_VOCAB, -5, PAD, PAD],    # bad ids past the length: usable
                     [9, PAD, 10, EOS, 1 << 40, PAD, PAD],    # an id that does not fit 32 bits, past the length
                     [1 << 40, 2, EOS, PAD, PAD, PAD, PAD],   # ... and inside it: unusable
                     [3, 4, 5, EOS, PAD, PAD, PAD]], np.int64)   # a negative length counts as 0
    lengths = np.array([4, 3, 4, 3, -2], np.int64)
    got = run_candidate_rows(dev(cand), dev(lengths), 6)
    want = M.candidate_rows(cand, lengths, 6, BASE, DEC_VOCAB, PAD, PAD)
    same(got, want)
    assert want["text_len"].tolist() == [-1, 2, 2, -1, 0] and want["out_len"].tolist() == [0, 3, 4, 0, 0]


def test_candidate_rows_wider_than_a_wave_and_a_strided_source():
    """S > 64 (two ballot rounds per row), more rows than one workgroup holds, rows read at a stride > S."""
    rng = np.random.default_rng(5)
    R, ld, S = 11, 150, 130
    cand = rng.integers(0, DEC_VOCAB, (R, ld))
    lengths = rng.integers(0, 160, R)
    lengths[0], lengths[1] = 130, 64
    got = run_candidate_rows(dev(cand), dev(lengths), S)
    same(got, M.candidate_rows(cand, lengths, S, BASE, DEC_VOCAB, PAD, PAD))


# ------------------------------------------------------------------------------------------ group_cosine
@pytest.mark.parametrize("B,n,P", [(3, 5, 64), (2, 64, 520), (1, 1, 1)])
def test_group_cosine(B, n, P):
    g = torch.Generator().manual_seed(B * 1000 + P)
    img, txt = torch.randn(B, P, generator=g) * 3.0, torch.randn(B * n, P, generator=g) * 0.5
    if P > 1:
        txt[1].zero_()                                  # a zero vector: the clamp, score exactly 0
        txt[2] = img[0] * 0.25                          # parallel: score 1
    score = torch.full((B * n,), -7.0, device=DEV)
    hip.group_cosine(img.to(DEV), txt.to(DEV), B, n, P, score)
    want = M.group_cosine(img.numpy(), txt.numpy(), n)
    err = np.abs(score.cpu().numpy().astype(np.float64) - want).max()
    bound = 4 * P * 2.0 ** -24          # f32 summation error of P terms on quantities of magnitude <= 1, with room
    print(f"group_cosine B={B} n={n} P={P}: max |err| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if P > 1:
        assert float(score[1]) == 0.0 and abs(float(score[2]) - 1.0) <= bound
    again = torch.empty_like(score)
    hip.group_cosine(img.to(DEV), txt.to(DEV), B, n, P, again)
    assert torch.equal(score, again)


def test_group_cosine_all_zero():
    score = torch.full((4,), -7.0, device=DEV)
    hip.group_cosine(torch.zeros(2, 8, device=DEV), torch.zeros(4, 8, device=DEV), 2, 2, 8, score)
    assert score.tolist() == [0.0] * 4


# ------------------------------------------------------------------------------------------ mine_pairs
def mining_case(n, seed):
    """B = 5 images of n candidates, S = 9: dyadic scores with ties; image 1 all-equal scores; a NaN, a +inf, ok zeros,
    duplicates (a three-way one when n allows), a too-short candidate; image 4 has every candidate left out."""
    rng = np.random.default_rng(seed)
    B, S = 5, 9
    scores = (rng.integers(-8, 9, (B, n)) / 8.0).astype(np.float32)
    scores[1] = 0.375
    lens = rng.integers(2, S + 1, (B, n)).astype(np.int32)
    ids = rng.integers(0, BASE, (B, n, S))
    ok = np.ones((B, n), np.uint8)
    if n >= 2:
        scores[0, n - 1] = np.nan
        ok[2, 0] = 0
        lens[3, 1] = 1                                            # too short
    if n >= 5:
        scores[0, 1] = np.inf
        scores[2, 3] = -np.inf
        for j in (2, 4):                                          # 0, 2 and 4 of image 3 are the same caption
            ids[3, j], lens[3, j] = ids[3, 0], lens[3, 0]
        ids[2, 2, :lens[2, 1]], lens[2, 2] = ids[2, 1, :lens[2, 1]], lens[2, 1]     # 2 repeats 1
        ids[0, 3], lens[0, 3] = ids[0, 2], max(2, lens[0, 2] - 1)                      # a prefix is not a duplicate
        lens[0, 2] = max(3, lens[0, 2])
    if n >= 33:
        scores[1, 20] = 0.5
        ids[1, 32], lens[1, 32] = ids[1, 7], lens[1, 7]
    ok[4, ::2] = 0
    scores[4, 1::2] = np.nan
    mask = (np.arange(S)[None, None] < lens[..., None])
    ids = np.where(mask, ids, PAD)
    return scores, ids.reshape(B * n, S).astype(np.int64), lens.reshape(-1), ok


@pytest.mark.parametrize("n", [1, 2, 5, 33, 64])
def test_mine_pairs(n):
    scores, ids, lens, ok = mining_case(n, 100 + n)
    d = dev(scores), dev(ids), dev(lens), dev(ok)
    first = None
    for rule in M.RULES:
        for threshold in (0.0, 0.25, 0.5):
            got = run_mine_pairs(*d, 2, rule, threshold)
            want = M.mine_pairs(scores, ids, lens, ok, 2, rule, threshold)
            for g, w, name in zip(got, want, ("rank", "pair_win", "pair_lose", "pair_margin", "pair_count")):
                assert np.array_equal(g.cpu().numpy(), w), (name, rule, threshold)
            assert want[4][4] == 0 and (want[0][4] == -1).all()        # the image with nobody left
            first = first or (got, (rule, threshold))
    if n >= 5:
        rank = M.mine_pairs(scores, ids, lens, ok, 2, "adjacent", 0.0)[0]
        assert rank[3, 2] == -1 and rank[3, 4] == -1 and rank[2, 2] == -1 and rank[0, 3] >= 0 and rank[0, 1] == -1
    again = run_mine_pairs(*d, 2, *first[1])
    assert all(torch.equal(a, b) for a, b in zip(first[0], again))
    # without the ok mask and with min_tokens 0: only the scores and the duplicates decide
    got = run_mine_pairs(d[0], d[1], d[2], None, 0, "adjacent", 0.0)
    want = M.mine_pairs(scores, ids, lens, None, 0, "adjacent", 0.0)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_mine_pairs_replays_the_reference_fixture(golden):
    """Every recorded case of the reference's rule, one launch per (n, threshold): winners and losers index for index."""
    g = golden("pair_mining")
    S = 4
    for n in range(1, 9):
        for threshold in sorted(set(g["threshold"][g["n"] == n].tolist())):
            sel = np.nonzero((g["n"] == n) & (g["threshold"] == threshold))[0]
            B = len(sel)
            scores = g["scores"][sel, :n]
            ids = np.tile(np.arange(B * n)[:, None] % BASE, (1, S)).astype(np.int64)       # all captions distinct
            lens = np.full(B * n, S, np.int32)
            rank, pw, pl, pm, cnt = (t.cpu().numpy() for t in run_mine_pairs(dev(scores), dev(ids), dev(lens), None, 2,
                                                                             "adjacent", float(threshold)))
            assert np.array_equal(cnt, g["count"][sel])
            for i, c in enumerate(sel):
                k = int(cnt[i])
                assert pw[i, :k].tolist() == g["win"][c, :k].tolist() and pl[i, :k].tolist() == g["lose"][c, :k].tolist()
                assert (pw[i, k:] == -1).all() and (pl[i, k:] == -1).all() and (pm[i, k:] == 0).all()


# ------------------------------------------------------------------------------------------ pair_rows
@pytest.mark.parametrize("cap", [12, 19])
def test_pair_rows(cap):
    rng = np.random.default_rng(9)
    B, n, S = 4, 4, 7
    lens = rng.integers(2, S + 1, B * n)
    dec_mask = (np.arange(S)[None] < lens[:, None]).astype(np.int64)
    dec_ids = np.where(dec_mask == 1, rng.integers(0, BASE, (B * n, S)), PAD).astype(np.int64)
    cnt = np.array([0, 3, 0, 1], np.int32)
    pw, pl = np.full((B, n), -1, np.int32), np.full((B, n), -1, np.int32)
    pm = np.zeros((B, n), np.float32)
    pw[1, :3], pl[1, :3], pm[1, :3] = [2, 0, 3], [0, 3, 1], [0.5, 0.25, 0.125]
    pw[3, :1], pl[3, :1], pm[3, :1] = [1], [2], [1.5]
    d = [dev(x) for x in (pw, pl, pm, cnt, dec_ids, dec_mask)]
    got = run_pair_rows(*d, cap)
    want = M.pair_rows(pw, pl, pm, cnt, dec_ids, dec_mask, cap, PAD)
    assert int(got["n_pairs"]) == want.pop("n_pairs") == 4
    same(got, want)
    assert got["pair_image"].tolist() == [1, 1, 1, 3] + [-1] * (cap - 4)
    assert (got["preferred_ids"][4:] == PAD).all() and (got["rejected_mask"][4:] == 0).all()
    again = run_pair_rows(*d, cap)
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_pair_rows_many_images_and_no_pairs():
    """More images than a wave has lanes (the prefix sum strides), then a batch without a single pair."""
    rng = np.random.default_rng(11)
    B, n, S = 70, 3, 5
    dec_mask = np.ones((B * n, S), np.int64)
    dec_ids = rng.integers(0, BASE, (B * n, S)).astype(np.int64)
    scores = (rng.integers(-4, 5, (B, n)) / 4.0).astype(np.float32)
    lens = np.full(B * n, S, np.int32)
    rank, pw, pl, pm, cnt = M.mine_pairs(scores, dec_ids, lens, None, 2, "adjacent", 0.25)
    cap = B * (n - 1)
    got = run_pair_rows(*[dev(x) for x in (pw, pl, pm, cnt, dec_ids, dec_mask)], cap)
    want = M.pair_rows(pw, pl, pm, cnt, dec_ids, dec_mask, cap, PAD)
    assert 0 < want["n_pairs"] < cap and int(got["n_pairs"]) == want.pop("n_pairs")
    same(got, want)
    cnt0 = np.zeros(B, np.int32)
    got = run_pair_rows(*[dev(x) for x in (pw, pl, pm, cnt0, dec_ids, dec_mask)], cap)
    assert int(got["n_pairs"]) == 0 and (got["pair_image"] == -1).all() and (got["preferred_mask"] == 0).all()
