"""Preference mining without a GPU: the restated pairing rule against what the reference's
``_process_scored_captions`` emitted (tests/golden/pair_mining.npz, tools/make_mining_golden.py), the config surface of
the ``mine_then_dpo`` objective, and the host-side argument checks of the four entries of csrc/mine.hip."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (loads libamdhip64 first, as the product does)

import mining_refs as M
from pgca_amd import REPO_ROOT, hip


def test_restatement_reproduces_the_reference_pairs(golden):
    g = golden("pair_mining")
    C = len(g["n"])
    assert C >= 200 and set(g["family"].tolist()) == {0, 1} and set(g["n"].tolist()) == set(range(1, 9))
    assert int(g["count"].sum()) > C and (g["count"] == 0).any()
    for c in range(C):
        n, k = int(g["n"][c]), int(g["count"][c])
        rank, win, lose, margin = M.pair_image(g["scores"][c, :n], g["threshold"][c])
        assert win == g["win"][c, :k].tolist() and lose == g["lose"][c, :k].tolist(), c
        assert sorted(rank.tolist()) == list(range(n))
        for w, l, d in zip(win, lose, margin):
            assert rank[l] == rank[w] + 1 and d == np.float32(g["scores"][c, w] - g["scores"][c, l])


def test_counting_rank_is_the_stable_descending_sort():
    """The kernel ranks by counting: #{i : s_i > s_j or (s_i == s_j and i < j)}; the restatement sorts as the reference
    does.  Same order, ties included."""
    rng = np.random.default_rng(3)
    for _ in range(500):
        n = int(rng.integers(1, 65))
        s = (rng.integers(-4, 5, n) / 4.0).astype(np.float32)
        counted = [int(sum(s[i] > s[j] or (s[i] == s[j] and i < j) for i in range(n))) for j in range(n)]
        assert counted == M.pair_image(s, 0.0)[0].tolist()


def test_filters_and_best_worst_rule():
    S = 6
    ids = np.full((5, S), 9, np.int64)
    ids[0, :3], ids[1, :3], ids[2, :3], ids[3, :1], ids[4, :4] = [1, 2, 3], [1, 2, 3], [1, 2, 4], [5], [1, 2, 3, 9]
    lens = np.array([3, 3, 3, 1, 4], np.int32)
    s = np.array([[0.5, 0.9, np.nan, 0.7, 0.25]], np.float32)
    rank, pw, pl, pm, cnt = M.mine_pairs(s, ids, lens, None, 2, "adjacent", 0.0)
    # 1 repeats 0, 2 is NaN, 3 is too short: 0 and 4 remain
    assert rank.tolist() == [[0, -1, -1, -1, 1]] and cnt.tolist() == [1]
    assert (pw[0, 0], pl[0, 0], pm[0, 0]) == (0, 4, np.float32(0.25)) and pw[0, 1:].tolist() == [-1] * 4
    s2 = np.array([[0.5, 0.0, 0.25, 1.0, 0.75]], np.float32)
    ok = np.array([[1, 1, 1, 1, 0]], np.uint8)
    rank, pw, pl, pm, cnt = M.mine_pairs(s2, ids, lens, ok, 1, "best_worst", 0.5)
    assert rank.tolist() == [[1, -1, 2, 0, -1]] and cnt.tolist() == [1] and (pw[0, 0], pl[0, 0]) == (3, 2)
    assert M.mine_pairs(s2, ids, lens, ok, 1, "best_worst", 0.8)[4].tolist() == [0]


def test_id_conversion_restatement():
    base, dec_vocab = 509, 512
    cand = np.array([[3, 510, 7, 509, 511, 2, 2], [4, 5, 512, 6, 511, 0, 0]], np.int64)
    r = M.candidate_rows(cand, [5, 5], 5, base, dec_vocab, base, base)
    assert r["dec_ids"][0].tolist() == [3, 510, 7, 509, 511] and r["text_ids"][0].tolist() == [3, 7, 509, 509, 509]
    assert (r["text_len"].tolist(), r["out_len"].tolist()) == ([2, -1], [5, 0])
    assert r["dec_mask"][1].sum() == 0 and (r["dec_ids"][1] == base).all() and r["text_mask"][1].sum() == 0


def test_mine_then_dpo_is_a_known_objective_and_the_reference_config_still_selects_dpo():
    import yaml
    from pgca_amd.config import MI355X_DEFAULTS, STAGE2_OBJECTIVES, Config, select_objective
    assert "mine_then_dpo" in STAGE2_OBJECTIVES
    assert select_objective({"mi355x": {"stage2": {"objective": "mine_then_dpo"}}}) == "mine_then_dpo"
    with open(os.path.join(REPO_ROOT, "tests", "golden", "reference_default.yaml"), "r", encoding="utf-8") as f:
        assert select_objective(yaml.safe_load(f)) == "dpo"
    cfg = Config(os.path.join(REPO_ROOT, "tests", "golden", "reference_default.yaml"))
    assert select_objective(cfg) == "dpo"
    assert MI355X_DEFAULTS["mining"] == {
        "num_candidates": 4, "rule": "adjacent", "threshold": 0.0, "scorer": "alignment", "max_length": 50,
        "min_tokens": 2, "temperature": 1.0, "top_p": 0.9, "top_k": 0, "repetition_penalty": 1.1,
        "no_repeat_ngram_size": 0, "decode_rows": 64, "seed": None}
    assert cfg.get("mi355x.mining.num_candidates") == 4 and cfg.get("mi355x.mining.seed") is None
    cfg.set("mi355x.stage2.objective", "mine_then_dpo")
    assert select_objective(cfg) == "mine_then_dpo"


def test_miner_defaults_are_the_config_defaults():
    import inspect
    from pgca_amd.config import MI355X_DEFAULTS
    from pgca_amd.mining import PreferenceMiner
    sig = inspect.signature(PreferenceMiner.__init__).parameters
    defaults = {k: p.default for k, p in sig.items() if k not in ("self", "model")}
    assert defaults == {k: v for k, v in MI355X_DEFAULTS["mining"].items() if k != "seed"}
    with pytest.raises(ValueError, match="num_candidates"):
        PreferenceMiner(None, num_candidates=65)
    with pytest.raises(ValueError, match="rule"):
        PreferenceMiner(None, rule="all_pairs")


def test_mined_data_keeps_each_image_once_and_cuts_to_a_batch_count():
    """``MinedPreferenceData`` needs no device: two mined batches (5 + 3 pairs over 2 + 2 images), then loaders."""
    from pgca_amd.mining import BATCH_KEYS, MinedPreferenceData
    S = 4

    def mined(pair_image, first_id):
        k = len(pair_image)
        ids = torch.arange(first_id, first_id + k)[:, None].repeat(1, S)
        return {"preferred_ids": ids, "preferred_mask": torch.ones(k, S, dtype=torch.int64), "rejected_ids": ids + 100,
                "rejected_mask": torch.ones(k, S, dtype=torch.int64), "preference_score": torch.full((k,), 0.5),
                "pair_image": torch.tensor(pair_image, dtype=torch.int32), "n_pairs": k,
                "rank": torch.tensor([[0, 1, 2, -1], [0, -1, 1, 2]], dtype=torch.int32),
                "source_images": torch.full((2, 3, 2, 2), float(first_id)) + torch.arange(2.0)[:, None, None, None]}

    data = MinedPreferenceData()
    assert len(data) == 0 and len(data.loader(2)) == 0 and list(data.loader(2)) == []
    data.add(mined([0, 0, 1, 1, 1], 0))
    data.add(mined([1, 0, 0], 10))
    assert len(data) == 8 and data.stats == {"images": 4, "candidates": 16, "left_out": 4, "pairs": 8}
    assert data._tables()["image"].shape[0] == 4                      # every image once, not once per pair
    batches = list(data.loader(3, shuffle=False, drop_last=True))
    assert len(batches) == 2 and set(batches[0]) == set(BATCH_KEYS) | {"image"}
    assert torch.cat([b["preferred_ids"][:, 0] for b in batches]).tolist() == [0, 1, 2, 3, 4, 10]
    # pair -> image: the second batch's images come after the first's two
    assert torch.cat([b["image"][:, 0, 0, 0] for b in batches]).tolist() == [0.0, 0.0, 1.0, 1.0, 1.0, 11.0]
    assert len(list(data.loader(3, drop_last=False))) == 3 and len(data.loader(3, drop_last=False, max_batches=2)) == 2
    a, b = data.loader(2, shuffle=True, seed=5, max_batches=3), data.loader(2, shuffle=True, seed=5, max_batches=3)
    first = [x["preferred_ids"][:, 0].tolist() for x in a]
    assert len(first) == 3 and first == [x["preferred_ids"][:, 0].tolist() for x in b]       # the seed decides the order
    assert first != [x["preferred_ids"][:, 0].tolist() for x in a]                           # a new order every pass


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        from pgca_amd import build
        build.build()
    return hip.load()


def _refused(lib, entry, args, naming):
    assert getattr(lib, entry)(*args, None) == -1, (entry, naming)
    msg = lib.pgca_last_error().decode()
    assert entry in msg and naming in msg, msg


def test_host_side_validation_of_the_mining_entries(lib):
    """Bad arguments are refused before any launch (so this runs without a GPU), with the entry and the argument named.
    A non-null pointer is any address: nothing is dereferenced on the host."""
    p = 4096
    rows = [p, 7, p, 6, 8, 509, 512, 509, 509, p, p, p, p, p, p]
    _refused(lib, "pgca_candidate_rows", [None] + rows[1:], "cand")
    _refused(lib, "pgca_candidate_rows", rows[:9] + [p, p, None, p, p, p], "text_ids")
    _refused(lib, "pgca_candidate_rows", [p, 0] + rows[2:], "ld_cand")
    _refused(lib, "pgca_candidate_rows", rows[:3] + [0] + rows[4:], "R > 0")
    _refused(lib, "pgca_candidate_rows", rows[:5] + [509, 508] + rows[7:], "dec_vocab")
    cos = [p, p, 3, 5, 64, p]
    _refused(lib, "pgca_group_cosine", [p, None] + cos[2:], "txt")
    _refused(lib, "pgca_group_cosine", cos[:3] + [0] + cos[4:], "n > 0")
    _refused(lib, "pgca_group_cosine", cos[:4] + [0, p], "P >= 1")
    mine = [p, p, p, None, 2, 4, 8, 2, 0, 0.0, p, p, p, p, p]
    _refused(lib, "pgca_mine_pairs", [None] + mine[1:], "score")
    _refused(lib, "pgca_mine_pairs", mine[:14] + [None], "pair_count")
    for n in (0, 65):
        _refused(lib, "pgca_mine_pairs", mine[:5] + [n] + mine[6:], "n <= 64")
    _refused(lib, "pgca_mine_pairs", mine[:8] + [2] + mine[9:], "rule")
    _refused(lib, "pgca_mine_pairs", mine[:9] + [float("nan")] + mine[10:], "threshold")
    pair = [p, p, p, p, p, p, 4, 4, 8, 12, 509, p, p, p, p, p, p, p]
    _refused(lib, "pgca_pair_rows", pair[:3] + [None] + pair[4:], "pair_count")
    _refused(lib, "pgca_pair_rows", pair[:17] + [None], "n_pairs")
    _refused(lib, "pgca_pair_rows", pair[:9] + [11] + pair[10:], "cap")
    for n in (0, 65):
        _refused(lib, "pgca_pair_rows", pair[:7] + [n] + pair[8:], "n <= 64")
    assert lib.pgca_version() == hip.ABI_VERSION == 306
    assert {"pgca_candidate_rows", "pgca_group_cosine", "pgca_mine_pairs", "pgca_pair_rows"} <= set(hip.EXPORTS)
