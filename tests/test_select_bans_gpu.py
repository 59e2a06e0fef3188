"""The ``_ex`` selection entries (csrc/select.hip: pgca_select_token_ex, pgca_select_beam_candidates_ex) against the
restatement of tests/beam_refs.py, which test_beam_refs_cpu.py pins to transformers' own processors: the n-gram ban,
the ban list (suppress_tokens, [EOS] under a minimum length), with and without the repetition penalty, for greedy,
sampling and beam candidates with and without noise.

As in test_select_gpu.py only DECISIVE inputs are compared (rows are redrawn while a cumulative mass lies within 1e-5
of a threshold, a beam case while two of its first K + 1 keys are closer than 1e-4); chosen tokens and candidate
indices must then be equal, log-probabilities within that file's 1e-4 and candidate scores within its 4 x torch's own
float32 error + 1e-6."""
import ctypes

import pytest
import torch

import beam_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-5
# a history in which the last n - 1 ids occur twice before (followed by 3 and by 4) and once more at the very end
HISTORY = [1, 2, 3, 1, 2, 4, 0, 1, 2]
# (n_ban, penalty, sample): every value of each meets every n_prev over the parametrised cases
COMBOS = [(0, 1.3, False), (1, 1.0, True), (5, 1.3, True), (5, 1.0, False), (1, 1.3, False), (0, 1.0, True)]


def _pad4(x):
    R_, V = x.shape
    buf = torch.full((R_, (V + 3) // 4 * 4), float("nan"))
    buf[:, :V] = x
    return buf.to(DEV)[:, :V]


def _ban_list(n_ban, V):
    return {0: [], 1: [2], 5: [0, 3, V + 3, -1, 5]}[n_ban]      # two of the five lie outside [0, V)


def _prev(Rows, n_prev, V, gen):
    prev = torch.randint(0, min(V, 5), (Rows, max(n_prev, 1)), generator=gen)[:, :n_prev]
    if n_prev == 9:
        prev[0] = torch.tensor(HISTORY)
    return prev


def _dev_ban(ids):
    return torch.tensor(ids, dtype=torch.int64, device=DEV) if ids else None


def _logits(Rows, V, gen):
    x = torch.randn(Rows, V, generator=gen) * (6.0 if V > 10000 else 3.0)
    x[:, :min(V, 6)] += 25.0 if V > 10000 else 4.0               # the ids histories and ban lists name are likely picks
    return x


def run_token(logits, prev, pen, T, top_k, top_p, u, n, ids):
    from pgca_amd import hip
    Rows, V = logits.shape
    nxt = torch.full((Rows,), -7, dtype=torch.int64, device=DEV)
    nlp = torch.full((Rows,), float("nan"), device=DEV)
    hip.select_token(_pad4(logits), V, Rows, prev.to(DEV), prev.shape[1], pen, T, top_k, top_p,
                     None if u is None else u.to(DEV), None, V + 1, nxt, nlp, n, _dev_ban(ids))
    return nxt.cpu(), nlp.cpu()


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("Rows", [1, 33])
@pytest.mark.parametrize("V", [7, 509, 50260])
def test_token_with_bans_equals_the_reference(V, Rows, n):
    gen = torch.Generator().manual_seed(V * 13 + Rows * 7 + n)
    n_prevs = sorted({0, max(n - 2, 0), n - 1, 9})
    changed = 0
    for i, n_prev in enumerate(n_prevs):
        for n_ban, pen, sample in (COMBOS[(2 * i + n) % 6], COMBOS[(2 * i + n + 1) % 6]):
            ids = _ban_list(n_ban, V)
            prev = _prev(Rows, n_prev, V, gen)
            logits = _logits(Rows, V, gen)
            u = torch.rand(Rows, generator=gen).clamp_(1e-6, 1 - 1e-6) if sample else None
            args = (prev, pen, 0.7, 50, 0.9)
            redrawn = 0
            for _ in range(4):
                want, want_lp, margin = R.select_token(logits, *args, u, None, V + 1, n, ids)
                bad = (margin < MARGIN).nonzero()[:, 0].tolist()
                if not bad:
                    break
                redrawn += len(bad)
                for r in bad:
                    logits[r] = _logits(1, V, gen)[0]
                    u[r] = float(torch.rand(1, generator=gen).clamp_(1e-6, 1 - 1e-6))
            assert not bad and redrawn <= max(1, 0.05 * Rows), f"{redrawn} of {Rows} rows redrawn: pick another seed"
            nxt, nlp = run_token(logits, *args, u, n, ids)
            where = (V, Rows, n, n_prev, n_ban, pen, sample)
            assert torch.equal(nxt, want), (where, (nxt != want).nonzero()[:, 0].tolist())
            assert float((nlp.double() - want_lp).abs().max()) <= 1e-4, where
            banned = R.ban_mask(prev, V, n, ids)
            assert not bool(banned.gather(1, nxt[:, None]).any()), where
            changed += int((R.select_token(logits, *args, u, None, V + 1)[0] != want).sum())
    assert changed > 0 or Rows == 1                              # the bans did decide some of these rows


def test_one_rows_history_does_not_ban_in_the_next_row():
    V = 509
    x = torch.zeros(2, V)
    x[0, 5], x[0, 9] = 3.0, 2.0
    x[1, 5], x[1, 9] = 3.0, 2.0
    prev = torch.tensor([[5, 7], [9, 7]])                        # n = 1: row 0 loses id 5, row 1 loses id 9
    nxt, _ = run_token(x, prev, 1.0, 1.0, 0, 1.0, None, 1, [])
    assert nxt.tolist() == [9, 5]
    prev = torch.tensor([[7, 5, 7], [5, 9, 7]])                  # n = 2: after 7 came 5 in row 0 only
    nxt, _ = run_token(x, prev, 1.0, 1.0, 0, 1.0, None, 2, [])
    assert nxt.tolist() == [9, 5]


def test_a_row_with_every_token_banned_yields_the_lowest_id():
    from pgca_amd import hip
    V = 7
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(3, V, generator=gen)
    prev = torch.randint(0, V, (3, 4), generator=gen)
    everything = list(range(V))
    lp = torch.log_softmax(x.double(), dim=-1)
    for u in (None, torch.tensor([0.3, 0.6, 0.9])):
        for pen in (1.0, 1.3):
            nxt, nlp = run_token(x, prev, pen, 0.7, 3, 0.9, u, 2, everything)
            assert nxt.tolist() == [0, 0, 0]
            assert float((nlp.double() - lp[:, 0]).abs().max()) <= 1e-4
    B, nb, K = 1, 3, 6
    score = torch.full((B, K), float("nan"), device=DEV)
    index = torch.full((B, K), -7, dtype=torch.int64, device=DEV)
    for noise in (0, 1):
        hip.select_beam_candidates(_pad4(x), V, B, nb, prev.to(DEV), 4, 1.3, noise, 0.7, 3, 0.9,
                                   torch.zeros(3, device=DEV), K, noise, 99, score, index, 2, _dev_ban(everything))
        assert bool((score == float("-inf")).all()) and index[0].tolist() == list(range(K))


# ------------------------------------------------------------------------------------------------ beam candidates
def run_beam(logits, B, nb, prev, pen, warp, T, top_k, top_p, bs, K, noise, seed, n, ids):
    from pgca_amd import hip
    V = logits.shape[1]
    score = torch.full((B, K), float("nan"), device=DEV)
    index = torch.full((B, K), -7, dtype=torch.int64, device=DEV)
    hip.select_beam_candidates(_pad4(logits), V, B, nb, prev.to(DEV), prev.shape[1], pen, warp, T, top_k, top_p,
                               bs.to(DEV), K, noise, seed, score, index, n, _dev_ban(ids))
    return score.cpu(), index.cpu()


def _torch_chain(logits, B, prev, pen, warp, T, top_k, top_p, bs, index, n, ids):
    """The torch path of _beam_search in float32 on the GPU, at the reference's candidates."""
    from pgca_amd.model import CaptionDecoder
    lp = torch.log_softmax(logits.to(DEV), dim=-1)
    lp = CaptionDecoder._process_scores(lp, prev.to(DEV), pen, warp, T, top_p, top_k, n, _dev_ban(ids))
    acc = (lp + bs.to(DEV)[:, None]).view(B, -1)
    return torch.gather(acc, 1, index.to(DEV)).cpu()


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [7, 509, 50260])
def test_beam_candidates_with_bans_equal_the_reference(V, B, nb, n):
    gen = torch.Generator().manual_seed(V * 11 + B * 5 + nb * 3 + n)
    K = 2 * nb
    n_prevs = sorted({0, max(n - 2, 0), n - 1, 9})
    for i, n_prev in enumerate(n_prevs):
        n_ban, pen, noise = COMBOS[(i + n + nb) % 6]
        noise = int(noise)
        ids = _ban_list(n_ban, V)
        for attempt in range(4):
            prev = _prev(B * nb, n_prev, V, gen)
            logits = _logits(B * nb, V, gen)
            bs = -torch.rand(B * nb, generator=gen) * 4
            args = (B, nb, prev, pen, bool(noise), 0.7, 50, 0.9, bs, K, noise, 4321 + n_prev)
            score, index, keys = R.beam_candidates(logits, *args, n, ids)
            gaps = keys[:, :-1] - keys[:, 1:]
            if not bool((gaps[torch.isfinite(gaps)] <= 1e-4).any()):
                break
        else:
            raise AssertionError("no decisive beam case found: pick another seed")
        got_score, got_index = run_beam(logits, *args, n, ids)
        where = (V, B, nb, n, n_prev, n_ban, pen, noise)
        assert torch.equal(got_index, index), where
        fin = torch.isfinite(score)
        assert torch.equal(torch.isfinite(got_score), fin) and bool((got_score[~fin] == float("-inf")).all()), where
        banned = R.ban_mask(prev, V, n, ids).view(B, nb * V)
        assert not bool(banned.gather(1, index)[fin].any()), where
        if bool(fin.any()):
            ours = float((got_score.double() - score)[fin].abs().max())
            t32 = _torch_chain(logits, B, prev, pen, bool(noise), 0.7, 50, 0.9, bs, index, n, ids)
            torchs = float((t32.double() - score)[fin].abs().max())
            print(f"cand_score {where}: kernel max err {ours:.3e}, torch f32 chain max err {torchs:.3e}")
            assert ours <= 4 * torchs + 1e-6, (where, ours, torchs)


# ------------------------------------------------------------------------------------------------ the old entries
def test_empty_options_equal_the_old_entry_points_bit_for_bit():
    from pgca_amd import hip
    lib = hip.load()
    V, Rows, B, nb, K = 50260, 8, 2, 4, 8
    gen = torch.Generator().manual_seed(77)
    logits = _pad4(torch.randn(Rows, V, generator=gen) * 6)
    prev = torch.randint(0, V, (Rows, 6), generator=gen).to(DEV)
    u = torch.rand(Rows, generator=gen).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for uu in (None, u):
        old = (torch.empty(Rows, dtype=torch.int64, device=DEV), torch.empty(Rows, device=DEV))
        new = (torch.empty(Rows, dtype=torch.int64, device=DEV), torch.empty(Rows, device=DEV))
        rc = lib.pgca_select_token(logits.data_ptr(), logits.stride(0), V, Rows, prev.data_ptr(), prev.stride(0), 6, 1.2,
                                   0.8, 40, 0.9, None if uu is None else uu.data_ptr(), None, V + 1, old[0].data_ptr(),
                                   old[1].data_ptr(), stream)
        assert rc == 0
        hip.select_token(logits, V, Rows, prev, 6, 1.2, 0.8, 40, 0.9, uu, None, V + 1, *new)
        assert torch.equal(old[0], new[0]) and torch.equal(old[1].view(torch.int32), new[1].view(torch.int32))
    bs = (-torch.rand(Rows, generator=gen)).to(DEV)
    for noise in (0, 1):
        old = (torch.empty(B, K, device=DEV), torch.empty(B, K, dtype=torch.int64, device=DEV))
        new = (torch.empty(B, K, device=DEV), torch.empty(B, K, dtype=torch.int64, device=DEV))
        rc = lib.pgca_select_beam_candidates(logits.data_ptr(), logits.stride(0), V, B, nb, prev.data_ptr(),
                                             prev.stride(0), 6, 1.2, noise, 0.8, 40, 0.9, bs.data_ptr(), K, noise,
                                             ctypes.c_uint32(11), old[0].data_ptr(), old[1].data_ptr(), stream)
        assert rc == 0
        hip.select_beam_candidates(logits, V, B, nb, prev, 6, 1.2, noise, 0.8, 40, 0.9, bs, K, noise, 11, *new)
        assert torch.equal(old[1], new[1]) and torch.equal(old[0].view(torch.int32), new[0].view(torch.int32))


def test_the_lds_limit_is_an_error_not_a_launch():
    from pgca_amd import hip
    V, nb = 50260, 8                                             # two planes x 8 rows x 6.3 KB > 60 KiB
    logits = torch.zeros(nb, (V + 3) // 4 * 4, device=DEV)[:, :V]
    prev = torch.zeros(nb, 4, dtype=torch.int64, device=DEV)
    score = torch.full((1, 2 * nb), 7.0, device=DEV)
    index = torch.full((1, 2 * nb), -7, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="61440"):
        hip.select_beam_candidates(logits, V, 1, nb, prev, 4, 1.1, 0, 1.0, 0, 1.0, torch.zeros(nb, device=DEV), 2 * nb,
                                   0, 0, score, index, 2, None)
    torch.cuda.synchronize()
    assert bool((score == 7.0).all()) and bool((index == -7).all())
    # one plane of each kind for the shipped default (4 beams, vocabulary 50 260) fits
    hip.select_beam_candidates(logits[:4], V, 1, 4, prev[:4], 4, 1.1, 0, 1.0, 0, 1.0, torch.zeros(4, device=DEV), 8, 0, 0,
                               score[:, :8].contiguous(), index[:, :8].contiguous(), 2, None)
    Vbig = 300000                                                # token kernel: two planes of 37.5 KB
    big = torch.zeros(1, Vbig, device=DEV)
    nxt = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="61440"):
        hip.select_token(big, Vbig, 1, prev[:1], 4, 1.1, 1.0, 0, 1.0, None, None, 0, nxt, torch.zeros(1, device=DEV), 1)
    torch.cuda.synchronize()
    assert int(nxt[0]) == -7
