"""``pgca_beam_step`` (csrc/beam.hip) against the restated step of tests/beam_refs.py, which test_beam_refs_cpu.py pins
to transformers' ``generate``, on constructed candidates.

Every case is a whole scenario: the kernel and the restatement start from HF's initial state and take the same
candidates step after step up to ``cur + 1 == L``, so each step's input is the previous step's output and the two
sequence buffers of the kernel change roles every step.  Integer state and flags must be equal, scores equal to 1e-6
relative.  Only slots whose score is above -1e8 are compared: the rest is HF's additively masked garbage, in which
-1e9 + x has swallowed x."""
import pytest
import torch

import beam_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, L, EOS, PAD = 509, 12, 508, 507
LIVE = -1.0e8


class Kernel:
    """Device state of one beam search and the ping-pong bookkeeping around ``hip.beam_step``."""

    def __init__(self, B, nb):
        st = R.new_state(B, nb, L, PAD)
        self.B, self.nb = B, nb
        self.run = [st["running_sequences"].to(DEV), st["running_sequences"].to(DEV).clone()]
        self.seq = [st["sequences"].to(DEV), st["sequences"].to(DEV).clone()]
        self.rbs, self.bs = st["running_beam_scores"].to(DEV), st["beam_scores"].to(DEV)
        self.fin, self.glen, self.unsat = st["is_sent_finished"].to(DEV), st["gen_len"].to(DEV), st["unsat"].to(DEV)
        self.tok = torch.full((B * nb,), -7, dtype=torch.int64, device=DEV)
        self.src = torch.full((B * nb,), -7, dtype=torch.int64, device=DEV)
        self.hits = torch.zeros(B, dtype=torch.bool, device=DEV)

    def step(self, score, index, cur, length_penalty, early_stopping):
        from pgca_amd import hip
        hip.beam_step(score.to(DEV), index.to(DEV), self.B, self.nb, V, cur, L, EOS, length_penalty, early_stopping,
                      self.run[0], self.run[1], self.rbs, self.seq[0], self.seq[1], self.bs, self.fin, self.glen,
                      self.unsat, self.tok, self.src, self.hits)
        self.run.reverse()
        self.seq.reverse()
        return dict(running_sequences=self.run[0].cpu(), sequences=self.seq[0].cpu(),
                    running_beam_scores=self.rbs.cpu(), beam_scores=self.bs.cpu(), is_sent_finished=self.fin.cpu(),
                    gen_len=self.glen.cpu(), unsat=self.unsat.cpu()), self.tok.cpu(), self.src.cpu(), self.hits.cpu()


def candidates(B, nb, cur, gen, eos_at=(), ties=False):
    """K = 2 * nb candidates per item in descending score order; [EOS] at the ranks ``eos_at``."""
    K = 2 * nb
    score = -0.5 * (cur + 1) - 0.3 * torch.arange(K).float()[None, :] - 0.2 * torch.rand(B, 1, generator=gen)
    score = score - 0.05 * torch.rand(B, K, generator=gen).sort(dim=-1)[0]
    if ties and K >= 4:
        score[:, 1] = score[:, 0]                                # equal inside the first nb
        score[:, K - 1] = score[:, K - 2]                        # ... and among the spares
    beam = torch.randint(0, nb, (B, K), generator=gen)
    tok = torch.randint(0, PAD, (B, K), generator=gen)
    for r in eos_at:
        if r < K:
            tok[:, r] = EOS
    return score, beam * V + tok


def compare(got, want, where):
    gs, gt, gsrc, gh = got
    ws, wt, wsrc, wh = want
    B, nb = ws["beam_scores"].shape
    assert torch.equal(gs["unsat"], ws["unsat"]) and torch.equal(gh, wh), where
    live = ws["beam_scores"] > LIVE
    assert torch.equal(gs["beam_scores"] > LIVE, live), where
    assert torch.allclose(gs["beam_scores"][live], ws["beam_scores"][live], rtol=1e-6, atol=0), where
    for k in ("sequences", "is_sent_finished", "gen_len"):
        assert torch.equal(gs[k][live], ws[k][live]), (where, k)
    live = ws["running_beam_scores"] > LIVE
    assert torch.equal(gs["running_beam_scores"] > LIVE, live), where
    assert torch.allclose(gs["running_beam_scores"][live], ws["running_beam_scores"][live], rtol=1e-6, atol=0), where
    assert torch.equal(gs["running_sequences"][live], ws["running_sequences"][live]), where
    assert torch.equal(gt[live.view(-1)], wt[live.view(-1)]) and torch.equal(gsrc[live.view(-1)], wsrc[live.view(-1)]), where
    assert bool(((gsrc >= 0) & (gsrc < B * nb)).all()), where


def scenario(B, nb, length_penalty, early_stopping, plan, seed, ties=False):
    """``plan``: step -> ranks that carry [EOS].  Returns the per-step reference states."""
    gen = torch.Generator().manual_seed(seed)
    ker = Kernel(B, nb)
    st = R.new_state(B, nb, L, PAD)
    states = []
    for cur in range(L):
        score, index = candidates(B, nb, cur, gen, plan(cur), ties)
        want = R.beam_step(st, score, index, V, cur, L, EOS, length_penalty, early_stopping)
        got = ker.step(score, index, cur, length_penalty, early_stopping)
        compare(got, want, (B, nb, length_penalty, early_stopping, cur))
        # the kernel goes on from ITS state, the restatement from its own: garbage slots may differ, live ones not
        st = want[0]
        states.append(want)
    assert bool(states[-1][3].all())                             # cur + 1 == L: every candidate hits
    return states


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nb", [1, 2, 4, 32])
def test_eos_inside_and_outside_the_first_num_beams(nb, B):
    inside = scenario(B, nb, 1.0, False, lambda cur: (0,) if cur in (2, 5) else (), 10 * nb + B)
    assert bool(inside[2][0]["is_sent_finished"][:, 0].all()) and int(inside[2][0]["gen_len"][0, 0]) == 3
    outside = scenario(B, nb, 1.0, False, lambda cur: (nb,) if cur in (2, 5) else (), 20 * nb + B)
    assert not bool(outside[5][0]["is_sent_finished"].any())     # a spare that ends is dropped, not finished
    assert int((outside[5][0]["running_sequences"][:, :, :6] == EOS).sum()) == 0


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nb", [1, 2, 4, 32])
def test_every_candidate_ends(nb, B):
    states = scenario(B, nb, 1.0, False, lambda cur: range(2 * nb) if cur == 3 else (), 30 * nb + B)
    assert bool(states[3][3].all()) and not bool(states[2][3].any())
    assert bool(states[3][0]["is_sent_finished"].all())
    assert bool((states[3][0]["running_beam_scores"] < LIVE).all())


@pytest.mark.parametrize("length_penalty,enters", [(0.0, False), (2.0, True)])
@pytest.mark.parametrize("nb", [2, 4])
def test_a_full_pool_takes_only_a_better_candidate(nb, length_penalty, enters):
    """Steps 1 .. fill the pool with one hypothesis each; the candidate that ends at step 9 scores -5 - noise: divided by
    10^0 it is worse than everything in the pool, divided by 10^2 better."""
    plan = lambda cur: (0,) if (1 <= cur <= nb or cur == 9) else ()  # noqa: E731
    states = scenario(3, nb, length_penalty, "never", plan, 40 * nb + int(length_penalty))
    before, after = states[8][0], states[9][0]
    assert bool(before["is_sent_finished"].all())
    assert bool((after["gen_len"] == 10).any(dim=-1).all()) == enters
    if not enters:
        assert torch.equal(after["sequences"], before["sequences"])


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("early_stopping", [False, True, "never"])
@pytest.mark.parametrize("nb", [2, 4])
def test_early_stopping_and_length_penalty(nb, early_stopping, length_penalty):
    plan = lambda cur: (0, nb - 1) if cur in (1, 2, 3, 6, 8) else ()  # noqa: E731
    states = scenario(3, nb, length_penalty, early_stopping, plan, 50 * nb + int(length_penalty))
    unsat = torch.stack([s[0]["unsat"] for s in states])
    if early_stopping == "never" and length_penalty > 0:
        assert bool(unsat[:-1].all())                            # scores / L^p can still beat the pool
    if early_stopping is False and length_penalty == 0.0:
        assert not bool(unsat[4].any())                          # the running best is already worse than the pool
    if early_stopping is True:                                   # a full pool is closed for good
        full = torch.stack([s[0]["is_sent_finished"].all(dim=-1) for s in states])
        first = int(full[:, 0].int().argmax())
        assert bool(full[first:, 0].all())
        assert torch.equal(states[-1][0]["sequences"][0], states[first][0]["sequences"][0])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nb", [2, 4, 32])
def test_exact_ties_go_to_the_lower_index(nb, B):
    states = scenario(B, nb, 1.0, False, lambda cur: (0, 1) if cur in (2, 4) else (), 60 * nb + B, ties=True)
    pool = states[2][0]
    assert bool((pool["beam_scores"][:, 0] == pool["beam_scores"][:, 1]).all())   # both tied candidates finished, in order
    # a candidate whose finished score equals one in the pool goes behind it: pool entries come first in the merge
    ker = Kernel(1, 2)
    st = R.new_state(1, 2, L, PAD)
    score = torch.tensor([[-1.0, -1.5, -2.0, -2.5]])
    index = torch.tensor([[EOS, 3, V + EOS, 4]])
    for cur, sc in ((0, score), (1, 2 * score)):                 # -2 / 2 == -1 / 1
        want = R.beam_step(st, sc, index, V, cur, L, EOS, 1.0, False)
        got = ker.step(sc, index, cur, 1.0, False)
        compare(got, want, ("pool tie", cur))
        st = want[0]
    assert st["beam_scores"][0].tolist() == [-1.0, -1.0] and st["gen_len"][0].tolist() == [1, 2]


def test_bad_arguments_are_errors():
    from pgca_amd import hip
    ker = Kernel(1, 2)
    score, index = torch.zeros(1, 4, device=DEV), torch.zeros(1, 4, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="pgca_beam_step"):    # in-place gather
        hip.beam_step(score, index, 1, 2, V, 0, L, EOS, 1.0, False, ker.run[0], ker.run[0], ker.rbs, ker.seq[0],
                      ker.seq[1], ker.bs, ker.fin, ker.glen, ker.unsat, ker.tok, ker.src, ker.hits)
    with pytest.raises(RuntimeError, match="pgca_beam_step"):    # cur == L
        hip.beam_step(score, index, 1, 2, V, L, L, EOS, 1.0, False, ker.run[0], ker.run[1], ker.rbs, ker.seq[0],
                      ker.seq[1], ker.bs, ker.fin, ker.glen, ker.unsat, ker.tok, ker.src, ker.hits)
