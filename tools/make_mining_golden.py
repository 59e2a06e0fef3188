#!/usr/bin/env python3
"""Record tests/golden/pair_mining.npz: what the reference's pairing rule emits for scored captions.

    python tools/make_mining_golden.py --reference <checkout of A-SHOJAEI/preference-guided-image-captioning-alignment>

Run by hand where the reference is checked out (it is not needed to run the tests).  The reference's
``data/loader.py`` is imported as it is - ``transformers`` first, then a stub ``torchvision`` so that its
``preprocessing`` module loads - and ``UltraFeedbackDataset._process_scored_captions`` (loader.py:416-451) is called
unbound with a ``SimpleNamespace(preference_threshold=..., logger=...)`` as ``self``.

The reference subtracts Python floats (float64); the kernel subtracts float32.  Every recorded case is therefore
checked here: for each adjacent pair of the sorted scores the float64 and the float32 decision agree.  Two families,
n = 1 .. 8:
  dyadic      scores on multiples of 1/8 (many ties), thresholds 0, 0.25, 0.5: both precisions are exact
  continuous  standard-normal float32 scores, thresholds 0.0, 0.6; a case with a difference within 1e-5 of the
              threshold is rejected (drawn again), and at most 1 % of the draws may be.
Recorded per case: family, n, scores [8] f32 (zero padded), threshold (float64), count, winners / losers [7] (-1 padded)
as candidate indices - the captions handed to the reference are the indices as strings.
"""
import argparse
import importlib
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAX = 8
FAMILIES = ("dyadic", "continuous")


def import_loader(reference: str):
    import transformers  # noqa: F401  (first: it must not see the stub below)
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tv.transforms)
    sys.path.insert(0, os.path.join(reference, "src"))
    return importlib.import_module("preference_guided_image_captioning_alignment.data.loader")


def reference_pairs(loader, scores, threshold):
    me = types.SimpleNamespace(preference_threshold=threshold, logger=logging.getLogger("golden"))
    item = {"image_path": "x", "captions": [str(j) for j in range(len(scores))], "scores": [float(s) for s in scores]}
    pairs = loader.UltraFeedbackDataset._process_scored_captions(me, item)
    return [int(p["preferred_caption"]) for p in pairs], [int(p["rejected_caption"]) for p in pairs]


def precisions_agree(scores, threshold, guard):
    """Adjacent differences of the sorted scores: float64 and float32 decide alike (and, with ``guard``, none lies
    within it of the threshold)."""
    s = np.sort(np.asarray(scores, np.float32))[::-1]
    for a, b in zip(s[:-1], s[1:]):
        d64, d32 = float(a) - float(b), np.float32(a - b)
        if guard and abs(d64 - threshold) < guard:
            return False
        if (d64 >= threshold) != bool(d32 >= np.float32(threshold)):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PGCA_REFERENCE"), required="PGCA_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pair_mining.npz"))
    ap.add_argument("--repeats", type=int, default=6)
    args = ap.parse_args()
    loader = import_loader(args.reference)
    rng = np.random.default_rng(20251)
    rows, drawn, rejected = [], 0, 0
    for family, thresholds, guard in (("dyadic", (0.0, 0.25, 0.5), 0.0), ("continuous", (0.0, 0.6), 1e-5)):
        for n in range(1, NMAX + 1):
            for threshold in thresholds:
                for _ in range(args.repeats):
                    while True:
                        drawn += 1
                        if family == "dyadic":
                            scores = (rng.integers(-8, 9, n) / 8.0).astype(np.float32)
                        else:
                            scores = rng.standard_normal(n).astype(np.float32)
                        if precisions_agree(scores, threshold, guard):
                            break
                        rejected += 1
                        assert family != "dyadic", "float32 and float64 must agree exactly on the dyadic grid"
                    win, lose = reference_pairs(loader, scores, threshold)
                    rows.append((FAMILIES.index(family), n, scores, threshold, win, lose))
    assert rejected <= 0.01 * drawn, f"{rejected} of {drawn} draws rejected"
    C = len(rows)
    out = dict(family=np.zeros(C, np.int32), n=np.zeros(C, np.int32), scores=np.zeros((C, NMAX), np.float32),
               threshold=np.zeros(C, np.float64), count=np.zeros(C, np.int32),
               win=np.full((C, NMAX - 1), -1, np.int32), lose=np.full((C, NMAX - 1), -1, np.int32))
    for c, (fam, n, scores, threshold, win, lose) in enumerate(rows):
        out["family"][c], out["n"][c], out["threshold"][c], out["count"][c] = fam, n, threshold, len(win)
        out["scores"][c, :n] = scores
        out["win"][c, :len(win)], out["lose"][c, :len(lose)] = win, lose
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {C} cases, {int(out['count'].sum())} pairs, {rejected} of {drawn} draws rejected")


if __name__ == "__main__":
    main()
