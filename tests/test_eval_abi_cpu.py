"""The limits of the caption-metric entry points are argument errors found before any launch: observable with no GPU.
Every entry is tried with S = 129, K = 9, base_vocab = 65536 and a null pointer where it has that parameter
(``pgca_token_overlap`` compares two single rows of plain ids: it has neither K nor a vocabulary)."""
import os

import pytest
import torch

from pgca_amd import abi, hip

ENTRIES = ("pgca_ngram_keys", "pgca_cider_rows", "pgca_bleu_stats", "pgca_token_overlap")
GOOD = {"G": 2, "N": 2, "R": 2, "K": 3, "S": 16, "order": 2, "base_vocab": 509, "distinct_per_group": 1, "table_len": 4,
        "n_docs": 2, "sigma": 6.0, "stream": None}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        from pgca_amd import build
        build.build()
    return hip.load()


@pytest.fixture(scope="module")
def host_buffer():
    return torch.zeros(4096, dtype=torch.int64)       # a non-null address; no entry gets as far as reading it


def call(lib, entry, buf, **change):
    """``entry`` with good scalar arguments and non-null pointers, except for ``change`` (name -> value)."""
    args = []
    for ctype, name in abi.PROTOTYPES[entry].params:
        if name in change:
            args.append(change[name])
        elif name in GOOD:
            args.append(GOOD[name])
        else:
            assert ctype.endswith("*"), (entry, name)
            args.append(buf.data_ptr())
    return getattr(lib, entry)(*args), lib.pgca_last_error().decode()


def test_the_entries_are_declared_without_a_new_struct_or_version():
    assert set(ENTRIES) <= set(abi.PROTOTYPES) and hip.ABI_VERSION == 306 and len(abi.STRUCTS) == 3
    assert (hip.EVAL_MAX_S, hip.EVAL_MAX_K, hip.EVAL_MAX_VOCAB) == (128, 8, 65535)
    assert abi.CONSTANTS["PGCA_EVAL_MAX_IMAGES"] == 1 << 24


@pytest.mark.parametrize("entry", ENTRIES)
def test_limits_are_refused_before_any_launch(lib, host_buffer, entry):
    names = [n for _, n in abi.PROTOTYPES[entry].params]
    images = next(n for n in ("G", "N", "R") if n in names)
    cases = [("S", 129), ("S", 0), (images, 1 << 24), (images, 0)]
    if "K" in names:
        cases += [("K", 9), ("K", 0)]
    if "base_vocab" in names:
        cases += [("base_vocab", 65536)]
    if "order" in names:
        cases += [("order", 5), ("order", 0)]
    pointers = [n for t, n in abi.PROTOTYPES[entry].params if t.endswith("*") and n != "stream"]
    assert len(pointers) >= 3
    cases += [(p, None) for p in pointers]
    for name, value in cases:
        rc, err = call(lib, entry, host_buffer, **{name: value})
        assert rc == -1 and entry in err, (entry, name, value, rc, err)
