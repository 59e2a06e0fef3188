"""``pgca_rouge_stats`` and ``pgca_meteor_stats`` are declared once in the header, add no struct and no ABI version,
and refuse every limit as an argument error before any launch: observable with no GPU.  Both are tried with S = 129 and
0, K = 9 and 0, base_vocab = 65536, N = 0 and 1 << 24, and each pointer null."""
import os

import pytest
import torch

from pgca_amd import abi, hip

ENTRIES = ("pgca_rouge_stats", "pgca_meteor_stats")
GOOD = {"N": 2, "K": 3, "S": 16, "base_vocab": 509, "stream": None}
PARAMS = ["pred_ids", "pred_len", "ref_ids", "ref_len", "N", "K", "S", "base_vocab", "out", "stream"]


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
    assert set(ENTRIES) <= set(abi.PROTOTYPES) and set(ENTRIES) <= set(hip.EXPORTS)
    assert hip.ABI_VERSION == 306 and len(abi.STRUCTS) == 3
    for entry in ENTRIES:
        assert [n for _, n in abi.PROTOTYPES[entry].params] == PARAMS, entry
    assert callable(hip.rouge_stats) and callable(hip.meteor_stats)


@pytest.mark.parametrize("entry", ENTRIES)
def test_limits_are_refused_before_any_launch(lib, host_buffer, entry):
    cases = [("S", 129), ("S", 0), ("K", 9), ("K", 0), ("base_vocab", 65536), ("N", 0), ("N", 1 << 24)]
    pointers = [n for t, n in abi.PROTOTYPES[entry].params if t.endswith("*") and n != "stream"]
    assert pointers == ["pred_ids", "pred_len", "ref_ids", "ref_len", "out"]
    cases += [(p, None) for p in pointers]
    for name, value in cases:
        rc, err = call(lib, entry, host_buffer, **{name: value})
        assert rc == -1 and entry in err, (entry, name, value, rc, err)
