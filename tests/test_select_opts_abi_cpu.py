"""C-ABI checks of the generation entries added with ``pgca_select_opts`` that need no GPU: the argument validation of
``pgca_select_*_ex`` / ``pgca_beam_step``, which happens before any launch (the struct's layout: test_abi_cpu.py)."""
import ctypes
import os

import pytest
import torch  # noqa: F401  (loads libamdhip64 first, as the product does)

from pgca_amd import hip


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hip.LIB_PATH):
        from pgca_amd import build
        build.build()
    return hip.load()


def test_validation_needs_no_gpu(lib):
    opts = hip.SelectOpts(2, 0, None)
    fake = 1 << 12                                               # a 16-byte aligned non-null "pointer": never dereferenced
    V, nb = 50260, 8
    # penalty AND bans for 8 rows of 50 260: two planes of 8 x 6 284 bytes do not fit the LDS
    rc = lib.pgca_select_beam_candidates_ex(fake, V, V, 1, nb, fake, 4, 4, 1.1, 0, 1.0, 0, 1.0, fake, 2 * nb, 0, 0, fake,
                                            fake, ctypes.byref(opts), None)
    assert rc == -1 and b"61440" in lib.pgca_last_error()
    rc = lib.pgca_select_token_ex(fake, 300000, 300000, 1, fake, 4, 4, 1.1, 1.0, 0, 1.0, None, None, 0, fake, fake,
                                  ctypes.byref(opts), None)
    assert rc == -1 and b"61440" in lib.pgca_last_error()
    bad = hip.SelectOpts(0, 3, None)                             # three ids announced, no list
    rc = lib.pgca_select_token_ex(fake, V, V, 1, None, 0, 0, 1.0, 1.0, 0, 1.0, None, None, 0, fake, fake,
                                  ctypes.byref(bad), None)
    assert rc == -1 and b"pgca_select_token" in lib.pgca_last_error()
    assert lib.pgca_select_token_ex(fake, V, V, 1, None, 0, 0, 1.0, 1.0, 0, 1.0, None, None, 0, fake, fake, None,
                                    None) == -1
    step = lambda nb, cur, es, out: lib.pgca_beam_step(fake, fake, 1, nb, V, cur, 12, 0, 1.0, es, fake, out, fake, fake,  # noqa: E731
                                                       fake + 64, fake, fake, fake, fake, fake, fake, fake, None)
    for args in ((33, 0, 0, fake + 64), (4, 12, 0, fake + 64), (4, 0, 3, fake + 64), (4, 0, 0, fake)):
        assert step(*args) == -1 and b"pgca_beam_step" in lib.pgca_last_error(), args
