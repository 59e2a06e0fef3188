"""What a captured decode step's validity rests on (``CaptionDecoderEngine.decode_advance``), checked on a CPU
``Workspace``: a key's allocation serial moves exactly when the key gets new storage, a stamp over a set of keys is the
conjunction of those, and the cache-stride vectors of different decode shapes live side by side."""
import torch

from pgca_amd.engine import GptTrunk, Workspace

F32 = torch.float32


def test_serial_changes_when_get_regrows_the_buffer():
    ws = Workspace("cpu")
    a = ws.get("gen.hf", (4, 8), F32)
    s0 = ws.serial["gen.hf"]
    b = ws.get("gen.hf", (40, 8), F32)
    assert b.data_ptr() != a.data_ptr()          # both alive here, so the addresses must differ: it IS a new allocation
    assert ws.serial["gen.hf"] != s0
    s1 = ws.serial["gen.hf"]
    ws.get("gen.hf", (40, 8), torch.bfloat16)    # another dtype is new storage as well
    assert ws.serial["gen.hf"] != s1


def test_serial_changes_when_cached_rebuilds():
    ws = Workspace("cpu")
    a = ws.cached("cu", (8, 4), lambda: torch.arange(9) * 4)
    s0 = ws.serial["cu"]
    assert ws.cached("cu", (8, 4), lambda: torch.arange(9) * 4) is a and ws.serial["cu"] == s0
    b = ws.cached("cu", (4, 8), lambda: torch.arange(5) * 8)
    assert b is not a and ws.serial["cu"] != s0
    s1 = ws.serial["cu"]
    c = ws.cached("cu", (8, 4), lambda: torch.arange(9) * 4)     # back to the first stamp: built again, a third tensor
    assert c is not a and c is not b and ws.serial["cu"] not in (s0, s1)


def test_serial_stays_on_a_same_size_or_smaller_request():
    ws = Workspace("cpu")
    a = ws.get("gen.x", (40, 8), F32)
    s0 = ws.serial["gen.x"]
    for shape in ((40, 8), (8, 40), (4, 8), (1,), (320,)):
        v = ws.get("gen.x", shape, F32, zero=True)
        assert v.data_ptr() == a.data_ptr() and ws.serial["gen.x"] == s0, shape


def test_recording_collects_the_keys_asked_for_inside_the_block_only():
    ws = Workspace("cpu")
    ws.get("before", (2,), F32)
    with ws.recording() as keys:
        ws.get("a", (2,), F32)
        ws.get("a", (1,), F32)
        ws.cached("c", (1,), lambda: torch.zeros(1))
        with ws.recording() as inner:
            ws.get("b", (2,), F32)
    ws.get("after", (2,), F32)
    assert keys == {"a", "b", "c"} and inner == {"b"}


def test_stamp_breaks_when_any_of_its_keys_reallocates_and_only_then():
    ws = Workspace("cpu")
    with ws.recording() as keys:
        ws.get("gen.kv", (2, 24, 6), torch.bfloat16)
        ws.get("gen.hf", (4, 8), F32)
        ws.cached("gen.cu.4x6", (4, 6), lambda: torch.arange(5) * 6)
    stamp = ws.stamp(keys)
    assert ws.stamp(keys) == stamp
    # unrelated keys come, grow and are rebuilt; the recorded ones are asked for again at their size or smaller
    ws.get("other", (4,), F32)
    ws.get("other", (400,), F32)
    ws.cached("gen.cu.6x4", (6, 4), lambda: torch.arange(7) * 4)
    ws.cached("gen.cu.6x4", (6, 5), lambda: torch.arange(7) * 5)
    ws.get("gen.hf", (2, 8), F32)
    ws.cached("gen.cu.4x6", (4, 6), lambda: torch.arange(5) * 6)
    assert ws.stamp(keys) == stamp
    for regrow in (lambda w: w.get("gen.kv", (2, 48, 6), torch.bfloat16), lambda w: w.get("gen.hf", (40, 8), F32),
                   lambda w: w.cached("gen.cu.4x6", (4, 7), lambda: torch.arange(5) * 7)):
        before = ws.stamp(keys)
        regrow(ws)
        assert ws.stamp(keys) != before
        assert ws.stamp(keys) != stamp


def test_equal_product_decode_shapes_keep_their_own_stride_vectors():
    """(8, 4) and (4, 8) share every sized buffer (R * smax = 32 rows) but not ``cu``: each keeps its own vector, alive
    at the same time, and coming back to a shape finds the vector it left."""
    from pgca_amd.arch import tiny_arch
    from pgca_amd.params import ParamStore
    arch = tiny_arch()
    ws = Workspace("cpu")
    trunk = GptTrunk(ParamStore(arch, "cpu", seed=0), "caption_decoder.lm_model.transformer", arch.gpt, ws, "d")
    a = trunk.decode_cache(8, 4)
    b = trunk.decode_cache(4, 8)
    a_again = trunk.decode_cache(8, 4)
    assert a.cu.tolist() == [4 * r for r in range(9)] and b.cu.tolist() == [8 * r for r in range(5)]
    assert a_again.cu is a.cu and a.cu.data_ptr() != b.cu.data_ptr()
    assert a.kv_all.data_ptr() == b.kv_all.data_ptr()            # the cache rows themselves ARE shared
    with ws.recording() as keys:
        trunk.decode_cache(8, 4)
    stamp = ws.stamp(keys)
    trunk.decode_cache(4, 8)
    trunk.decode_cache(8, 4)
    assert ws.stamp(keys) == stamp
