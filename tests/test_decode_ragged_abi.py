"""CPU-side checks of the ragged decode path: the four entry points of csrc/decode_ragged.hip / csrc/decoder.hip load from the
library, their workspace queries behave, and the Python surface (StandInHead.generate(prompt_lengths=),
InferenceEngine.generate_batch(batch_size=), InferenceEngine.answer_batch, ops.attention_decode_ragged) is there."""
import ctypes
import inspect
import os

import pytest

from lidar_vision_vqa_amd import _ffi

NEW = ("lvq_attention_decode_ragged_workspace_bytes", "lvq_attention_decode_ragged", "lvq_qwen2_decode_ragged_workspace_bytes",
       "lvq_qwen2_decode_step_ragged")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.lib()


def test_ragged_symbols_are_declared_and_exported(lib):
    declared = _ffi.declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name


def test_attention_workspace_query(lib):
    q = lambda batch, H, Hk, lmax, dh, prec: int(lib.lvq_attention_decode_ragged_workspace_bytes(
        *(ctypes.c_int(v) for v in (batch, H, Hk, lmax, dh, prec))))
    assert q(4, 14, 2, 1000, 64, 3) > 0
    # invalid shapes: no sequences, no keys, heads that do not group, a group wider than one MFMA tile, head dims the kernel does not
    # take, an unknown precision
    for bad in ((0, 14, 2, 1000, 64, 3), (4, 14, 2, 0, 64, 3), (4, 14, 4, 1000, 64, 3), (4, 34, 2, 1000, 64, 3), (4, 14, 2, 1000, 72, 3),
                (4, 14, 2, 1000, 144, 3), (4, 14, 2, 1000, 64, 2), (4, 0, 2, 1000, 64, 1), (4, 14, 0, 1000, 64, 1)):
        assert q(*bad) == 0, bad
    sizes = [q(4, 14, 2, lmax, 64, 1) for lmax in (100, 1000, 4000, 16000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
    assert q(8, 14, 2, 4000, 64, 1) > q(4, 14, 2, 4000, 64, 1)


def test_step_workspace_query(lib):
    q = lambda batch, d, H, Hk, inter, lmax, prec: int(lib.lvq_qwen2_decode_ragged_workspace_bytes(
        *(ctypes.c_int(v) for v in (batch, d, H, Hk, inter, lmax, prec))))
    assert q(8, 896, 14, 2, 4864, 1000, 3) > 0
    for bad in ((0, 896, 14, 2, 4864, 1000, 3), (8, 896, 13, 2, 4864, 1000, 3), (8, 896, 14, 2, 0, 1000, 3), (8, 896, 14, 2, 4864, 0, 3),
                (8, 896, 14, 4, 4864, 1000, 3), (8, 72 * 14, 14, 2, 4864, 1000, 3)):
        assert q(*bad) == 0, bad
    sizes = [q(8, 896, 14, 2, 4864, lmax, 3) for lmax in (100, 1000, 4000, 16000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), sizes
    # the ragged step needs what the scalar-position step needs besides attention scratch, plus the key-count array
    assert q(8, 896, 14, 2, 4864, 1000, 3) > 8 * (2 * 4864 * 4 + 896 * 4)


def test_python_surface():
    from lidar_vision_vqa_amd import engine, head, ops
    g = inspect.signature(head.StandInHead.generate).parameters
    assert "prompt_lengths" in g and g["prompt_lengths"].default is None
    b = inspect.signature(engine.InferenceEngine.generate_batch).parameters
    assert "batch_size" in b and b["batch_size"].default == 1
    assert list(b)[:4] == ["self", "questions", "bevs", "sample_tokens"]            # the reference's positional order is kept
    a = inspect.signature(engine.InferenceEngine.answer_batch).parameters
    assert list(a)[1:] == ["questions", "bevs", "sample_tokens", "decoding", "generator"]
    assert callable(ops.attention_decode_ragged)
