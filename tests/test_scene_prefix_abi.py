"""CPU-side checks of the shared-prefix path: the four entry points of csrc/decode_shared.hip / csrc/decoder.hip load from the library,
their workspace queries behave, the Python surface (StandInHead.prefill_prefix / generate(prefix=, prefix_index=),
InferenceEngine.open_scene / Scene.ask / generate_batch(share_scenes=)) is there, and the engine's grouping of questions by scene is
right on an engine built from fakes."""
import ctypes
import inspect
import os
import weakref

import pytest
import torch

from lidar_vision_vqa_amd import _ffi, synth

NEW = ("lvq_attention_extend_shared_workspace_bytes", "lvq_attention_extend_shared", "lvq_qwen2_extend_shared_workspace_bytes",
       "lvq_qwen2_extend_shared")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _ffi.lib()


def test_shared_symbols_are_declared_exported_and_listed(lib):
    declared = _ffi.declared_symbols()
    txt = open(os.path.join(os.path.dirname(_ffi.HEADER_PATH), "..", "INTEGRATION.md")).read()
    table = txt[txt.index("abi-table:begin"):]
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert f"| `{name}` |" in table, name


def test_attention_workspace_query(lib):
    q = lambda batch, lq, H, Hk, pmax, lown, dh, prec: int(lib.lvq_attention_extend_shared_workspace_bytes(
        *(ctypes.c_int(v) for v in (batch, lq, H, Hk, pmax, lown, dh, prec))))
    assert q(8, 60, 14, 2, 840, 124, 64, 3) > 0
    # no sequences, no query rows, no prefix rows, no own rows, heads that do not group, a group wider than one MFMA tile, head dims the
    # kernel does not take, an unknown precision
    for bad in ((0, 60, 14, 2, 840, 124, 64, 3), (8, 0, 14, 2, 840, 124, 64, 3), (8, 60, 14, 2, 0, 124, 64, 3), (8, 60, 14, 2, 840, 0, 64, 3),
                (8, 60, 14, 4, 840, 124, 64, 3), (8, 60, 34, 2, 840, 124, 64, 3), (8, 60, 14, 2, 840, 124, 72, 3),
                (8, 60, 14, 2, 840, 124, 144, 3), (8, 60, 14, 2, 840, 124, 64, 2), (8, 60, 0, 2, 840, 124, 64, 1), (8, 60, 14, 0, 840, 124, 64, 1)):
        assert q(*bad) == 0, bad
    grows = lambda sizes: sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert grows([q(8, lq, 14, 2, 840, 124, 64, 1) for lq in (1, 2, 17, 60)])
    assert grows([q(8, 60, 14, 2, 840, lown, 64, 1) for lown in (100, 1000, 4000)])
    assert grows([q(batch, 60, 14, 2, 840, 124, 64, 1) for batch in (1, 3, 8)])
    # one query row, and the prefix and own rows in one cache: what lvq_attention_decode_ragged asks for
    assert q(8, 1, 14, 2, 840, 184, 64, 3) == int(lib.lvq_attention_decode_ragged_workspace_bytes(
        *(ctypes.c_int(v) for v in (8, 14, 2, 1024, 64, 3))))


def test_step_workspace_query(lib):
    q = lambda batch, lq, d, H, Hk, inter, pmax, lown, prec: int(lib.lvq_qwen2_extend_shared_workspace_bytes(
        *(ctypes.c_int(v) for v in (batch, lq, d, H, Hk, inter, pmax, lown, prec))))
    assert q(8, 60, 896, 14, 2, 4864, 840, 124, 3) > 0
    for bad in ((0, 60, 896, 14, 2, 4864, 840, 124, 3), (8, 0, 896, 14, 2, 4864, 840, 124, 3), (8, 60, 896, 13, 2, 4864, 840, 124, 3),
                (8, 60, 896, 14, 2, 0, 840, 124, 3), (8, 60, 896, 14, 2, 4864, 0, 124, 3), (8, 60, 896, 14, 2, 4864, 840, 0, 3),
                (8, 60, 896, 14, 4, 4864, 840, 124, 3), (8, 60, 72 * 14, 14, 2, 4864, 840, 124, 3)):
        assert q(*bad) == 0, bad
    grows = lambda sizes: sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert grows([q(8, lq, 896, 14, 2, 4864, 840, 124, 3) for lq in (1, 2, 17, 60)])
    assert grows([q(8, 60, 896, 14, 2, 4864, 840, lown, 3) for lown in (100, 1000, 4000)])
    assert grows([q(batch, 60, 896, 14, 2, 4864, 840, 124, 3) for batch in (1, 3, 8)])
    # the activations of batch * lq rows (fp32 gate|up and residual) are in it
    assert q(8, 60, 896, 14, 2, 4864, 840, 124, 3) > 8 * 60 * (2 * 4864 * 4 + 896 * 4)


def test_python_surface():
    from lidar_vision_vqa_amd import engine, head, ops
    g = inspect.signature(head.StandInHead.generate).parameters
    assert g["prefix"].default is None and g["prefix_index"].default is None
    p = inspect.signature(head.StandInHead.prefill_prefix).parameters
    assert list(p) == ["self", "inputs_embeds", "lengths"] and p["lengths"].default is None
    b = inspect.signature(engine.InferenceEngine.generate_batch).parameters
    assert list(b)[:5] == ["self", "questions", "bevs", "sample_tokens", "batch_size"]      # the reference's positional order is kept
    assert b["share_scenes"].default is False and b["batch_size"].default == 1
    o = inspect.signature(engine.InferenceEngine.open_scene).parameters
    assert list(o) == ["self", "bev", "sample_token"] and o["sample_token"].default is None
    assert list(inspect.signature(engine.Scene.ask).parameters)[:2] == ["self", "questions"]
    assert callable(ops.attention_extend_shared) and hasattr(head, "PrefixCache")


# ------------------------------------------------------------------------------------------------
# the engine's grouping, on fakes
# ------------------------------------------------------------------------------------------------
D = 2


class CountingLidar:
    """BEV -> 3 prompt rows filled with the BEV's mean: the scene's mark"""

    def __init__(self):
        self.calls = []

    def __call__(self, bev):
        self.calls.append(tuple(bev.shape))
        return bev.mean().reshape(1, 1, 1).expand(bev.shape[0], 3, D).contiguous()


class RecordingHead:
    """A `base_model` that computes nothing: embedding row of token i = (i, 1); `prefill_prefix` keeps the rows as layer 0's keys;
    `generate` answers (mark of the sequence's prefix, last three characters of its question) and records its arguments."""

    def __init__(self):
        self.prefills, self.calls = [], []

    def get_input_embeddings(self):
        return lambda ids: torch.stack([ids.float(), torch.ones_like(ids).float()], dim=-1)

    def prefill_prefix(self, inputs_embeds, lengths=None):
        from lidar_vision_vqa_amd import head
        G, P, _ = inputs_embeds.shape
        self.prefills.append((G, P))
        rows = inputs_embeds.clone()
        return head.PrefixCache([((rows, None), (rows, None))], torch.full((G,), P, dtype=torch.int32), [P] * G, P, "fake", (), weakref.ref(self))

    def generate(self, inputs_embeds, attention_mask=None, prompt_lengths=None, prefix=None, prefix_index=None, **kw):
        self.calls.append(dict(shape=tuple(inputs_embeds.shape), lens=prompt_lengths.tolist(), index=prefix_index.tolist(),
                               plen=prefix.plen.tolist(), kw=kw))
        tail = len("\nAnswer:")
        out = []
        for b, n in enumerate(prompt_lengths.tolist()):
            assert bool((attention_mask[b, :n] == 1).all()) and bool((attention_mask[b, n:] == 0).all())
            g = prefix_index[b]
            mark = int(round(float(prefix.layers[0][0][0][g, 1, 0]) / 0.2))              # row 1: the first LiDAR prompt row, scaled
            assert int(prefix.layers[0][0][0][g, int(prefix.plen[g]) - 1, 0]) == 3         # the last prefix row is <lidar_end>
            out.append([4 + mark] + [int(v) for v in inputs_embeds[b, n - tail - 3:n - tail, 0]])
        return torch.tensor(out)


class PlainHead(RecordingHead):
    """`generate` without a `prefix` parameter (a transformers-style model object)"""
    prefill_prefix = None

    def generate(self, inputs_embeds, attention_mask=None, **kw):
        self.calls.append(dict(shape=tuple(inputs_embeds.shape), kw=kw))
        return torch.full((inputs_embeds.shape[0], 2), 40)


def _engine(base, lidar):
    from lidar_vision_vqa_amd import engine
    tok = synth.DummyTokenizer(128)
    return engine.InferenceEngine(dict(tokenizer=tok, base_model=base, vat_lidar=lidar, device=torch.device("cpu"), d_model=D,
                                       config=dict(use_vision=False, prefix_scale=0.2, system_prompt="Drive."))), tok


def _want(tok, mark, question):
    return tok.decode([4 + mark] + tok.encode(question[-3:])).strip()


def test_share_scenes_grouping_prefix_index_and_answer_order():
    base, lidar = RecordingHead(), CountingLidar()
    eng, tok = _engine(base, lidar)
    bev = {m: torch.full((4, 6, 6), float(m)) for m in (5, 10, 15)}
    same_path = "scene_c.npy"
    # three scenes with 1, 3 and 4 questions, interleaved; scene 15 twice under another sample token = a fourth scene
    triples = [("count cars", bev[10], "b"), ("any truck", bev[5], "a"), ("is it wet", bev[15], "c"), ("how fast", bev[10], "b"),
               ("left or right", bev[15], "c"), ("who is near", bev[15], "c"), ("safe to go", bev[10], "b"), ("one more", bev[15], "c"),
               ("other token", bev[15], "d")]
    qs, bs, ts = (list(x) for x in zip(*triples))
    marks = [10, 5, 15, 10, 15, 15, 10, 15, 15]
    want = [_want(tok, m, q) for m, q in zip(marks, qs)]
    got = eng.generate_batch(qs, bs, ts, 4, share_scenes=True, max_new_tokens=4, do_sample=False)
    assert got == want
    assert len(lidar.calls) == 4 and all(c == (1, 4, 6, 6) for c in lidar.calls)          # one LiDAR pass per scene
    P = 2 + 3                                                                            # <lidar_start>, 3 prompt rows, <lidar_end>
    assert base.prefills == [(1, P)] * 4
    assert [c["shape"][0] for c in base.calls] == [4, 4, 1]
    # prefix_index counts the scenes of ONE call in the order they first appear in it
    assert [c["index"] for c in base.calls] == [[0, 1, 2, 0], [0, 0, 1, 0], [0]]
    assert [c["plen"] for c in base.calls] == [[P] * 3, [P] * 2, [P]]
    sys_rows = len("Drive.\n\n") + len("\nAnswer:")
    assert base.calls[0]["lens"] == [sys_rows + len(q) for q in qs[:4]]                  # only the rows behind <lidar_end>
    assert all(c["kw"]["max_new_tokens"] == 4 and c["kw"]["do_sample"] is False for c in base.calls)
    # one call for everything; the same object without sample tokens is one scene
    base.calls.clear(), lidar.calls.clear()
    assert eng.generate_batch(qs, bs, None, 16, share_scenes=True, max_new_tokens=4, do_sample=False) == want
    assert len(base.calls) == 1 and len(lidar.calls) == 3 and base.calls[0]["index"] == [0, 1, 2, 0, 2, 2, 0, 2, 2]


def test_open_scene_and_ask_on_fakes():
    base, lidar = RecordingHead(), CountingLidar()
    eng, tok = _engine(base, lidar)
    scene = eng.open_scene(torch.full((4, 6, 6), 7.0), "tok")
    assert scene.n_rows == 5 and len(lidar.calls) == 1 and base.prefills == [(1, 5)]
    qs = ["what is ahead", "okay?", "turn"]
    assert scene.ask(qs, max_new_tokens=3, do_sample=False) == [_want(tok, 7, q) for q in qs]
    assert scene.ask([]) == []
    assert len(lidar.calls) == 1 and len(base.prefills) == 1 and len(base.calls) == 1 and base.calls[0]["index"] == [0, 0, 0]
    other = eng.open_scene(torch.full((4, 6, 6), 9.0))
    scene.lidar = other.lidar                                   # a scene whose prompt no longer starts with the cached rows
    with pytest.raises(_ffi.LvqError):
        scene.ask(["what now"])


def test_share_scenes_without_prefix_support_takes_the_existing_path():
    base, lidar = PlainHead(), CountingLidar()
    eng, tok = _engine(base, lidar)
    b = torch.full((4, 6, 6), 5.0)
    out = eng.generate_batch(["a b c", "d e f"], [b, b], ["s", "s"], share_scenes=True, max_new_tokens=2, do_sample=False)
    assert out == [tok.decode([40, 40]).strip()] * 2
    assert len(base.calls) == 2 and len(lidar.calls) == 2 and all(c["shape"][0] == 1 and c["shape"][1] > 5 for c in base.calls)
    with pytest.raises(_ffi.LvqError):
        eng.open_scene(b)
