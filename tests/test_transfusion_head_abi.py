"""The entry points of csrc/transfusion_head.hip on the host: exported by the built library, declared in include/lvq.h, bound in ops.py, listed in
INTEGRATION.md, and refusing with the documented codes before anything is launched (no GPU is needed: every refusal is a host-side check)."""
import ctypes
import os

import pytest

from lidar_vision_vqa_amd import _ffi as F
from lidar_vision_vqa_amd import ops

ENTRY_POINTS = ["lvq_heatmap_proposals", "lvq_heatmap_proposals_workspace_bytes", "lvq_pos_embed_learned", "lvq_transfusion_queries",
                "lvq_transfusion_add_pe", "lvq_transfusion_tail", "lvq_transfusion_tail_workspace_bytes"]
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -5
P = ctypes.c_void_p(4096)                          # a non-NULL, 16-byte aligned stand-in: a refused call reads nothing


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(F.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return F.lib()


def test_exported_declared_bound_and_listed(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    table = text[text.index("abi-table:begin"):]
    src = open(os.path.join(root, "lidar-vision-vqa_amd", "ops.py")).read()
    for n in ENTRY_POINTS:
        assert n in F.declared_symbols() and hasattr(lib, n) and f"| `{n}` |" in table, n
        assert f"L.{n}(" in src or f"lib().{n}(" in src, n
    for fn in ("heatmap_proposals", "pos_embed_learned", "transfusion_queries", "transfusion_add_pe", "transfusion_tail"):
        assert callable(getattr(ops, fn))
    assert "LVQ_HEAD_TORCH_POST" in text and "TransFusionHead" in text


def test_heatmap_proposals_refusals(lib):
    n = ctypes.c_size_t(0)
    assert lib.lvq_heatmap_proposals_workspace_bytes(2, 10, 24, 24, ctypes.byref(n)) == 0 and n.value >= 2 * 10 * 24 * 24 * 4
    assert lib.lvq_heatmap_proposals_workspace_bytes(2, 10, 24, 24, None) == EINVAL
    assert lib.lvq_heatmap_proposals_workspace_bytes(2, 65, 24, 24, ctypes.byref(n)) == EINVAL
    assert lib.lvq_heatmap_proposals_workspace_bytes(1, 64, 8192, 8192, ctypes.byref(n)) == EUNSUPPORTED

    def call(batch=2, c_total=64, h=24, w=24, first=0, n_cls=10, kernel=3, p=48, maps=P, ws=P, ws_bytes=1 << 30):
        return lib.lvq_heatmap_proposals(maps, batch, c_total, h, w, first, n_cls, 0x300, kernel, p, P, P, P, ws, ws_bytes, None)
    assert call(p=1025) == EUNSUPPORTED and call(kernel=1) == EUNSUPPORTED and call(kernel=5) == EUNSUPPORTED
    assert call(n_cls=1, h=3, w=3, p=10) == EINVAL            # P > n_cls H W
    assert call(h=2) == EINVAL and call(w=2) == EINVAL
    assert call(n_cls=65, c_total=128) == EINVAL
    assert call(first=60) == EINVAL and call(maps=None) == EINVAL and call(p=0) == EINVAL and call(batch=0) == EINVAL
    assert call(ws_bytes=16) == EWORKSPACE and call(ws=None) == EWORKSPACE


def test_pos_embed_and_queries_refusals(lib):
    def pe(n=8, d=128, d_out=128, pos=P, w2=P):
        return lib.lvq_pos_embed_learned(pos, n, d, d_out, P, P, P, w2, P, P, None)
    assert pe(n=0) == EINVAL and pe(pos=None) == EINVAL and pe(d=0) == EINVAL and pe(d_out=0) == EINVAL
    assert pe(d=130) == EUNSUPPORTED and pe(d=516) == EUNSUPPORTED and pe(d_out=516) == EUNSUPPORTED
    assert pe(w2=ctypes.c_void_p(4100)) == EUNSUPPORTED

    def q(batch=2, h=24, w=24, d=128, p=48, n_cls=10, y=24, hi=P):
        return lib.lvq_transfusion_queries(hi, None, batch, h, w, d, P, p, n_cls, y, P, P, P, P, P, P, P, P, P, P, P, None)
    assert q(hi=None) == EINVAL and q(p=0) == EINVAL and q(y=0) == EINVAL and q(batch=0) == EINVAL
    assert q(d=144) == EUNSUPPORTED and q(n_cls=65) == EUNSUPPORTED and q(d=100) == EUNSUPPORTED
    assert lib.lvq_transfusion_add_pe(None, P, 8, P, None, None) == EINVAL and lib.lvq_transfusion_add_pe(P, P, 0, P, None, None) == EINVAL


def test_tail_refusals(lib):
    n = ctypes.c_size_t(0)
    assert lib.lvq_transfusion_tail_workspace_bytes(2, 48, 9, ctypes.byref(n)) == 0 and n.value >= 2 * 48 * 11 * 4
    assert lib.lvq_transfusion_tail_workspace_bytes(2, 48, 8, ctypes.byref(n)) == EINVAL
    assert lib.lvq_transfusion_tail_workspace_bytes(2, 1025, 9, ctypes.byref(n)) == EUNSUPPORTED
    geo = F.f32x([0.075, 0.075])
    lim = F.f32x([-1, -1, -1, 1, 1, 1])

    def call(batch=2, p=48, ffn=256, n_cls=10, vel=1, x=P, w1=P, ws=P, ws_bytes=1 << 20, stride=8):
        return lib.lvq_transfusion_tail(x, P, P, P, batch, p, ffn, n_cls, vel, w1, P, P, P, P, P, 1e-5, P, P, P, P, P, stride, geo, geo, lim, 0.0,
                                        P, P, P, P, P, ws, ws_bytes, None)
    assert call(x=None) == EINVAL and call(batch=0) == EINVAL and call(stride=0) == EINVAL and call(n_cls=0) == EINVAL
    assert call(p=1025) == EUNSUPPORTED and call(ffn=96) == EUNSUPPORTED and call(ffn=576) == EUNSUPPORTED and call(n_cls=65) == EUNSUPPORTED
    assert call(w1=ctypes.c_void_p(4100)) == EUNSUPPORTED
    assert call(ws_bytes=64) == EWORKSPACE and call(ws=None) == EWORKSPACE
