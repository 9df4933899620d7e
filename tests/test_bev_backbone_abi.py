"""CPU-side checks of the dense BEV backbone's boundary: the conv2d entry points are declared in include/lvq.h and exported by the built
library, the host-only size queries return the documented values, shapes outside the family are refused with the documented codes before
any launch (no GPU is present here), and the registries carry the reference's NAME strings."""
import ctypes
import os

import pytest

from lidar_vision_vqa_amd import _ffi

SYMBOLS = ("lvq_conv2d_plane_elems", "lvq_conv2d_out_size", "lvq_conv2d_to_planes", "lvq_conv2d_packed_elems", "lvq_conv2d_pack_weights",
           "lvq_conv2d", "lvq_deconv2d")
EINVAL, EUNSUPPORTED = -1, -5
C = ctypes.c_int
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_ffi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = _ffi.lib()
    L.lvq_conv2d_plane_elems.restype = ctypes.c_size_t
    L.lvq_conv2d_packed_elems.restype = ctypes.c_size_t
    return L


def test_symbols_are_declared_and_exported(lib):
    declared = _ffi.declared_symbols()
    for s in SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s


def test_size_queries(lib):
    # planes: batch * h * w * (c rounded up to 32)
    assert lib.lvq_conv2d_plane_elems(C(2), C(64), C(16), C(24)) == 2 * 16 * 24 * 64
    assert lib.lvq_conv2d_plane_elems(C(1), C(5), C(3), C(3)) == 9 * 32
    assert lib.lvq_conv2d_plane_elems(C(1), C(384), C(8), C(8)) == 64 * 384
    assert lib.lvq_conv2d_plane_elems(C(1), C(513), C(8), C(8)) == 0 and lib.lvq_conv2d_plane_elems(C(0), C(64), C(8), C(8)) == 0
    # torch's output sizes: kernel 3 / padding 1 -> floor((H - 1) / s) + 1; kernel = stride -> floor(H / s)
    for h in (1, 2, 7, 8, 9, 16, 17, 33):
        for s in (1, 2):
            assert lib.lvq_conv2d_out_size(C(h), C(3), C(s)) == (h - 1) // s + 1 == (h + 2 - 3) // s + 1
        for s in (1, 2, 4):
            assert lib.lvq_conv2d_out_size(C(h), C(s), C(s)) == h // s
    assert lib.lvq_conv2d_out_size(C(8), C(3), C(4)) == EUNSUPPORTED and lib.lvq_conv2d_out_size(C(8), C(5), C(1)) == EUNSUPPORTED
    assert lib.lvq_conv2d_out_size(C(8), C(2), C(1)) == EUNSUPPORTED and lib.lvq_conv2d_out_size(C(0), C(3), C(1)) == EINVAL
    # packed weights: (c_in rounded up to 32) * kernel^2 * c_out per part
    for cin, cout in ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (384, 384), (512, 512), (5, 64), (40, 128)):
        cp = (cin + 31) // 32 * 32
        assert lib.lvq_conv2d_packed_elems(C(cout), C(cin), C(3), C(0)) == cp * 9 * cout
        for s in (1, 2, 4):
            assert lib.lvq_conv2d_packed_elems(C(cout), C(cin), C(s), C(0)) == cp * s * s * cout
            assert lib.lvq_conv2d_packed_elems(C(cout), C(cin), C(s), C(1)) == cp * s * s * cout
    for cin, cout in ((64, 48), (64, 32), (64, 576), (0, 64), (513, 64), (64, 96)):
        assert lib.lvq_conv2d_packed_elems(C(cout), C(cin), C(3), C(0)) == 0, (cin, cout)
    assert lib.lvq_conv2d_packed_elems(C(64), C(64), C(5), C(0)) == 0 and lib.lvq_conv2d_packed_elems(C(64), C(64), C(3), C(1)) == 0


def conv(lib, *, c_in=64, c_out=64, kernel=3, stride=1, h=8, w=8, batch=1, in_lo=0, w_lo=0, scale=0, shift=0, out_hi=256, out_lo=0, out_f32=0,
         c_total=None, c_off=0, in_hi=256, w_hi=256):
    """The argument checks run before anything is dereferenced or launched: pointers here are fake, 16-byte aligned addresses."""
    return lib.lvq_conv2d(P(in_hi), P(in_lo), C(batch), C(h), C(w), C(c_in), P(w_hi), P(w_lo), C(c_out), C(kernel), C(stride), P(scale), P(shift),
                          C(1), P(out_hi), P(out_lo), P(out_f32), C(c_out if c_total is None else c_total), C(c_off), P(0))


def deconv(lib, *, c_in=64, c_out=64, stride=2, h=8, w=8, c_total=None, c_off=0, out_hi=256):
    return lib.lvq_deconv2d(P(256), P(0), C(1), C(h), C(w), C(c_in), P(256), P(0), C(c_out), C(stride), P(0), P(0), C(1), P(out_hi), P(0), P(0),
                            C(c_out if c_total is None else c_total), C(c_off), P(0))


def test_unsupported_shapes_and_inconsistent_calls_are_refused_before_any_launch(lib):
    for kw in (dict(c_out=48), dict(c_out=96), dict(c_out=576), dict(c_in=513), dict(kernel=3, stride=4), dict(kernel=5, stride=1),
               dict(kernel=2, stride=1), dict(kernel=4, stride=2), dict(batch=65536), dict(in_hi=264)):
        assert conv(lib, **kw) == EUNSUPPORTED, kw
    for kw in (dict(h=0), dict(c_in=0), dict(c_out=0), dict(batch=0), dict(stride=0), dict(in_hi=0), dict(w_hi=0), dict(out_hi=0),
               dict(scale=256), dict(shift=256), dict(in_lo=256), dict(w_lo=256), dict(out_hi=0, out_lo=256, out_f32=256),
               dict(c_total=128, c_off=65), dict(c_total=32), dict(c_off=-1), dict(kernel=4, stride=4, h=3)):
        assert conv(lib, **kw) == EINVAL, kw
    assert deconv(lib, stride=3) == EUNSUPPORTED and deconv(lib, stride=8) == EUNSUPPORTED and deconv(lib, c_out=32) == EUNSUPPORTED
    assert deconv(lib, stride=0) == EINVAL and deconv(lib, c_total=64, c_off=1) == EINVAL and deconv(lib, out_hi=0) == EINVAL
    assert lib.lvq_conv2d_to_planes(P(256), C(1), C(513), C(8), C(8), P(256), P(0), P(0)) == EUNSUPPORTED
    assert lib.lvq_conv2d_to_planes(P(0), C(1), C(64), C(8), C(8), P(256), P(0), P(0)) == EINVAL
    assert lib.lvq_conv2d_pack_weights(P(256), C(48), C(64), C(3), C(0), P(256), P(0), P(0)) == EUNSUPPORTED
    assert lib.lvq_conv2d_pack_weights(P(0), C(64), C(64), C(3), C(0), P(256), P(0), P(0)) == EINVAL


def test_registries_carry_the_reference_s_names():
    from lidar_vision_vqa_amd import backbone2d, bev, lidar
    assert backbone2d.backbones_2d_all == {"BaseBEVBackbone": backbone2d.BaseBEVBackbone, "BaseBEVBackboneV1": backbone2d.BaseBEVBackboneV1}
    assert lidar.map_to_bev_all["HeightCompression"] is bev.HeightCompression
    assert lidar.map_to_bev_all["PointPillarScatter"] is lidar.PointPillarScatter


def test_module_refuses_cpu_tensors_and_train_mode():
    import torch
    import bev_backbone_cases as BC
    from lidar_vision_vqa_amd import backbone2d
    m = backbone2d.BaseBEVBackbone(BC.case_cfg("nusc_second"), 256)
    with pytest.raises(_ffi.LvqError), torch.no_grad():
        m(dict(spatial_features=torch.zeros(1, 256, 16, 16)))                   # train() mode
    with pytest.raises(_ffi.LvqError), torch.no_grad():
        m.eval()(dict(spatial_features=torch.zeros(1, 256, 16, 16)))            # CPU tensor: no fallback
