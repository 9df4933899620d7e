"""_ffi.workspace: the one grow-only scratch cache behind every workspace the package hands to the C ABI.  What it shares decides
which calls may overlap on different streams, so the key (device, tag, stream or none) is checked here on tiny buffers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from lidar_vision_vqa_amd import _ffi as F  # noqa: E402


def test_grow_only_per_device_and_tag():
    dev = torch.device("cuda", torch.cuda.current_device())
    a = F.workspace(1000, dev, "test_grow")
    assert a.dtype == torch.uint8 and a.device == dev and a.numel() == 1000
    assert F.workspace(10, dev, "test_grow") is a and F.workspace(1000, dev, "test_grow") is a
    b = F.workspace(1001, dev, "test_grow")
    assert b is not a and b.numel() == 1001 and F.workspace(1, dev, "test_grow") is b
    assert F.workspace(8, dev, "test_grow_other") is not b


def test_floor_is_honoured_on_every_allocation():
    dev = torch.device("cuda", torch.cuda.current_device())
    a = F.workspace(16, dev, "test_floor", floor=4096)
    assert a.numel() == 4096 and F.workspace(4096, dev, "test_floor", floor=4096) is a
    b = F.workspace(5000, dev, "test_floor", floor=8192)
    assert b is not a and b.numel() == 8192
    assert F.workspace(9000, dev, "test_floor", floor=8192).numel() == 9000


def test_per_stream_separates_streams_and_the_default_shares():
    dev = torch.device("cuda", torch.cuda.current_device())
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    got = {}
    for name, s in (("s1", s1), ("s2", s2), ("s1 again", s1)):
        with torch.cuda.stream(s):
            got[name] = (F.workspace(64, dev, "test_streams", per_stream=True), F.workspace(64, dev, "test_streams"))
    assert got["s1"][0] is not got["s2"][0] and got["s1"][0].data_ptr() != got["s2"][0].data_ptr()
    assert got["s1 again"][0] is got["s1"][0]
    assert got["s1"][1] is got["s2"][1] and got["s1"][1] is not got["s1"][0]


def test_unindexed_device_is_the_current_device():
    cur = torch.cuda.current_device()
    a = F.workspace(32, torch.device("cuda"), "test_index")
    assert F.workspace(32, torch.device("cuda", cur), "test_index") is a and F.workspace(32, f"cuda:{cur}", "test_index") is a
