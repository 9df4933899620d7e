"""_ffi.version_of / _ffi.derived: the one rule by which everything computed from weights alone is kept and rebuilt (beside
_ffi.workspace), and _ffi.fold_batchnorm.  The helper reads tensor metadata only, so all of this runs on CPU tensors."""
import glob
import os

import pytest
import torch
import torch.nn as nn

from lidar_vision_vqa_amd import _ffi as F


class Counted:
    """derived() over a module's weight with a build that counts its calls."""

    def __init__(self, mod=None):
        self.mod = mod or nn.Linear(4, 3)
        self.cache, self.calls = {}, 0

    def build(self):
        self.calls += 1
        return self.mod.weight.detach().clone()

    def get(self, key="w", extra=(), tensors=None):
        return F.derived(self.cache, key, (self.mod.weight,) if tensors is None else tensors, self.build, extra)


def test_a_hit_returns_the_same_object_without_building():
    c = Counted()
    first = c.get()
    assert c.get() is first and c.get() is first and c.calls == 1
    assert c.cache["w"] == (F.version_of((c.mod.weight,)), first) and c.cache["w"][1] is first


def _mul(c):
    with torch.no_grad():
        c.mod.weight.mul_(2.0)


def _load(c):
    c.mod.load_state_dict({k: v + 1.0 for k, v in c.mod.state_dict().items()})


def _data(c):
    c.mod.weight.data = torch.ones(3, 4)


def _double(c):
    c.mod.double()


@pytest.mark.parametrize("change", [_mul, _load, _data, _double], ids=["mul_", "load_state_dict", "data", "double"])
def test_a_changed_tensor_rebuilds_exactly_once(change):
    c = Counted()
    first = c.get()
    change(c)
    second = c.get()
    assert c.calls == 2 and second is not first and torch.equal(second, c.mod.weight.detach())
    assert c.get() is second and c.calls == 2


def test_another_shape_at_the_same_storage_rebuilds_exactly_once():
    c = Counted()
    w = c.mod.weight.detach()
    flat = w.view(12)
    assert flat.data_ptr() == w.data_ptr() and flat._version == w._version
    first = c.get(tensors=(w,))
    second = c.get(tensors=(flat,))
    assert c.calls == 2 and second is not first
    assert c.get(tensors=(flat,)) is second and c.calls == 2


def test_a_changed_extra_rebuilds_exactly_once():
    c = Counted()
    first = c.get(extra=("mixed", False))
    assert c.get(extra=("mixed", False)) is first and c.calls == 1
    second = c.get(extra=("bf16", False))
    assert c.calls == 2 and second is not first
    assert c.get(extra=("bf16", False)) is second and c.calls == 2


def test_keys_of_one_dict_do_not_disturb_each_other():
    c = Counted()
    a, b = c.get(("query_side", "mixed")), c.get(("query_side", "bf16"))
    assert c.calls == 2 and a is not b
    assert c.get(("query_side", "mixed")) is a and c.get(("query_side", "bf16")) is b and c.calls == 2
    _mul(c)
    a2 = c.get(("query_side", "mixed"))
    assert c.calls == 3 and a2 is not a and c.cache[("query_side", "bf16")][1] is b       # the other key keeps its (now old) entry
    assert c.get(("query_side", "bf16")) is not b and c.calls == 4


def test_none_tensors_are_skipped():
    lin = nn.Linear(4, 3, bias=False)
    assert F.version_of((lin.weight, lin.bias)) == F.version_of((lin.weight,)) == F.version_of((None, lin.weight, None))
    assert F.version_of((None,)) == () and F.version_of((), ("x", 1)) == ("x", 1)
    c = Counted(lin)
    first = c.get(tensors=(lin.weight, lin.bias))
    assert c.get(tensors=(lin.weight,)) is first and c.calls == 1


def test_a_raising_build_leaves_the_old_entry():
    c = Counted()
    first = c.get()
    entry = c.cache["w"]
    _mul(c)

    def broken():
        raise RuntimeError("no kernel for this shape")
    with pytest.raises(RuntimeError, match="no kernel"):
        F.derived(c.cache, "w", (c.mod.weight,), broken)
    assert c.cache["w"] is entry and c.cache["w"][1] is first
    with pytest.raises(RuntimeError):
        F.derived(c.cache, "never built", (c.mod.weight,), broken)
    assert "never built" not in c.cache
    assert c.get() is not first and c.calls == 2                   # the next good build replaces it


def test_version_of_is_a_superset_of_every_earlier_tuple():
    """Equal version_of results imply equal (data_ptr, _version) tuples -- and equal (.., shape, device) ones: no site can gain a stale
    hit from the wider tuple.  Checked over pairs of lists drawn from tensors that share storage, version counters or neither."""
    base = torch.zeros(12)
    other = torch.zeros(12)
    pool = [base, base.view(3, 4), base.view(12), base[6:], base.detach(), other, other.view(4, 3), torch.zeros(12, dtype=torch.float64)]
    with torch.no_grad():
        other.add_(1.0)                                              # _version 1 against base's 0
    narrow = lambda ts: tuple((t.data_ptr(), t._version) for t in ts)
    wide = lambda ts: tuple((t.data_ptr(), t._version, tuple(t.shape), t.device) for t in ts)
    same = 0
    for a in pool:
        for b in pool:
            for c in pool:
                x, y = [a, c], [b, c]
                if F.version_of(x) == F.version_of(y):
                    same += 1
                    assert narrow(x) == narrow(y) and wide(x) == wide(y)
                else:
                    assert wide(x) != wide(y)
    assert same > len(pool) ** 2                                     # more than the identical pairs: base / base.view(12) / base.detach()


@pytest.mark.parametrize("bn", [nn.BatchNorm1d(16), nn.BatchNorm2d(16, eps=1e-3)], ids=["1d", "2d_eps1e-3"])
def test_fold_batchnorm_is_the_expression_written_out(bn):
    g = torch.Generator().manual_seed(1905)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.1 * torch.randn(16, generator=g))
        bn.bias.copy_(0.1 * torch.randn(16, generator=g))
        bn.running_mean.copy_(torch.randn(16, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(16, generator=g))
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.float() * scale
    got = F.fold_batchnorm(bn.eval())
    assert torch.equal(got[0], scale) and torch.equal(got[1], shift)
    assert all(t.is_contiguous() and t.dtype == torch.float32 and not t.requires_grad for t in got)


def test_only_the_ffi_module_reads_version_counters():
    """An eighth hand-written variant of the rule would have to read `._version`: only _ffi.version_of does."""
    pkg = os.path.dirname(os.path.abspath(F.__file__))
    files = sorted(glob.glob(os.path.join(pkg, "*.py")))
    assert len(files) > 10
    users = [os.path.basename(f) for f in files if "._version" in open(f).read()]
    assert users == ["_ffi.py"]
