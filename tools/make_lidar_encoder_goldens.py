#!/usr/bin/env python3
"""tools/make_lidar_encoder_goldens.py -- tests/golden/lidar_pin_* from the UNMODIFIED reference classes of the LiDAR encoder's sparse
side: the five sparse backbones, HeightCompression, the four dynamic VFEs, and the chain VFE -> BACKBONE_3D -> MAP_TO_BEV ->
BACKBONE_2D of every model config under the reference's tools/cfgs/nuscenes_models/.

Runs only where the reference is mounted (tools/make_goldens.py explains the pattern: empty parent packages are registered so that
pcdet/__init__.py is never executed; weights and inputs come from seeds; only what the classes RETURN is stored, as numbers, names and
settings).  The classes import spconv and torch_scatter, which are not installed: tools/ref_standins.py registers stand-ins for the
surface they touch, and states what that leaves assumed.  The dynamic VFEs' constructors call `.cuda()`; they are built inside
ref_standins.cuda_is_identity().  base_bev_backbone.py needs the removed alias `np.int` (tools/make_bev_backbone_golden.py).

The NAME -> class registries are read from the reference's own `__init__.py` files: their `__all__` tables are parsed as data (the
files themselves import classes this path does not need and cannot load), and each class is imported from the file the table names.

Precision: the backbones, HeightCompression and the 2-D backbones run in fp64 (torch's default dtype is switched while they are built
and run), so the tests' existing bars apply to the fixtures unchanged.  The VFEs run in fp32 as they do in the reference: their
voxelisation arithmetic is part of what is pinned.  In a config's chain the VFE's fp32 result is widened to fp64 on the way into
BACKBONE_3D / MAP_TO_BEV, and kept in the fixture where a sparse backbone consumes it, so that the restated fp64 chains can start from
the same numbers.

    python tools/make_lidar_encoder_goldens.py            # rewrites tests/golden/lidar_pin_*
    python tools/make_lidar_encoder_goldens.py --check    # regenerates in memory, prints the max difference to the committed files (0)

Printed on the last run: every fixture's size, and per backbone / config the active fraction of the last sparse stage and max|out|
(asserted: each sparse stage has active and inactive sites, max|out| > 1e-2).
"""
from __future__ import annotations

import ast
import contextlib
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import bev_backbone_cases as BC  # noqa: E402
import lidar_encoder_pin_cases as P  # noqa: E402
import make_goldens as MG  # noqa: E402
import ref_standins as RS  # noqa: E402

PCDET = os.path.join(MG.REF, "lidar-encoder", "pcdet")
CFGS = os.path.join(MG.REF, "lidar-encoder", "tools", "cfgs")
PACKAGES = {"vfe": "pcdet.models.backbones_3d.vfe", "backbone_3d": "pcdet.models.backbones_3d", "map_to_bev": "pcdet.models.backbones_2d.map_to_bev",
            "backbone_2d": "pcdet.models.backbones_2d"}
MAX_BYTES = 480 * 1024


# --------------------------------------------------------------------------------------------------------------------------------
# the reference's classes
# --------------------------------------------------------------------------------------------------------------------------------
class Registry:
    """registry[NAME] -> class, as the package's `__all__` table names it; the class's file is imported on first use."""

    def __init__(self, package):
        self.package = package
        init = os.path.join(PCDET, *package.split(".")[1:], "__init__.py")
        with open(init) as f:
            tree = ast.parse(f.read())
        self.module_of, self.class_of = {}, {}
        for node in tree.body:
            if isinstance(node, ast.ImportFrom) and node.level == 1:
                for a in node.names:
                    self.module_of[a.asname or a.name] = node.module
            elif isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "__all__":
                self.class_of = {k.value: v.id for k, v in zip(node.value.keys, node.value.values)}

    def __contains__(self, name):
        return name in self.class_of

    def __getitem__(self, name):
        cls = self.class_of[name]
        return getattr(importlib.import_module(f"{self.package}.{self.module_of[cls]}"), cls)


def import_reference():
    np.int = int
    RS.install_spconv()
    RS.install_torch_scatter()
    for n in ("pcdet", "pcdet.utils", "pcdet.models", *PACKAGES.values()):
        MG._stub(n, os.path.join(PCDET, *n.split(".")[1:]))
    return {kind: Registry(package) for kind, package in PACKAGES.items()}


@contextlib.contextmanager
def fp64():
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)


def load(m, sd):
    own = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(np.asarray(sd[k])).to(v.dtype).reshape(v.shape) for k, v in own.items()}, strict=True)
    assert list(own) == list(sd), "key order differs"
    return m.eval()


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x if dtype is None else x.to(dtype)


def npy(x):
    return x.detach().cpu().numpy()


def alive(name, tensors, out, both=True):
    """A dead or saturated chain must not pass vacuously: every sparse stage has active and inactive sites (`both`; the small cases of
    fixture a are the existing tests', which assert their own properties where they are built), the result is not vanishing."""
    frac = None
    for k, s in tensors.items():
        n, total = len(s.indices), s.batch_size * int(np.prod(s.spatial_shape))
        assert 0 < len(np.unique(npy(s.indices), axis=0)) < total + (not both), f"{name} {k}: {n} rows of {total} sites"
        frac = n / total
    mag = float(np.abs(out).max())
    assert mag > 1e-2, f"{name}: max|out| {mag:.3e}"
    return f"last sparse stage {frac:.3f} active, max|out| {mag:.3f}" if frac is not None else f"max|out| {mag:.3f}"


# --------------------------------------------------------------------------------------------------------------------------------
# fixture a
# --------------------------------------------------------------------------------------------------------------------------------
def backbone_fixture(R, name, returns):
    k = P.backbone_case(name)
    with fp64():
        m = load(R["backbone_3d"][k["cls"]](BC.Cfg(k["cfg"]), k["cin"], np.asarray(k["grid"])), k["sd"])
        key = "pillar" if k["cls"] in P.C.PILLAR else "voxel"
        bd = {f"{key}_features": t(k["feat"], torch.float64), f"{key}_coords": t(k["idx"]), "batch_size": k["batch"]}
        before = set(bd)
        bd = m(bd)
        arrays, st = {}, P.sparse_stages(bd, k["cls"])
        for stage in P.stage_names(k["cls"]):
            s = st[stage]
            arrays.update(P.pack_sparse(stage, npy(s.features), npy(s.indices), s.spatial_shape, multiset=stage == "merged"))
        if key == "pillar":
            out = npy(bd["multi_scale_2d_features"]["x_conv5"])
            arrays.update(P.pack_dense("x_conv4", npy(bd["multi_scale_2d_features"]["x_conv4"])))
            arrays.update(P.pack_dense("x_conv5", out))
        else:
            out = npy(bd["encoded_spconv_tensor"].features)
        returns[name] = P.returned_names(before, bd)
        if name == P.HEIGHT_COMPRESSION_OF:
            hc = R["map_to_bev"]["HeightCompression"](BC.Cfg(NUM_BEV_FEATURES=256))
            arrays.update(P.pack_dense("spatial_features", npy(hc(bd)["spatial_features"])))
            returns["HeightCompression"] = P.returned_names(before | set(returns[name]["keys"]), bd)
    return arrays, alive(name, {s: v for s, v in st.items() if s != "merged"}, out, both=False)


# --------------------------------------------------------------------------------------------------------------------------------
# dynamic VFEs
# --------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recorded_inverse(seen):
    """The classes hand their inverse map (torch.unique's) to torch_scatter and return neither it nor the counts: take both there."""
    ts = sys.modules["torch_scatter"]
    real = ts.scatter_mean, ts.scatter_max

    def wrap(f):
        def g(src, index, *a, **kw):
            seen.append(npy(index))
            return f(src, index, *a, **kw)
        return g

    ts.scatter_mean, ts.scatter_max = wrap(real[0]), wrap(real[1])
    try:
        yield
    finally:
        ts.scatter_mean, ts.scatter_max = real


def run_dynamic(R, cls, cfg, args, seed, points, batch_size):
    with RS.cuda_is_identity():
        m = R["vfe"][cls](model_cfg=BC.Cfg(cfg), **dict(args, grid_size=np.asarray(args["grid_size"]))).eval()
        if seed is not None:
            load(m, P.seeded_state(m, seed))
        seen = []
        bd = dict(points=t(points), batch_size=batch_size)
        before = set(bd)
        with recorded_inverse(seen):
            bd = m(bd)
    assert seen and all(np.array_equal(seen[0], s) for s in seen)
    return bd, before, seen[0]


def dynamic_fixture(R, name, returns):
    cls, cfg, args, kind, seed = P.dynamic_setup(name)
    bd, before, inv = run_dynamic(R, cls, cfg, args, seed, P.dynamic_points(), P.DYN_POINTS[0])
    coords = npy(bd["pillar_coords" if kind == "simple2d" else "voxel_coords"])
    feats = npy(bd["voxel_features" if kind == "mean" else "pillar_features"])
    assert feats.dtype == np.float32 and len(feats) == len(coords) == int(inv.max()) + 1 and 0 < len(inv) < len(P.dynamic_points())
    returns["dyn_" + name] = P.returned_names(before, bd)
    arrays = dict(coords=coords.astype(np.int32), unq_inv=inv.astype(np.int32), unq_cnt=np.bincount(inv, minlength=len(coords)).astype(np.int32),
                  **P.pack("features", feats))
    return arrays, f"{len(inv)} of {len(P.dynamic_points())} points in {len(coords)} cells, max|out| {np.abs(feats).max():.3f}"


# --------------------------------------------------------------------------------------------------------------------------------
# fixture c
# --------------------------------------------------------------------------------------------------------------------------------
def read_settings():
    """{config file name: LiDAR-encoder settings}, settings only: the four module tables, the voxeliser's sizes and caps (the `test`
    entry), the range and the point feature list, each from the model file or, where it does not set it, from its _BASE_CONFIG_."""
    import yaml
    folder = os.path.join(CFGS, "nuscenes_models")
    out = {}
    for fn in sorted(os.listdir(folder)):
        with open(os.path.join(folder, fn)) as f:
            c = yaml.safe_load(f)
        data = c["DATA_CONFIG"]
        with open(os.path.join(CFGS, "..", data["_BASE_CONFIG_"])) as f:
            base = yaml.safe_load(f)
        procs = data.get("DATA_PROCESSOR", base["DATA_PROCESSOR"])             # a model file's list replaces the base's
        vox = next(p for p in procs if p["NAME"].startswith("transform_points_to_voxels"))
        enc = data.get("POINT_FEATURE_ENCODING", base["POINT_FEATURE_ENCODING"])
        s = {k: c["MODEL"].get(k) for k in ("VFE", "BACKBONE_3D", "MAP_TO_BEV", "BACKBONE_2D")}
        s.update(MODEL=c["MODEL"]["NAME"], voxel_size=vox["VOXEL_SIZE"], point_cloud_range=data.get("POINT_CLOUD_RANGE", base["POINT_CLOUD_RANGE"]),
                 used_feature_list=enc["used_feature_list"], num_point_features=len(enc["used_feature_list"]),
                 max_points_per_voxel=vox.get("MAX_POINTS_PER_VOXEL"), max_voxels=(vox.get("MAX_NUMBER_OF_VOXELS") or {}).get("test"))
        out[fn[:-len(".yaml")]] = s
    return out


def config_fixture(R, name, s, returns):
    inp = P.config_input(s)
    arrays, sparse, names = {}, {}, {}
    hard = s["VFE"]["NAME"] in P.HARD_VFES
    if hard:
        bd = dict(voxels=t(inp["voxels"]), voxel_num_points=t(inp["voxel_num_points"]).float(), voxel_coords=t(inp["voxel_coords"]).float(),
                  batch_size=inp["batch_size"])
        arrays["checksum"] = np.int64(inp["checksum"])
        arrays["n_voxels"] = np.int64(len(inp["voxel_coords"]))
    else:
        bd = dict(points=t(inp["points"]), batch_size=inp["batch_size"])
    before = set(bd)
    with RS.cuda_is_identity():
        chain = P.build_chain(s, R)
    for stage, m in chain:
        names[stage] = P.names_of(m, whole=False)
        if stage == "vfe":
            load(m, P.seeded_state(m, P.CFG_SEED[stage])) if len(m.state_dict()) else m.eval()
            bd = m(bd)
            nxt = chain[1][0]
            if not hard:
                key = "pillar_coords" if "pillar_coords" in bd else "voxel_coords"
                arrays["vfe.coords"] = npy(bd[key]).astype(np.int32)
            for key in ("voxel_features", "pillar_features"):
                if key in bd:
                    f = npy(bd[key])
                    assert f.dtype == np.float32
                    # a sparse backbone's restated chain starts from these numbers: kept whole; else packed for the VFE's own check
                    arrays.update({"vfe.features_whole": f} if nxt == "backbone_3d" else P.pack("vfe.features", f))
                    bd[key] = bd[key].double()
                    if "voxel_features" in bd and "pillar_features" in bd:
                        bd["voxel_features"] = bd["pillar_features"] = bd[key]
                    break
            continue
        with fp64():
            m = m.double()
            load(m, P.seeded_state(m, P.CFG_SEED[stage])) if len(m.state_dict()) else m.eval()
            bd = m(bd)
        if stage == "backbone_3d":
            cls = s["BACKBONE_3D"]["NAME"]
            sparse = P.sparse_stages(bd, cls)
            for k, v in sparse.items():
                o = P.ascending(npy(v.indices), npy(v.features) if k == "merged" else None)
                arrays[f"{k}.idx"] = npy(v.indices)[o].astype(np.int16 if int(npy(v.indices).max()) < 32768 else np.int32)
                arrays[f"{k}.shape"] = np.asarray(v.spatial_shape, np.int32)
    if "spatial_features_2d" in bd:
        out = npy(bd["spatial_features_2d"])
        arrays.update(P.pack_dense("spatial_features_2d", out))
    else:
        e = bd["encoded_spconv_tensor"]
        out = npy(e.features)
        arrays.update(P.pack_sparse("out", out, npy(e.indices), e.spatial_shape))
    returns["cfg_" + name] = dict(P.returned_names(before, bd), modules=names)
    return arrays, alive(name, {k: v for k, v in sparse.items() if k != "merged"}, out)


# --------------------------------------------------------------------------------------------------------------------------------
def generate():
    """{file name under tests/golden/: dict of arrays (.npz) or a JSON-able object (.json)}."""
    R = import_reference()
    files, returns, notes = {}, {}, {}
    for name in P.BACKBONES:
        files[f"{P.PREFIX}{name}.npz"], notes[name] = backbone_fixture(R, name, returns)
    for name in P.DYNAMIC:
        files[f"{P.PREFIX}dyn_{name}.npz"], notes["dyn_" + name] = dynamic_fixture(R, name, returns)
    settings = read_settings()
    for name, s in settings.items():
        files[f"{P.PREFIX}cfg_{name}.npz"], notes["cfg_" + name] = config_fixture(R, name, s, returns)
    modules = {}
    for variant in P.NAME_VARIANTS:
        with RS.cuda_is_identity():
            modules[variant] = P.names_of(P.construct(R, variant))
    files[f"{P.PREFIX}names.json"] = dict(modules=modules, returns=returns,
                                          registries={kind: sorted(R[kind].class_of) for kind in R})
    files[f"{P.PREFIX}configs.json"] = settings
    return files, notes


def as_json(obj):
    return json.dumps(obj, indent=1, sort_keys=True) + "\n"


def difference(path, new):
    if path.endswith(".json"):
        with open(path) as f:
            return 0.0 if f.read() == as_json(new) else float("inf")
    old = np.load(path)
    if sorted(old.files) != sorted(new):
        return float("inf")
    worst = 0.0
    for k in new:
        a, b = np.asarray(new[k]), old[k]
        if a.shape != b.shape or a.dtype != b.dtype:
            return float("inf")
        if a.size:
            worst = max(worst, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))
    return worst


@torch.no_grad()
def main():
    check = "--check" in sys.argv
    torch.set_num_threads(8)
    files, notes = generate()
    worst = 0.0
    for fn, content in files.items():
        path = os.path.join(MG.OUT, fn)
        if check:
            d = difference(path, content) if os.path.exists(path) else float("inf")
            worst = max(worst, d)
            print(f"  {fn:60s} max difference {d:g}")
            continue
        if fn.endswith(".json"):
            with open(path, "w") as f:
                f.write(as_json(content))
        else:
            np.savez_compressed(path, **content)
        size = os.path.getsize(path)
        print(f"  {fn:60s} {size / 1024:6.0f} KiB   {notes.get(fn[len(P.PREFIX):-4], '')}")
        assert size < MAX_BYTES, f"{fn}: {size} bytes"
    if check:
        stale = sorted(f for f in os.listdir(MG.OUT) if f.startswith(P.PREFIX) and f not in files)
        print(f"max difference to the committed fixtures: {worst:g}" + (f"; not regenerated: {stale}" if stale else ""))
        sys.exit(0 if worst == 0.0 and not stale else 1)
    print("done")


if __name__ == "__main__":
    main()
