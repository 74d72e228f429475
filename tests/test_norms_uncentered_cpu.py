"""The uncentered position / group / all norms from outside, without a device: the names `bcos.modules.norms` exports, what the classes
look like (against tests/golden/unorms_surface.json, recorded from the reference's own classes by tests/golden/make_golden_unorms.py),
the C ABI's declarations and prototypes, and the argument errors the entry points return before any HIP call.
"""
import ctypes as C
import importlib
import inspect
import json
import os
import re

import pytest
import torch

NAMES = ["PositionNormUncentered2d", "GroupNormUncentered2d", "GNInstanceNormUncentered2d", "GNLayerNormUncentered2d",
         "AllNormUncentered2d", "group_norm_uncentered"]
ENTRY_POINTS = ["bcos_layernorm_unc_fwd", "bcos_layernorm_unc_bwd_detached", "bcos_layernorm_unc_bwd",
                "bcos_groupnorm_unc_fwd", "bcos_groupnorm_unc_bwd_detached", "bcos_groupnorm_unc_bwd"]
BASES = ("LayerNorm", "GroupNorm", "BatchNorm2d", "DetachableModule", "GroupNormUncentered2d")
ATTRS = ("normalized_shape", "num_groups", "num_channels", "num_features", "momentum", "affine", "elementwise_affine",
         "track_running_stats", "features")


@pytest.fixture(scope="module")
def recorded(golden_dir):
    with open(os.path.join(golden_dir, "unorms_surface.json")) as f:
        return json.load(f)


def _defaults(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def test_all_six_names_import_from_the_norms_package():
    import bcos.modules.norms as norms
    for name in NAMES:
        assert hasattr(norms, name), name
        assert name in norms.uncentered_norms.__dict__, name
    from bcos.modules.norms import (AllNormUncentered2d, GNInstanceNormUncentered2d, GNLayerNormUncentered2d,  # noqa: F401
                                    GroupNormUncentered2d, PositionNormUncentered2d, group_norm_uncentered)
    assert "BatchNormUncentered2d" in norms.__dict__ and "DetachablePositionNorm2d" in norms.__dict__      # and nothing went away


def test_module_files_export_what_the_reference_exports(recorded):
    for mod, names in recorded["uncentered_norms.__all__"].items():
        ours = importlib.import_module("bcos.modules.norms.uncentered_norms." + mod)
        assert list(ours.__all__) == names, mod
    fa = importlib.import_module("bcos.modules.norms.uncentered_norms.allnorm_uncentered").all_norm_uncentered_2d
    fg = importlib.import_module("bcos.modules.norms.uncentered_norms.groupnorm_uncentered").group_norm_uncentered
    assert _defaults(fa) == recorded["all_norm_uncentered_2d"] and _defaults(fg) == recorded["group_norm_uncentered"]


@pytest.mark.parametrize("cls_name", NAMES[:5])
def test_class_looks_like_the_reference_class(recorded, cls_name):
    import bcos.modules.norms as norms
    want = recorded[cls_name]
    cls = getattr(norms, cls_name)
    args = want["args"]
    m = cls(*args)
    assert [b.__name__ for b in cls.__mro__[1:] if b.__name__ in BASES] == want["bases"]
    sig = inspect.signature(cls.__init__)
    assert [[n, str(p.kind), None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in sig.parameters.items()] == want["init"]
    assert m.eps == want["eps"] and bool(m.detach) == want["detach_default"]
    assert {n: list(p.shape) for n, p in m.named_parameters()} == want["parameters"]
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == want["state_dict"]
    assert list(m.state_dict().keys()) == list(want["state_dict"].keys())
    for attr in ATTRS:
        assert hasattr(m, attr) == (attr in want), attr
        if attr in want:
            v = getattr(m, attr)
            assert (list(v) if isinstance(v, tuple) else v) == want[attr], attr
    for wrap, key in ((norms.NoBias, "nobias"), (norms.Unaffine, "unaffine")):
        w = wrap(cls)(*args)
        assert w._get_name() == want[key]["name"] and wrap(cls).__name__ == want[key]["factory"]
        assert list(w.state_dict().keys()) == want[key]["state_dict"]
        assert w.bias is None and (w.weight is None) == (key == "unaffine")
    m.set_explanation_mode(True)
    assert m.detach and m.is_in_explanation_mode


def test_all_norm_tracks_its_statistics_like_a_batch_norm_over_one_feature():
    from bcos.modules.norms import AllNormUncentered2d
    m = AllNormUncentered2d(64, eps=1e-3, momentum=None, affine=False, track_running_stats=True)
    assert m.num_features == 1 and m.momentum is None and m.weight is None and tuple(m.running_var.shape) == (1,)
    assert int(m.num_batches_tracked) == 0 and m.eps == 1e-3
    m = AllNormUncentered2d(64, track_running_stats=False)
    assert m.running_var is None and m.num_batches_tracked is None and tuple(m.weight.shape) == (1,)


def test_modules_have_no_cpu_fallback():
    from bcos.modules.norms import AllNormUncentered2d, GroupNormUncentered2d, PositionNormUncentered2d
    from bcos_hip.lib import BcosHipError
    x = torch.randn(2, 8, 3, 3)
    for m in (PositionNormUncentered2d(8), GroupNormUncentered2d(2, 8), AllNormUncentered2d(8), AllNormUncentered2d(8).eval()):
        with pytest.raises(BcosHipError):
            m(x)


def test_header_sources_and_prototypes():
    from bcos_hip import lib
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(os.path.dirname(here), "include", "bcos_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in lib.SIGNATURES, name
        decl = re.search(r"^int " + name + r"\((.*?)\);", header, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[name][1]), name              # one ctypes type per declared argument
    assert "bcos_norms.hip" in lib.SOURCES and (lib.CSRC / "bcos_norms.hip").exists()
    for ref in ("posnorm_uncentered.py:39-58", "groupnorm_uncentered.py:21-61"):       # the declarations carry the reference's file:line
        assert ref in header, ref
    assert lib.ABI_VERSION == 12 and re.search(r"#define\s+BCOS_ABI_VERSION\s+12\b", header)
    from bcos_hip import ops
    for name in ENTRY_POINTS:               # reached through the wrapper of the centred operation, `centered=False`
        wrapper = getattr(ops, name[len("bcos_"):].replace("_unc_", "_"))
        assert callable(wrapper) and inspect.signature(wrapper).parameters["centered"].default is True, name
        assert not hasattr(ops, name[len("bcos_"):]), name


def test_argument_errors_return_inval_without_a_device(hip_lib):
    from bcos_hip import lib as blib
    lib = hip_lib
    p = C.c_void_p(4096)          # never dereferenced: every call below is refused before any HIP call
    calls = {
        "fwd NULL x": lambda: lib.bcos_layernorm_unc_fwd(None, p, p, p, p, 4, 8, 1e-5, None),
        "fwd NULL y": lambda: lib.bcos_layernorm_unc_fwd(p, p, p, None, p, 4, 8, 1e-5, None),
        "fwd rows=0": lambda: lib.bcos_layernorm_unc_fwd(p, p, p, p, p, 0, 8, 1e-5, None),
        "fwd D=-1": lambda: lib.bcos_layernorm_unc_fwd(p, p, p, p, p, 4, -1, 1e-5, None),
        "bwd_detached NULL gy": lambda: lib.bcos_layernorm_unc_bwd_detached(None, p, p, None, None, p, p, 4, 8, None),
        "bwd_detached NULL rstd": lambda: lib.bcos_layernorm_unc_bwd_detached(p, p, None, None, None, p, p, 4, 8, None),
        "bwd_detached no output": lambda: lib.bcos_layernorm_unc_bwd_detached(p, p, p, None, None, None, None, 4, 8, None),
        "bwd_detached rows=0": lambda: lib.bcos_layernorm_unc_bwd_detached(p, p, p, None, None, p, p, 0, 8, None),
        "bwd NULL x": lambda: lib.bcos_layernorm_unc_bwd(p, None, p, p, None, p, p, 4, 8, None),
        "bwd NULL gx": lambda: lib.bcos_layernorm_unc_bwd(p, p, p, p, None, None, p, 4, 8, None),
        "bwd D=0": lambda: lib.bcos_layernorm_unc_bwd(p, p, p, p, None, p, p, 4, 0, None),
        "group fwd C=6 G=4": lambda: lib.bcos_groupnorm_unc_fwd(p, p, p, p, p, 2, 8, 6, 4, 1e-5, None),
        "group fwd NULL y": lambda: lib.bcos_groupnorm_unc_fwd(p, p, p, None, p, 2, 8, 8, 4, 1e-5, None),
        "group fwd N=0": lambda: lib.bcos_groupnorm_unc_fwd(p, p, p, p, p, 0, 8, 8, 4, 1e-5, None),
        "group bwd_detached C=6 G=4": lambda: lib.bcos_groupnorm_unc_bwd_detached(p, p, p, p, 2, 8, 6, 4, None),
        "group bwd_detached NULL rstd": lambda: lib.bcos_groupnorm_unc_bwd_detached(p, p, None, p, 2, 8, 8, 4, None),
        "group bwd_detached G=0": lambda: lib.bcos_groupnorm_unc_bwd_detached(p, p, p, p, 2, 8, 8, 0, None),
        "group bwd C=6 G=4": lambda: lib.bcos_groupnorm_unc_bwd(p, p, p, p, p, p, 2, 8, 6, 4, None),
        "group bwd NULL x": lambda: lib.bcos_groupnorm_unc_bwd(p, None, p, p, p, p, 2, 8, 8, 4, None),
        "group bwd HW=0": lambda: lib.bcos_groupnorm_unc_bwd(p, p, p, p, p, p, 2, 0, 8, 4, None),
    }
    for what, call in calls.items():
        rc = call()
        assert rc == blib.BCOS_E_INVAL, (what, rc)
        assert lib.bcos_last_error_string().decode().startswith("bcos_"), what
