"""Every `droid_backends.<name>` and every `lietorch` name the reference's Python uses resolves in the adapters
(SURVEY.md section 8(b)).  The names and parameter lists the reference uses are committed vectors
(tests/golden/api_surface.json, scanned from the reference tree by tests/golden/make_api_surface.py; data only)."""
import inspect
import json
import os

import pytest


@pytest.fixture(scope="module")
def surface(golden_dir):
    with open(os.path.join(golden_dir, "api_surface.json")) as fh:
        return json.load(fh)


def test_every_droid_backends_attribute_the_reference_uses_exists(surface):
    import droid_backends
    used = set(surface["droid_backends_attrs"])
    assert {"ba", "corr_index_forward", "frame_distance", "depth_filter", "iproj"} <= used  # the scan saw the call sites
    missing = sorted(n for n in used if not hasattr(droid_backends, n))
    assert not missing, missing


def test_every_lietorch_name_the_reference_imports_exists(surface):
    import lietorch
    used = set(surface["lietorch_imports"])
    assert "SE3" in used
    missing = sorted(n for n in used if not hasattr(lietorch, n))
    assert not missing, missing
    # the SE3 methods and attributes called on pose objects in the hot path and its callers
    missing = sorted(n for n in surface["se3_attrs"] if not hasattr(lietorch.SE3, n) and n != "data")
    assert not missing, missing


def test_corr_mirrors_have_the_reference_signatures(surface):
    """dbaf_amd.corr is what INTEGRATION.md swaps in for `from modules.corr import CorrBlock, AltCorrBlock`
    (covisible_graph.py:7, motion_filter.py:8): every public name and every parameter list must match"""
    from dbaf_amd import corr as mine
    assert set(surface["corr_signatures"]) == {"CorrBlock", "AltCorrBlock", "CorrSampler", "CorrLayer"}
    for cls, members in surface["corr_signatures"].items():
        assert hasattr(mine, cls), cls
        mc = getattr(mine, cls)
        assert "__init__" in members, cls
        for name, rp in members.items():
            assert hasattr(mc, name), (cls, name)
            mp = list(inspect.signature(getattr(mc, name)).parameters)
            assert mp[:len(rp)] == rp, (cls, name, rp, mp)   # the mirror may add trailing keyword options only
            extra = [inspect.signature(getattr(mc, name)).parameters[k] for k in mp[len(rp):]]
            assert all(e.default is not inspect.Parameter.empty for e in extra), (cls, name, mp)


def _nparams(fn):
    """number of parameters of a Python function or of a pybind11 builtin (whose signature is the first docstring line)"""
    import inspect
    try:
        return len(inspect.signature(fn).parameters)
    except ValueError:
        head = fn.__doc__.splitlines()[0]
        inner = head[head.index("(") + 1:head.rindex(")")]
        return len([a for a in inner.split(",") if a.strip()]) if inner.strip() else 0


def test_droid_backends_signatures_match_the_bindings(surface):
    """src/droid.cpp: every m.def / class method bound there exists here with the same number of parameters -- in the
    package AND in the compiled adapter (csrc_ext/droid_backends_ext.cpp), which must be a drop-in by itself"""
    import droid_backends
    bound = surface["bindings"]
    assert len(bound) >= 10
    for pyname, nargs in bound.items():
        fn = getattr(droid_backends, pyname)
        assert _nparams(fn) == nargs, (pyname, nargs)
        if droid_backends.compiled is not None and pyname != "ba_extend":   # (ba_extend: debug variant, Python only)
            assert _nparams(getattr(droid_backends.compiled, pyname)) == nargs, ("compiled", pyname, nargs)
    methods = surface["bacore_methods"]
    assert set(methods) >= {"init", "hessian", "optimize", "retract"}
    for pyname, nargs in methods.items():
        fn = getattr(droid_backends.BACore, pyname)
        assert len(inspect.signature(fn).parameters) == nargs + 1, (pyname, nargs)  # + self
        if droid_backends.compiled is not None:
            assert _nparams(getattr(droid_backends.compiled.BACore, pyname)) == nargs + 1, ("compiled", pyname, nargs)
