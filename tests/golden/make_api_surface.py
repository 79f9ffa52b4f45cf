"""Generates tests/golden/api_surface.json by SCANNING the reference's Python and binding sources.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_api_surface.py <checkout of the reference project>
(the tests run without the reference tree, which is why the result is committed).

What is captured -- names and parameter counts only, no reference source (tests/test_api_surface.py reads it):
  droid_backends_attrs   every `droid_backends.<name>` in dbaf/**/*.py and the top-level scripts
  lietorch_imports       every name of a `from lietorch import ...`
  se3_attrs              the SE3 methods / attributes called on pose objects
  corr_signatures        the parameter lists of the public methods of dbaf/modules/corr.py's four classes
  bindings               src/droid.cpp: m.def name -> number of parameters of the bound C++ function
  bacore_methods         src/droid.cpp / src/bacore.h: BACore method name -> number of parameters (without self)
"""
import glob
import importlib.util
import inspect
import json
import os
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _sources(ref_root):
    files = glob.glob(os.path.join(ref_root, "dbaf", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ref_root, "*.py"))
    return [open(f, errors="ignore").read() for f in files]


def _ref_corr_module(ref_root):
    """the reference's dbaf/modules/corr.py imported with an empty stand-in for its native module"""
    saved = sys.modules.get("droid_backends")
    sys.modules["droid_backends"] = types.ModuleType("droid_backends")
    try:
        spec = importlib.util.spec_from_file_location("_ref_modules_corr", os.path.join(ref_root, "dbaf", "modules", "corr.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is not None:
            sys.modules["droid_backends"] = saved
        else:
            del sys.modules["droid_backends"]
    return mod


def _nargs(params):
    return len([a for a in params.split(",") if a.strip()])


def main(ref_root):
    texts = _sources(ref_root)
    attrs, imports, se3 = set(), set(), set()
    for text in texts:
        attrs |= set(re.findall(r"\bdroid_backends\.([A-Za-z_]\w*)", text))
        for names in re.findall(r"from\s+lietorch\s+import\s+([^\n]+)", text):
            imports |= {n.strip() for n in names.replace("(", "").replace(")", "").split(",") if n.strip()}
        se3 |= set(re.findall(r"\bSE3\.([A-Za-z_]\w*)", text))
        se3 |= set(re.findall(r"\bSE3\([^)]*\)\.([A-Za-z_]\w*)", text))
        se3 |= set(re.findall(r"\b(?:Gs?|Gij|Gi|Gj|poses|Ps?|dP|d)\s*(?:\[[^\]]*\])?\.(inv|retr|adjT|adj|matrix|translation|data|log|exp|scale|vec|cpu|act)\b", text))

    ref = _ref_corr_module(ref_root)
    corr = {}
    for cls in ("CorrBlock", "AltCorrBlock", "CorrSampler", "CorrLayer"):
        corr[cls] = {}
        for name, member in inspect.getmembers(getattr(ref, cls), predicate=inspect.isfunction):
            if name.startswith("_") and name not in ("__init__", "__call__", "__getitem__"):
                continue
            corr[cls][name] = list(inspect.signature(member).parameters)

    text = open(os.path.join(ref_root, "src", "droid.cpp")).read()
    bindings = {}
    for pyname, cname in re.findall(r'm\.def\("(\w+)",\s*&(\w+)', text):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*\{" % cname, text)
        bindings[pyname] = _nargs(m.group(1))
    hdr = open(os.path.join(ref_root, "src", "bacore.h")).read()
    methods = {}
    for pyname, cname in re.findall(r'\.def\("(\w+)",\s*&BACore::(\w+)\)', text):
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % cname, hdr)
        methods[pyname] = _nargs(m.group(1))

    out = {"droid_backends_attrs": sorted(attrs), "lietorch_imports": sorted(imports), "se3_attrs": sorted(se3),
           "corr_signatures": corr, "bindings": bindings, "bacore_methods": methods}
    with open(os.path.join(HERE, "api_surface.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
