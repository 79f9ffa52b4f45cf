"""Records graph states before and after the reference's OWN CovisibleGraph.add_factors (dbaf/covisible_graph.py:102-149)
-- data only -- by running its Python on the CPU in the authoring container, as make_factor_edits.py does for the
retirement calls.

The class is imported from /root/reference at run time; absent third-party modules are replaced by inert stand-ins.  The
method is called unbound on an attribute holder carrying exactly what it reads: the graph's tensors, `device`,
`max_factors`, `corr_impl` and a `video` with nets, inps, fmaps and `reproject` bound to a deterministic function of
(ii, jj) (tests/add_factors_model.py::make_golden_reproject).  The module's CorrBlock name is bound to a recorder that
keeps the two map operands it is given and answers cat / __getitem__ on them, so the recorded "corr" is the pair of
operand rows per edge.  Nothing of the reference is copied.  Payload values are small integers on 3 x 4 maps, so the
compressed file stays small.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_add_factors_golden.py

Cases: some proposals filtered; none filtered; all filtered (nothing assigned); an eviction with pairwise distinct ages
(where the reference's argsort order is defined); n_new > max_factors (a negative limit); the first call (corr, net, inp
None); a stereo edge with two-camera fmaps; remove=False over the limit (no eviction).
tests/test_add_factors_model.py holds the numpy model against the file; tests/test_gpu_add_factors.py replays it on the
device.
"""
import importlib
import os
import sys
import types
import warnings
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference/dbaf"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

from add_factors_model import GRAPH_KEYS, VIDEO_KEYS, make_golden_reproject  # noqa: E402

H, W, C, FRAMES = 3, 4, 8, 9


def _import_with_stand_ins(name):
    """import `name` from the reference; every module it wants and this machine lacks becomes a MagicMock"""
    for _ in range(64):
        try:
            return importlib.import_module(name)
        except ImportError as e:
            missing = getattr(e, "name", None)
            if not missing or missing == name:
                raise
            sys.modules[missing] = mock.MagicMock()
    raise RuntimeError("too many missing modules while importing %s" % name)


def _np(t):
    return None if t is None else np.array(t.detach().cpu().numpy(), copy=True, order="C")


class RecordingCorr:
    """stands where the module's CorrBlock stands: keeps the operands, edits them as the real block edits its volumes"""

    def __init__(self, fmap1, fmap2):
        self.f1, self.f2 = fmap1, fmap2

    def cat(self, other):
        self.f1, self.f2 = torch.cat([self.f1, other.f1], 1), torch.cat([self.f2, other.f2], 1)
        return self

    def __getitem__(self, index):
        self.f1, self.f2 = self.f1[:, index], self.f2[:, index]
        return self


def make_graph(CovisibleGraph, seed, edges, inactive, ages, max_factors, cams=1, first=False):
    g = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *shape, dtype=torch.float32):
        return torch.randint(lo, hi, shape, generator=g).to(dtype)

    n, n_inac, B = len(edges), len(inactive), FRAMES + 1
    lst = lambda es, k: torch.tensor([e[k] for e in es], dtype=torch.long)  # noqa: E731
    graph = object.__new__(CovisibleGraph)
    graph.device, graph.corr_impl, graph.max_factors = "cpu", "volume", max_factors
    graph.ii, graph.jj, graph.age = lst(edges, 0), lst(edges, 1), torch.tensor(ages, dtype=torch.long)
    graph.target, graph.weight = ints(-9, 9, 1, n, H, W, 2), ints(0, 5, 1, n, H, W, 2)
    graph.ii_inac, graph.jj_inac = lst(inactive, 0), lst(inactive, 1)
    graph.target_inac, graph.weight_inac = ints(-9, 9, 1, n_inac, H, W, 2), ints(0, 5, 1, n_inac, H, W, 2)
    reproject = make_golden_reproject(H, W)
    graph.video = types.SimpleNamespace(
        nets=ints(-4, 4, B, C, H, W, dtype=torch.half), inps=ints(-4, 4, B, C, H, W, dtype=torch.half),
        fmaps=ints(-4, 4, B, cams, C, H, W, dtype=torch.half),
        reproject=lambda ii, jj: (torch.from_numpy(reproject(ii.numpy(), jj.numpy())), None))
    if first:
        graph.corr, graph.net, graph.inp = None, None, None
    else:
        graph.net, graph.inp = ints(-4, 4, 1, n, C, H, W, dtype=torch.half), ints(-4, 4, 1, n, C, H, W, dtype=torch.half)
        c = (graph.ii == graph.jj).long()
        graph.corr = RecordingCorr(graph.video.fmaps[graph.ii, 0][None], graph.video.fmaps[graph.jj, c][None])
    return graph


def snapshot(graph):
    st = {k: _np(getattr(graph, k)) for k in GRAPH_KEYS if not k.startswith("corr")}
    st["corr_f1"] = None if graph.corr is None else _np(graph.corr.f1)
    st["corr_f2"] = None if graph.corr is None else _np(graph.corr.f2)
    return st


def main():
    torch.manual_seed(0)
    cg = _import_with_stand_ins("covisible_graph")
    cg.CorrBlock = RecordingCorr
    CovisibleGraph = cg.CovisibleGraph
    out, cases = {}, []
    act = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 4), (4, 2), (3, 5), (5, 3)]
    inac = [(0, 2), (2, 0), (0, 3)]
    distinct = [7, 3, 11, 0, 5, 9, 2, 4]
    #        name               proposal                                         remove max_factors cams first
    table = [("some_filtered", [(5, 6), (1, 2), (6, 5), (0, 3), (6, 7), (6, 5)], False, 48, 1, False),
             ("none_filtered", [(5, 6), (6, 5), (6, 7)], False, 48, 1, False),
             ("all_filtered", [(1, 2), (0, 3), (5, 3)], True, 4, 1, False),
             ("eviction_distinct_ages", [(5, 6), (6, 5), (1, 2), (6, 7)], True, 9, 1, False),
             ("more_new_than_max_factors", [(5, 6), (6, 5), (6, 7), (7, 6)], True, 3, 1, False),
             ("first_call", [(0, 1), (1, 0), (1, 2)], False, 48, 1, True),
             ("stereo_edge", [(6, 6), (5, 6), (2, 2)], False, 48, 2, False),
             ("over_limit_without_remove", [(5, 6), (6, 5), (6, 7)], False, 9, 1, False)]
    for seed, (name, prop, remove, max_factors, cams, first) in enumerate(table):
        graph = make_graph(CovisibleGraph, 10 + seed, [] if first else act, [] if first else inac,
                           [] if first else distinct, max_factors, cams=cams, first=first)
        before = snapshot(graph)
        ii = torch.tensor([e[0] for e in prop], dtype=torch.long)
        jj = torch.tensor([e[1] for e in prop], dtype=torch.long)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")   # (autocast without a device)
            graph.add_factors(ii, jj, remove=remove)
        after = snapshot(graph)
        cases.append(name)
        for tag, st in (("before", before), ("after", after)):
            for k, v in st.items():
                if v is not None:
                    out["%s/%s/%s" % (name, tag, k)] = v
        for k in VIDEO_KEYS:
            out["%s/video/%s" % (name, k)] = _np(getattr(graph.video, k))
        for k, v in dict(ii=_np(ii), jj=_np(jj), remove=remove, max_factors=max_factors).items():
            out["%s/arg/%s" % (name, k)] = np.asarray(v)
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "add_factors.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %d arrays, %d bytes" % (path, len(cases), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
