"""Records graph states before and after the reference's OWN edge retirement -- data only -- by running its Python on
the CPU in the authoring container:

    CovisibleGraph.rm_factors(mask, store=False / True)       dbaf/covisible_graph.py:152-176
    CovisibleGraph.rm_keyframe(ix)                            dbaf/covisible_graph.py:180-211, once with an ix that an
                                                              inactive edge touches and once with one that none does
                                                              (both sides of `if torch.any(m)`)
    DBAFusionFrontend.__rollup(roll)                          dbaf/dbaf_frontend.py:84-152 (imu disabled); only the edge
                                                              lists of the graph are recorded

The classes are imported from /root/reference at run time; absent third-party modules are replaced by inert stand-ins.
The methods are called unbound on attribute holders carrying exactly what they read (the graph's tensors, a `video`
with the nine buffers and a lock, the reference's CorrBlock holding one tiny level whose rows are their own slot ids),
so no network, dataset or device is needed.  Nothing of the reference is copied.  Payload values are small integers, so
the compressed file stays small.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_factor_edits.py

tests/test_factors_model.py holds the numpy model against the file; tests/test_gpu_factors.py replays it on the device.
"""
import contextlib
import importlib
import os
import sys
import types
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference/dbaf"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

from factors_model import EDGE_KEYS, VIDEO_KEYS  # noqa: E402

H, W, C, FRAMES = 3, 4, 128, 9   # maps 3x4, net / inp channels as the reference has them


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


def make_graph(CovisibleGraph, CorrBlock, seed, n, n_inac, with_video=False):
    g = torch.Generator().manual_seed(seed)

    def ints(lo, hi, *shape, dtype=torch.float32):
        return torch.randint(lo, hi, shape, generator=g).to(dtype)

    graph = object.__new__(CovisibleGraph)
    graph.corr_impl = "volume"
    graph.ii, graph.jj = ints(0, FRAMES, n, dtype=torch.long), ints(0, FRAMES, n, dtype=torch.long)
    graph.age = ints(0, 30, n, dtype=torch.long)
    graph.target, graph.weight = ints(-9, 9, 1, n, H, W, 2), ints(0, 5, 1, n, H, W, 2)
    graph.net, graph.inp = ints(-4, 4, 1, n, C, H, W, dtype=torch.half), ints(-4, 4, 1, n, C, H, W, dtype=torch.half)
    graph.ii_inac, graph.jj_inac = ints(0, FRAMES, n_inac, dtype=torch.long), ints(0, FRAMES, n_inac, dtype=torch.long)
    graph.target_inac, graph.weight_inac = ints(-9, 9, 1, n_inac, H, W, 2), ints(0, 5, 1, n_inac, H, W, 2)
    graph.ii_bad, graph.jj_bad = ints(0, FRAMES, 3, dtype=torch.long), ints(0, FRAMES, 3, dtype=torch.long)
    corr = object.__new__(CorrBlock)
    corr.num_levels = 1
    corr.corr_pyramid = [torch.randperm(n + 5, generator=g)[:n].clone()]   # one level: row k holds edge k's slot id
    graph.corr = corr
    if with_video:
        B = FRAMES + 1
        graph.video = types.SimpleNamespace(
            images=ints(0, 256, B, 3, 8 * H, 8 * W, dtype=torch.uint8), poses=ints(-5, 5, B, 7), disps=ints(1, 9, B, H, W),
            disps_sens=ints(0, 9, B, H, W), intrinsics=ints(1, 50, B, 4), nets=ints(-4, 4, B, C, H, W, dtype=torch.half),
            inps=ints(-4, 4, B, C, H, W, dtype=torch.half), fmaps=ints(-4, 4, B, 1, C, H, W, dtype=torch.half),
            tstamp=ints(0, 1000, B, dtype=torch.float64), get_lock=contextlib.nullcontext)
    return graph


def snapshot(graph, with_video=False):
    st = {k: _np(getattr(graph, k)) for k in EDGE_KEYS if k != "corr"}
    st["corr"] = _np(graph.corr.corr_pyramid[0])
    if with_video:
        st.update({k: _np(getattr(graph.video, k)) for k in VIDEO_KEYS})
    return st


def main():
    torch.manual_seed(0)
    cg = _import_with_stand_ins("covisible_graph")
    fe = _import_with_stand_ins("dbaf_frontend")
    corr_mod = _import_with_stand_ins("modules.corr")
    CovisibleGraph, CorrBlock, Frontend = cg.CovisibleGraph, corr_mod.CorrBlock, fe.DBAFusionFrontend
    out, cases = {}, []

    def record(case, before, after, **args):
        cases.append(case)
        for tag, st in (("before", before), ("after", after)):
            for k, v in st.items():
                if v is not None:
                    out["%s/%s/%s" % (case, tag, k)] = v
        for k, v in args.items():
            out["%s/arg/%s" % (case, k)] = np.asarray(v)

    # ---- rm_factors, store=False and store=True ---------------------------------------------------------------------
    for case, store, seed in (("rm_factors_drop", False, 1), ("rm_factors_store", True, 2)):
        graph = make_graph(CovisibleGraph, CorrBlock, seed, n=10, n_inac=4)
        mask = torch.tensor([0, 1, 0, 0, 1, 1, 0, 0, 0, 1], dtype=torch.bool)
        before = snapshot(graph)
        graph.rm_factors(mask, store=store)
        record(case, before, snapshot(graph), mask=_np(mask), store=store)

    # ---- rm_keyframe: an ix that an inactive edge touches, and one that none does ---------------------------------------
    for case, seed, touch in (("rm_keyframe_inac_hit", 3, True), ("rm_keyframe_inac_miss", 4, False)):
        graph = make_graph(CovisibleGraph, CorrBlock, seed, n=12, n_inac=6, with_video=True)
        ix = 5
        graph.ii[3], graph.jj[7] = ix, ix   # the active list always has edges of the frame that goes
        hit = (graph.ii_inac == ix) | (graph.jj_inac == ix)
        if touch:
            graph.jj_inac[2] = ix
        else:
            graph.ii_inac[graph.ii_inac == ix] = ix + 2
            graph.jj_inac[graph.jj_inac == ix] = ix - 2
        hit = (graph.ii_inac == ix) | (graph.jj_inac == ix)
        assert bool(hit.any()) == touch
        before = snapshot(graph, with_video=True)
        graph.rm_keyframe(ix)
        record(case, before, snapshot(graph, with_video=True), ix=ix)

    # ---- __rollup: the edge statements ----------------------------------------------------------------------------------
    graph = make_graph(CovisibleGraph, CorrBlock, 5, n=10, n_inac=8, with_video=True)
    roll = 3
    graph.ii, graph.jj = graph.ii + roll, graph.jj + roll       # active edges live in the part of the window that stays
    graph.ii_bad, graph.jj_bad = graph.ii_bad + roll, graph.jj_bad + roll
    v = graph.video
    for k in ("dirty", "red"):
        setattr(v, k, torch.zeros(FRAMES + 1, dtype=torch.bool))
    v.disps_up = torch.zeros(FRAMES + 1, 8 * H, 8 * W)
    v.counter = types.SimpleNamespace(value=FRAMES)
    v.last_t0, v.last_t1, v.cur_ii, v.cur_jj, v.imu_enabled = 4, 8, torch.zeros(0).long(), torch.zeros(0).long(), False
    v.state = types.SimpleNamespace(**{k: list(range(FRAMES)) for k in (
        "timestamps", "wTbs", "vs", "bs", "preintegrations", "preintegrations_meas", "gnss_valid", "gnss_position",
        "odo_valid", "odo_vel")})
    front = object.__new__(Frontend)
    front.video, front.graph, front.t1, front.count = v, graph, FRAMES, FRAMES
    before = snapshot(graph)
    getattr(front, "_DBAFusionFrontend__rollup")(roll)
    after = snapshot(graph)
    assert 0 < after["ii_inac"].shape[0] < before["ii_inac"].shape[0]
    record("rollup", before, after, roll=roll)

    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "factor_edits.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %d arrays, %d bytes" % (path, len(cases), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
