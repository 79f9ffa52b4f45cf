"""Stage 0 of a keyed BA call as a workgroup of the call's first linearisation (csrc/ba_kernels.hip: ba_linearize_kernel's TF
variant; csrc/ba_host.hip: ba_run_loop) against the separate launch (DBA_BA_STAGE0=launch) and the CPU oracle.

Every case goes through droid_backends.ba / ba_clamped with two iterations and deterministic accumulation.  The cases run once in
this process (the default path) and once in a fresh child process with DBA_BA_STAGE0=launch; poses, inverse depths and dx must be
the same bits, and the index tables each path leaves in the workspace the same integers.  Against the float64 oracle the
tolerances are those tests/test_gpu_ba.py uses for maps of these sizes: test_ba_random_graphs_match_oracle's for the 8 x 8 maps
(its maps are 8 x 12), _compare_with_oracle's for the 16 x 24 ones (test_ba_duplicate_edges_and_edgeless_window_frame's size)."""
import functools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":      # the child process: the paths tests/conftest.py sets
    for p in (os.path.join(HERE, "..", "dba-fusion_amd"), os.path.join(HERE, ".."), HERE):
        sys.path.insert(0, os.path.abspath(p))

import torch  # noqa: E402

from dbaf_amd import synthetic as syn  # noqa: E402
from util import to_dev, check_state  # noqa: E402

try:
    import pytest
    pytestmark = pytest.mark.gpu
except ImportError:          # (the child needs none of it)
    pytest = None

FOLD_MAX_N, FOLD_MAX_B = 256, 512     # csrc/ba_kernels.h


def _tile(ii, jj, n):
    """the first n edges of the list repeated (duplicate edges are legal: the reference sums them)"""
    reps = (n + len(ii) - 1) // len(ii)
    return np.tile(ii, reps)[:n].copy(), np.tile(jj, reps)[:n].copy()


def _banded_n(n, num_kf=7, radius=3, h=8, w=8, seed=0, **kw):
    ii, jj = _tile(*syn.graph_banded(num_kf, radius), n)
    return syn.make_window(ii, jj, num_kf, h, w, seed=seed, **kw)


def _edge_cases(h, w, seed):
    """one window with: frame 3 of [t0, t1) without an out-edge, sources 0 and 1 below t0 = 2 (a slot, no pose row), targets 0 and
    1 outside the window, (2, 4) and (4, 2) twice, ii unsorted"""
    ii = np.array([4, 0, 2, 5, 1, 2, 4, 0, 5, 2, 4, 1, 2], np.int64)
    jj = np.array([2, 2, 4, 4, 4, 0, 5, 1, 2, 4, 2, 3, 1], np.int64)
    W = syn.make_window(ii, jj, 6, h, w, seed=seed, t0=2)
    assert 3 in W.kx and 3 not in ii and 0 in W.kx and W.t0 == 2
    return W


def _other_graph(W, seed):
    """another graph with the shapes of W: some edges re-targeted, and its own measurements"""
    ii, jj = W.ii.copy(), W.jj.copy()
    for n in range(0, len(jj), 3):
        jj[n] = (jj[n] + 1) % W.num_kf
        if jj[n] == ii[n]:
            jj[n] = (jj[n] + 1) % W.num_kf
    return syn.make_window(ii, jj, W.num_kf, W.h, W.w, seed=seed, t0=W.t0, buffer=W.B)


@functools.lru_cache(maxsize=None)
# name -> (the windows called one after the other, each with new tensors for everything; motion_only; ba_clamped?; eta rows)
def _cases():
    c = {}
    a8, a16 = syn.make_window(*syn.graph_banded(5, 2), 5, 8, 8, seed=21), syn.make_window(*syn.graph_banded(6, 2), 6, 16, 24, seed=22)
    c["same_graph_new_objects_8x8"] = dict(seq=[a8, a8, a8])
    c["same_graph_new_objects_16x24_clamped"] = dict(seq=[a16, a16, a16], clamped=True)
    b8, b16 = _other_graph(a8, 23), _other_graph(a16, 24)
    c["alternating_graphs_8x8"] = dict(seq=[a8, b8, a8, b8])
    c["alternating_graphs_16x24"] = dict(seq=[a16, b16, a16, b16])
    for n in (1, 63, 64, 65):       # different N on one buffer / map / window: a wave's worth of edges and its neighbours
        c["n%d_8x8" % n] = dict(seq=[_banded_n(n, seed=30 + n)])
    c["n65_16x24"] = dict(seq=[_banded_n(65, h=16, w=24, seed=40)])
    c["edge_cases_8x8"] = dict(seq=[_edge_cases(8, 8, 41)])
    c["edge_cases_16x24"] = dict(seq=[_edge_cases(16, 24, 42)])
    c["edge_cases_motion_only_16x24"] = dict(seq=[_edge_cases(16, 24, 43)], motion_only=True)
    c["motion_only_8x8_clamped"] = dict(seq=[a8, b8], motion_only=True, clamped=True)
    c["eta_one_row_16x24"] = dict(seq=[a16, a16], eta_rows=1)
    c["eta_one_row_edge_cases_8x8"] = dict(seq=[_edge_cases(8, 8, 44)], eta_rows=1)
    # just above the admission bounds: the separate launch on both sides
    c["above_bound_n%d_8x8" % (FOLD_MAX_N + 1)] = dict(seq=[_banded_n(FOLD_MAX_N + 1, seed=45)])
    c["above_bound_b%d_8x8" % (FOLD_MAX_B + 1)] = dict(seq=[syn.make_window(*syn.graph_banded(5, 2), 5, 8, 8, seed=46,
                                                                            buffer=FOLD_MAX_B + 1)])
    c["at_bound_n%d_b%d_8x8" % (FOLD_MAX_N, FOLD_MAX_B)] = dict(seq=[_banded_n(FOLD_MAX_N, seed=47, buffer=FOLD_MAX_B)])
    return c


def _align(x):
    return (x + 255) // 256 * 256


def _tables(W):
    """the index tables in the workspace droid_backends.ba keeps for W's shape, as csrc/ba_host.hip (ba_plan) lays them out; only
    what stage 0 writes of each"""
    import ctypes
    from dbaf_amd import _lib
    from droid_backends import _BA_WS
    dims = (W.N, W.B, W.h, W.w, W.t0, W.t1)
    key = [k for k in _BA_WS.ws if k[-1] == dims and k[0] != "bacore"][0]
    ws = _BA_WS.ws[key][0]
    lay = _lib.BaLayout()
    _lib.load().dba_ba_get_layout(*dims, ctypes.byref(lay))
    N, B, P, Mmax = W.N, W.B, W.t1 - W.t0, lay.Mmax
    assert Mmax == min(B, P + N)
    off, sizes = lay.meta, {}
    for name, ints in (("meta", 32), ("gkey", 8 + 2 * N), ("kx", max(Mmax, 1)), ("frame_slot", B), ("eoff", Mmax + 1),
                       ("elist", max(N, 1)), ("elist_rank", max(N, 1)), ("fpose", max(P, 1)), ("einfo", 2 * max(N, 1)),
                       ("rowinfo", 8 * max(P + N, 1)), ("fhead", 4 * max(Mmax, 1)), ("frow", 2 * max(P + N, 1))):
        sizes[name] = (off, ints)
        off = _align(off + 4 * ints)
    assert sizes["kx"][0] == lay.kx and off == lay.E, "the test's copy of the workspace layout is out of date"
    get = lambda name: ws[sizes[name][0]:sizes[name][0] + 4 * sizes[name][1]].view(torch.int32).cpu().numpy()  # noqa: E731
    M = int(get("meta")[0])
    assert M == W.M
    return dict(kx=get("kx")[:M], eoff=get("eoff")[:M + 1], elist=get("elist")[:N], einfo=get("einfo")[:2 * N],
                rowinfo=get("rowinfo")[:8 * (P + N)].reshape(-1, 8)[:, :5].copy(), fpose=get("fpose")[:P], gkey=get("gkey"),
                frame_slot=get("frame_slot"))


def _call(W, motion_only=False, clamped=False, eta_rows=None):
    import droid_backends
    d = to_dev(W)
    eta = d["eta"] if eta_rows is None else d["eta"][:eta_rows].contiguous()
    fn = droid_backends.ba_clamped if clamped else droid_backends.ba
    dx, dz = fn(d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["target"], d["weight"], eta, d["ii"], d["jj"],
                W.t0, W.t1, 2, W.lm, W.ep, motion_only)
    torch.cuda.synchronize()
    droid_backends.check_async_errors()
    return d["poses"].cpu().numpy(), d["disps"].cpu().numpy(), dx.cpu().numpy()


def run_cases():
    """every case's calls in order: {case/call index/poses | disps | dx, case/tables/<name>}"""
    from dbaf_amd import _lib
    lib = _lib.load()
    assert lib.dba_ba_set_deterministic(1) == 0
    out = {}
    try:
        for name, c in _cases().items():
            kw = dict(motion_only=c.get("motion_only", False), clamped=c.get("clamped", False), eta_rows=c.get("eta_rows"))
            for k, W in enumerate(c["seq"]):
                p, z, dx = _call(W, **kw)
                out["%s/%d/poses" % (name, k)], out["%s/%d/disps" % (name, k)], out["%s/%d/dx" % (name, k)] = p, z, dx
                if k == 0 or k == len(c["seq"]) - 1:
                    for t, v in _tables(W).items():
                        out["%s/%d/tables/%s" % (name, k, t)] = v
    finally:
        lib.dba_ba_set_deterministic(0)
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **run_cases())
    sys.exit(0)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """(the default path's results, the separate launch's from a fresh process)"""
    assert os.environ.get("DBA_BA_STAGE0") is None, "the test compares the default with DBA_BA_STAGE0=launch itself"
    path = str(tmp_path_factory.mktemp("stage0") / "launch.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, DBA_BA_STAGE0="launch"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(path) as f:
        launch = {k: f[k] for k in f.files}
    return run_cases(), launch


CASES = list(_cases())


@pytest.mark.parametrize("name", CASES)
def test_fold_and_separate_launch_give_the_same_bits_and_tables(both, name):
    fold, launch = both
    keys = [k for k in fold if k.startswith(name + "/")]
    assert keys and sorted(keys) == sorted(k for k in launch if k.startswith(name + "/"))
    for k in keys:
        assert fold[k].dtype == launch[k].dtype and fold[k].shape == launch[k].shape, k
        assert np.array_equal(fold[k].view(np.int32), launch[k].view(np.int32)), k


@pytest.mark.parametrize("name", CASES)
def test_fold_matches_the_oracle(both, name):
    from oracle import oracle as orc
    fold, c = both[0], _cases()[name]
    seen = {}
    for k, W in enumerate(c["seq"]):
        p, z, dx = (fold["%s/%d/%s" % (name, k, what)] for what in ("poses", "disps", "dx"))
        if id(W) in seen:        # the same window again, in new tensor objects: the same result, from the kept tables or rebuilt ones
            q = seen[id(W)]
            assert all(np.array_equal(fold["%s/%d/%s" % (name, k, what)], fold["%s/%d/%s" % (name, q, what)])
                       for what in ("poses", "disps", "dx")), (name, k)
            continue
        seen[id(W)] = k
        eta = W.eta if c.get("eta_rows") is None else W.eta[:c["eta_rows"]]
        mo = c.get("motion_only", False)
        args = (W.poses, W.disps, W.intrinsics, W.disps_sens, W.target, W.weight, eta, W.ii, W.jj, W.t0, W.t1, 2, W.lm, W.ep,
                mo, 0.05)
        r32, r64 = orc.ba(*args, np.float32), orc.ba(*args, np.float64)
        clamp = (lambda a: np.maximum(a, 0.001)) if c.get("clamped") else (lambda a: a)     # noqa: E731
        if mo:
            assert np.array_equal(z, clamp(W.disps))
        if np.abs(r64["dx"]).max() == 0.0:   # the damped system was not positive definite: zero update on both sides
            assert np.abs(dx).max() == 0.0
            continue
        if W.h * W.w == 64:
            print(name, k, check_state(p, clamp(z), r64["poses"], clamp(r64["disps"]), W.disps, ref32_disps=clamp(r32["disps"]),
                                       ref32_poses=r32["poses"], d_rtol=2e-3, frac=0.95, ref32_factor=6.0))
        else:
            print(name, k, check_state(p, clamp(z), r64["poses"], clamp(r64["disps"]), W.disps, ref32_disps=clamp(r32["disps"])))


def test_fold_rejects_a_mismatching_eta_and_recovers():
    """1 < eta rows != |kx|: the call changes nothing and the next call on the workspace raises, as with the separate launch
    (test_gpu_ba.py: test_ba_rejects_an_eta_with_the_wrong_number_of_rows); the verdict does not outlive the call: a correct call
    on the same workspace then gives what it gives on a fresh one, whether the graph's key matches (the tables are kept) or not"""
    import droid_backends
    from dbaf_amd import _lib
    from droid_backends import _BA_WS
    lib = _lib.load()
    assert lib.dba_ba_set_deterministic(1) == 0
    try:
        _eta_cases(droid_backends, _BA_WS)
    finally:
        lib.dba_ba_set_deterministic(0)


def _eta_cases(droid_backends, _BA_WS):
    W = _edge_cases(8, 8, 51)
    W2 = _other_graph(W, 52)
    assert W.M > 3 and W2.M == W.M
    saved = _BA_WS.enabled
    _BA_WS.enabled = False      # a fresh workspace and a separate stage 0 per call
    try:
        ref, ref2 = _call(W), _call(W2)
    finally:
        _BA_WS.enabled = saved
    torch.cuda.synchronize()
    droid_backends.check_async_errors()
    first = _call(W)
    assert all(np.array_equal(a, b) for a, b in zip(first, ref))
    for Wbad, Wgood, want in ((W, W, ref), (W2, W, ref), (W, W2, ref2)):
        d = to_dev(Wbad)
        eta = torch.full((Wbad.M - 1, Wbad.h, Wbad.w), 3e-7, device="cuda")
        p0, z0 = d["poses"].clone(), d["disps"].clone()
        dx, dz = droid_backends.ba(d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["target"], d["weight"], eta,
                                   d["ii"], d["jj"], Wbad.t0, Wbad.t1, 2, Wbad.lm, Wbad.ep, False)
        torch.cuda.synchronize()
        assert torch.equal(d["poses"], p0) and torch.equal(d["disps"], z0) and not dx.any() and not dz.any()
        with pytest.raises(RuntimeError, match="eta with %d rows.*= %d rows" % (Wbad.M - 1, Wbad.M)):
            _call(Wgood)
        got = _call(Wgood)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
