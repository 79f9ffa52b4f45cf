"""The (row, partner) Schur form on the pair list (ba_schur_pairs_kernel: one workgroup per listed pair, a chunk's pixels
loaded in one phase, one transposing reduction per wave) against the (row, partner slot) grid (ba_schur_kernel, kept as
dba_ba_schur_sparse_select(1) / DBA_SCHUR_SPARSE=legacy).

Both form every float sum the same way, so with deterministic accumulation (integer atomics: order-independent) H, b, dx and
the retracted state of ba(iterations=2) must be identical bit for bit; without it the new form is held to the float64 arbiter
at the tolerances of util.check_state.  The pair list itself is compared with a numpy enumeration, and between stage 0 folded
into the first linearisation and stage 0 as a launch of its own."""
import ctypes

import numpy as np
import pytest
import torch

from dbaf_amd import synthetic as syn
from util import to_dev, check_state

pytestmark = pytest.mark.gpu

SCHUR_CH, BATCH_PIXELS = 2, 2048     # csrc/ba_kernels.h, csrc/ba_kernels.hip (256 * SCHUR_BATCH)

WINDOWS = {
    # chunk 32 < 256: most lanes of the one-phase load are predicated off
    "3kf_2edges_8x8": lambda: syn.make_window(np.array([1, 2], np.int64), np.array([2, 1], np.int64), 3, 8, 8, seed=71,
                                              intr=(4.0, 4.0, 4.1, 3.9)),
    # HW = 240, no multiple of 256
    "5kf_radius2_12x20": lambda: syn.make_window(*syn.graph_banded(5, 2), 5, 12, 20, seed=72, intr=(8.0, 8.5, 10.2, 6.1)),
    # chunk 1513: above 1024 and odd
    "9kf_36edges_55x55": lambda: syn.make_window(*syn.graph_banded(9, 2, extra=[(0, 3), (1, 4), (2, 5)]), 9, 55, 55, seed=14,
                                                 intr=(20.5, 20.5, 27.4, 27.6)),
    # two fixed frames in front: edges whose target is outside [t0, t1), and source frames that are no window pose
    "6kf_targets_outside_12x20": lambda: syn.make_window(*syn.graph_banded(6, 2), 6, 12, 20, seed=73, t0=2,
                                                         intr=(8.0, 8.5, 10.2, 6.1)),
    # the first pose fixed (t0 = 1), a buffer longer than the window
    "4kf_fixed_first_pose_16x16": lambda: syn.make_window(*syn.graph_banded(4, 3), 4, 16, 16, seed=74, buffer=7,
                                                          intr=(8.0, 8.0, 8.1, 7.9)),
    # 8 keyframes at 48 x 64: chunk 1536, the one-phase form with its last two trips predicated off
    "8kf_48x64": lambda: syn.make_window(*syn.graph_banded(8, 2), 8, 48, 64, seed=75, intr=(30.0, 30.0, 31.5, 23.7)),
    # chunk 2113 > 2048: the pixel loop
    "8kf_65x65_loop": lambda: syn.make_window(*syn.graph_banded(8, 2), 8, 65, 65, seed=76, intr=(30.0, 30.0, 32.2, 32.4)),
}


def test_the_cases_cover_both_pixel_paths():
    chunk = lambda h, w: (h * w + SCHUR_CH - 1) // SCHUR_CH  # noqa: E731
    assert chunk(8, 8) < 256 and 1024 < chunk(55, 55) <= BATCH_PIXELS and chunk(55, 55) % 2 and chunk(65, 65) > BATCH_PIXELS


def _lib():
    from dbaf_amd import _lib as L
    return L, L.load()


def _workspace(W):
    from droid_backends import _BA_WS
    dims = (W.N, W.B, W.h, W.w, W.t0, W.t1)
    key = [k for k in _BA_WS.ws if k[-1] == dims and k[0] != "bacore"][0]
    return dims, _BA_WS.ws[key][0]


def _pairs_of(ws, dims):
    L, lib = _lib()
    off, cap = ctypes.c_size_t(0), ctypes.c_int(0)
    L.check(lib.dba_ba_pairs_table(*dims, ctypes.byref(off), ctypes.byref(cap)), "dba_ba_pairs_table")
    t = ws[off.value:off.value + 16 * (1 + cap.value)].view(torch.int32).cpu().numpy().reshape(-1, 4)
    n = int(t[0, 0])
    assert 0 <= n <= cap.value, (n, cap.value)
    return t[0].copy(), t[1:1 + n].copy()


def _expected_pairs(W):
    """rows of E: pose p (frame t0 + p) | P + edge n.  A source frame couples its own pose row (if it is a window pose) and its
    out-edges with a target inside the window, in ascending edge id; every unordered pair of those, self pairs included"""
    P = W.t1 - W.t0
    slot = {int(f): m for m, f in enumerate(W.kx)}
    out = set()
    for f, m in slot.items():
        rows = [(f - W.t0, f - W.t0)] if 0 <= f - W.t0 < P else []
        rows += [(P + n, int(W.jj[n]) - W.t0) for n in range(W.N) if int(W.ii[n]) == f and 0 <= int(W.jj[n]) - W.t0 < P]
        for a in range(len(rows)):
            for b in range(a, len(rows)):
                out.add((rows[a][0], rows[b][0], rows[a][1] | (rows[b][1] << 16), m))
    return out


def _ba(W, legacy, deterministic):
    import droid_backends
    L, lib = _lib()
    assert lib.dba_ba_schur_sparse_select(1 if legacy else 0) == 0
    assert lib.dba_ba_set_deterministic(1 if deterministic else 0) == 0
    try:
        d = to_dev(W)
        dx, dz = droid_backends.ba(d["poses"], d["disps"], d["intrinsics"], d["disps_sens"], d["target"], d["weight"], d["eta"],
                                   d["ii"], d["jj"], W.t0, W.t1, 2, W.lm, W.ep, False)
        torch.cuda.synchronize()
        droid_backends.check_async_errors()
        dims, ws = _workspace(W)
        lay = L.BaLayout()
        L.check(lib.dba_ba_get_layout(*dims, ctypes.byref(lay)), "dba_ba_get_layout")
        n6 = 6 * lay.P
        H = ws[lay.H:lay.H + 8 * n6 * n6].view(torch.float64).cpu().numpy().reshape(n6, n6)
        b = ws[lay.b:lay.b + 8 * n6].view(torch.float64).cpu().numpy()
        return dict(poses=d["poses"].cpu().numpy(), disps=d["disps"].cpu().numpy(), dx=dx.cpu().numpy(), dz=dz.cpu().numpy(),
                    H=np.tril(H), b=b.copy())
    finally:
        lib.dba_ba_schur_sparse_select(0)
        lib.dba_ba_set_deterministic(0)


_ORACLE = {}


def _oracle(name, W):
    if name not in _ORACLE:
        from oracle import oracle as orc
        args = (W.poses, W.disps, W.intrinsics, W.disps_sens, W.target, W.weight, W.eta, W.ii, W.jj, W.t0, W.t1, 2, W.lm, W.ep,
                False, 0.05)
        _ORACLE[name] = (orc.ba(*args, np.float64), orc.ba(*args, np.float32))
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(WINDOWS))
def test_pair_list_form_gives_the_bits_of_the_row_partner_grid(name):
    W = WINDOWS[name]()
    L, lib = _lib()
    assert lib.dba_ba_schur_auto_form(W.N, W.t1 - W.t0) == 1, "the window must take the (row, partner) form"
    new = _ba(W, legacy=False, deterministic=True)
    old = _ba(W, legacy=True, deterministic=True)
    assert np.isfinite(new["H"]).all() and np.abs(new["H"]).max() > 0 and np.abs(new["dx"]).max() > 0
    for k in ("H", "b", "dx", "dz", "poses", "disps"):
        a, b = new[k], old[k]
        same = np.array_equal(a.view(np.uint8), b.view(np.uint8))
        print(name, k, "identical" if same else "max |diff| %.3e of %.3e" % (np.abs(a - b).max(), np.abs(b).max()))
        assert same, (name, k)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_pair_list_form_matches_the_float64_arbiter(name):
    W = WINDOWS[name]()
    r64, r32 = _oracle(name, W)
    new = _ba(W, legacy=False, deterministic=False)
    clamp = lambda a: np.maximum(a, 0.001)  # noqa: E731
    msg = check_state(new["poses"], clamp(new["disps"]), r64["poses"], clamp(r64["disps"]), W.disps,
                      ref32_disps=clamp(r32["disps"]))
    print(name, "vs fp64 arbiter:", msg)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_pair_list_is_the_graphs_and_the_same_from_both_stage0_paths(name):
    """droid_backends.ba prepares by key, i.e. with stage 0 folded into its first linearisation (the default); dba_ba_prepare
    on a fresh workspace is the separate launch (ba_prepare_kernel), what DBA_BA_STAGE0=launch runs"""
    W = WINDOWS[name]()
    L, lib = _lib()
    _ba(W, legacy=False, deterministic=False)
    dims, ws = _workspace(W)
    head, folded = _pairs_of(ws, dims)
    assert head[1:].tolist() == [0, 0, 0]
    want = _expected_pairs(W)
    got = set(map(tuple, folded.tolist()))
    assert len(got) == len(folded), "a pair is listed twice"
    assert got == want, (sorted(got - want)[:5], sorted(want - got)[:5])
    nbytes = lib.dba_ba_workspace_bytes(*dims)
    ws2 = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ii, jj = (torch.from_numpy(a).cuda() for a in (W.ii, W.jj))
    L.check(lib.dba_ba_workspace_init(*dims, ws2.data_ptr(), nbytes, None), "dba_ba_workspace_init")
    L.check(lib.dba_ba_prepare(ii.data_ptr(), jj.data_ptr(), *dims, ws2.data_ptr(), nbytes, None), "dba_ba_prepare")
    torch.cuda.synchronize()
    head2, launched = _pairs_of(ws2, dims)
    assert np.array_equal(head, head2) and np.array_equal(folded, launched)
