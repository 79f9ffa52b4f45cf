"""CPU: the statement and the cases of tests/conv_agg_mean_cases.py -- the float64 frame mean against torch's, the exactness
claims of the exact cases, the member table's reference, the new entry points in the header and in the built library, the
switch's default, and the host-side refusals of dba_conv3x3_mean_f16 and dba_frame_members.  The refusals are called only with
arguments the functions reject BEFORE any runtime call: their pointers are made-up addresses that nothing dereferences."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import conv_agg_mean_cases as MC

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SYMBOLS = ("dba_conv3x3_mean_f16", "dba_frame_members", "dba_frame_members_max_slots")
DBA_ERR_ARG = -1


def test_symbols_in_header_and_library():
    header = open(os.path.join(ROOT, "include", "dba_hip.h")).read()
    from dbaf_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in _lib.SYMBOLS and getattr(lib, s) is not None
    assert "out_rows" in header
    assert lib.dba_frame_members_max_slots() == lib.dba_frame_plan_max_rows()


def test_the_switch_is_off_by_default_and_forwards():
    from dbaf_amd import conv
    from dbaf_amd import update_op as U
    assert U.GraphAgg.fuse_mean is False
    m = U.UpdateModule()
    assert m.fuse_mean is False and m.agg.fuse_mean is False
    m.fuse_mean = 1
    assert m.agg.fuse_mean is True and m.fuse_mean is True
    assert (m.fuse_agg, m.fuse_conv, m.fuse_upmask, m.fuse_flow_stem) == (False, False, False, False)
    assert callable(conv.conv3x3_frame_mean) and callable(conv.frame_members)


def test_routing_rule_is_the_measured_verdict():
    """frames x tiles of the five measured states on 256 compute units (profiles/conv_agg_mean_bench.json) and the windows
    of the module tests"""
    from dbaf_amd import conv
    measured = [(12, 64, 64, True), (12, 55, 55, True), (25, 64, 64, False), (32, 28, 107, True), (10, 48, 64, False)]
    for frames, h, w, pays in measured:
        assert conv.frame_mean_pays(frames, h, w, 256) is pays, (frames, h, w)
    for n, F, ht, wd, _ in MC.WINDOWS:
        assert conv.frame_mean_pays(F, ht, wd, 256) is True
    assert conv.frame_mean_pays(16, 64, 64, 256) is True       # exactly one round


@pytest.mark.parametrize("edges", MC.EDGE_LISTS, ids=lambda e: e[0])
def test_statement_against_torch_float64(edges):
    _, inverse, F = edges
    x, w, b = MC.random_inputs((5, 7), (32, 64))
    n = len(inverse)
    mean, s, count, c = MC.frame_mean_ref(x[:n], w, b, inverse, F)
    conv = torch.nn.functional.conv2d(torch.from_numpy(x[:n].astype(np.float64)), torch.from_numpy(w.astype(np.float64)),
                                      torch.from_numpy(b.astype(np.float64)), padding=1)
    r = torch.relu(conv.to(torch.float16).to(torch.float64))       # the half the first launch stores
    keep = [e for e in range(n) if 0 <= inverse[e] < F]
    ref = torch.zeros((F,) + tuple(r.shape[1:]), dtype=torch.float64)
    ref.index_add_(0, torch.tensor([inverse[e] for e in keep]), r[keep])
    cnt = np.bincount([inverse[e] for e in keep], minlength=F)
    assert np.array_equal(count, cnt)
    ref = ref.numpy() / np.maximum(cnt, 1).reshape(-1, 1, 1, 1)
    # conv_c's float64 sum and torch's differ in order: a half rounding may flip on a tie-close entry, nowhere else
    close = np.abs(mean - ref) <= 2.0 ** -10 * np.maximum(np.abs(ref), 2.0 ** -14)
    assert close.all() and (mean == ref).mean() > 0.99
    assert (mean[count == 0] == 0).all()


def test_interleaved_inverse_is_torch_uniques():
    _, inv = torch.unique(torch.tensor(MC.INTERLEAVED_II), return_inverse=True)
    assert tuple(inv.tolist()) == MC.EDGE_LISTS[2][1] and MC.EDGE_LISTS[2][2] == 4
    for n, F, ht, wd, ii in MC.WINDOWS:
        assert len(ii) == n and len(set(ii)) == F


@pytest.mark.parametrize("edges", MC.EXACT_LISTS, ids=lambda e: e[0])
def test_exact_cases_are_exact(edges):
    r = MC.exact_reference(edges[0])
    c, s, count = r["c"], r["sum"], r["count"]
    # integers, exact in half per edge and in float32 per slot
    assert np.array_equal(np.round(c), c) and np.abs(c).max() <= 2048
    assert np.array_equal(np.round(s), s) and s.max() < 2 ** 24
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    assert (c < 0).mean() > 0.2 and (c > 0).mean() > 0.2
    # the ReLU sits before the mean: taking it behind the mean gives another tensor
    behind = np.zeros_like(s)
    for e, slot in enumerate(r["inverse"]):
        behind[slot] += c[e]
    behind = np.maximum(behind / np.maximum(count, 1).reshape(-1, 1, 1, 1), 0)
    many = count > 1
    assert many.any() and (behind[many] != r["mean"][many]).mean() > 0.2
    assert sorted(set(count.tolist())) == ([1, 2, 3] if edges[0] == "interleaved" else [4])
    # counts 1, 2, 4: the float32 division is exact, so the stored half is the statement rounded once
    pow2 = np.isin(count, (1, 2, 4))
    q = MC.half_of_division(s, count)
    assert np.array_equal(q[pow2].view(np.uint16), r["mean"][pow2].astype(np.float16).view(np.uint16))
    if (count == 3).any():
        third = q[count == 3].astype(np.float64)
        assert np.abs(third - r["mean"][count == 3]).max() <= 0.5 * 2.0 ** -10 * np.abs(r["mean"][count == 3]).max() + 2.0 ** -24


@pytest.mark.parametrize("case", MC.TABLE_CASES, ids=lambda c: "n%d_F%d" % c[:2])
def test_members_reference(case):
    n, F, seed = case
    inv = MC.table_case(n, F, seed)
    seg, mem = MC.members_ref(inv, F)
    assert seg.shape == (F + 1,) and mem.shape == (n,) and seg[0] == 0 and (np.diff(seg) >= 0).all()
    inside = (inv >= 0) & (inv < F)
    assert seg[F] == inside.sum() and (mem[seg[F]:] == -1).all()
    for s in range(F):
        m = mem[seg[s]:seg[s + 1]]
        assert (inv[m] == s).all() and (np.diff(m) > 0).all()
    assert sorted(mem[:seg[F]].tolist()) == np.nonzero(inside)[0].tolist()


# ---- host-side refusals: every call below is rejected before the function makes any runtime call ---------------------------

A = 1 << 20          # made-up addresses, 16-byte aligned; nothing reads them
GOOD = dict(src=A, c_in=32, weight=2 * A, bias=3 * A, c_out=64, n=3, h=5, w=7, seg_start=4 * A, members=5 * A, F=2, out=6 * A,
            out_rows=2)
ORDER = ("src", "c_in", "weight", "bias", "c_out", "n", "h", "w", "seg_start", "members", "F", "out", "out_rows")
POINTERS = ("src", "weight", "bias", "seg_start", "members", "out")
REFUSED = [("F=0", dict(F=0)), ("F=-1", dict(F=-1)), ("F>out_rows", dict(F=3)), ("F>>out_rows", dict(F=4096, out_rows=1)),
           ("out_rows=0", dict(out_rows=0)), ("n=0", dict(n=0)), ("n=-5", dict(n=-5)), ("null src", dict(src=None)),
           ("null weight", dict(weight=None)), ("null seg_start", dict(seg_start=None)), ("null members", dict(members=None)),
           ("null out", dict(out=None)), ("c_in=16", dict(c_in=16)), ("c_in=0", dict(c_in=0)), ("c_out=32", dict(c_out=32)),
           ("c_out=96", dict(c_out=96)), ("weight+8", dict(weight=2 * A + 8)), ("h=0", dict(h=0)), ("w=-1", dict(w=-1)),
           ("out in src", dict(out=A + 64))]


@pytest.mark.parametrize("change", REFUSED, ids=lambda c: c[0])
def test_entry_refuses_on_the_host(change):
    from dbaf_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **change[1])
    assert a != GOOD
    args = [ctypes.c_void_p(a[k]) if k in POINTERS else a[k] for k in ORDER]
    assert lib.dba_conv3x3_mean_f16(*args, None) == DBA_ERR_ARG


@pytest.mark.parametrize("change", [("n=0", dict(n=0)), ("F=0", dict(F=0)), ("F beyond the plan", dict(F=4097)),
                                    ("null inverse", dict(inverse=None)), ("null seg_start", dict(seg_start=None)),
                                    ("null members", dict(members=None))], ids=lambda c: c[0])
def test_members_entry_refuses_on_the_host(change):
    from dbaf_amd import _lib
    lib = _lib.load()
    a = dict(dict(inverse=A, n=3, F=2, seg_start=2 * A, members=3 * A), **change[1])
    ptr = lambda v: ctypes.c_void_p(v)   # noqa: E731
    assert lib.dba_frame_members(ptr(a["inverse"]), a["n"], a["F"], ptr(a["seg_start"]), ptr(a["members"]), None) == DBA_ERR_ARG
