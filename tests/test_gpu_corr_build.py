"""The correlation build on the device against its float64 statement (tests/corr_build_cases.py): every line of the case table
through the fused build, through the unfused pipeline and into a slot-addressed store with guard bytes, on all levels, under the
rules of its input classes; the route each line reaches; source and target maps of different sizes; the forms behind the
DBA_BUILD_* switches in child sessions."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import corr_build_cases as S

pytestmark = pytest.mark.gpu

GUARD = 4096          # bytes of pattern before and after each level store
PATTERN = 0xA5        # ... and in the spare slot and the planes' padding: a half of bits 0xA5A5 wherever nothing may be written
FORCED_NOW = [k for k in S.FORCED if os.environ.get(k.split("=")[0]) == k.split("=")[1]]
WORST = {}            # route -> worst |err| / bound of the random class, for the last test of the file
CHILD_LIMIT = 420


def _lib():
    from dbaf_amd import _lib
    return _lib.load()


def _grid(h1, w1):
    hg, wg = ctypes.c_int(0), ctypes.c_int(0)
    tw = _lib().dba_corr_sheared_grid(int(h1), int(w1), ctypes.byref(hg), ctypes.byref(wg))
    return int(tw), hg.value, wg.value


def _bits(x):
    return np.ascontiguousarray(x, np.float16).view(np.uint16)


def _host(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _canon(b):
    """every NaN as one bit pattern (which NaN comes out of inf - inf is not part of the statement)"""
    b = np.array(b, np.uint16)
    b[(b & 0x7FFF) > 0x7C00] = 0x7E00
    return b


def _dev(f):
    return torch.from_numpy(np.array(f, copy=True))[None].cuda()


def _supported(c):
    return bool(_lib().dba_corr_volume_build_sheared_supported(c.C, c.h1, c.w1, c.h2, c.w2, c.levels))


def _check_route(c):
    route = _lib().dba_corr_volume_build_route(c.C, c.h1, c.w1, c.h2, c.w2, c.levels)
    if FORCED_NOW:
        for k in FORCED_NOW:
            assert S.FORCED[k](route), (k, S.ROUTE_NAMES[route])
    else:
        assert S.ROUTE_NAMES[route] == c.route
    return route


# ---- the three ways to build ------------------------------------------------------------------------------------------
def _fused(c, t1, t2):
    from dbaf_amd.corr import CorrBlock
    lv = CorrBlock.build_sheared_fused(t1, t2, c.levels)
    assert (lv is not None) == _supported(c)
    return None if lv is None else [_host(v) for v in lv]


def _unfused(c, t1, t2):
    from dbaf_amd.corr import CorrBlock
    return [_host(v) for v in CorrBlock.shear_pyramid(CorrBlock.build_pyramid(t1, t2, c.levels))]


def _into_store(c, t1, t2, grid):
    """the level stores are views into ONE allocation filled with the pattern: a guard before and after each level, one spare
    slot, the edges in slots that are not their numbers.  Equal maps go through a CorrBlock whose stores these views are (the call
    CorrBlock.cat makes for new edges), unequal ones through the C ABI, which is all that takes them.  Afterwards the guards and
    the spare slot still hold the pattern, and so does the padding of linear planes where the fused build wrote the store."""
    from dbaf_amd import _lib as L
    from dbaf_amd.corr import CorrBlock
    lib = L.load()
    n, cap, spare = c.n, c.n + 1, min(1, c.n)
    hw1p = S.plane_elems(c.h1, c.w1, grid)
    assert hw1p == lib.dba_corr_sheared_plane_elems(c.h1, c.w1)
    shapes = [(cap, c.h2 >> l, c.w2 >> l, hw1p) for l in range(c.levels)]
    sizes = [2 * int(np.prod(s)) for s in shapes]
    offs, total = [], GUARD
    for sz in sizes:
        offs.append(total)
        total += (sz + GUARD + 255) // 256 * 256
    alloc = torch.full((total,), PATTERN, dtype=torch.uint8, device="cuda")
    views = [alloc[o:o + sz].view(torch.float16).view(sh) for o, sz, sh in zip(offs, sizes, shapes)]
    slots = [s for s in range(cap) if s != spare][::-1]
    slots_t = torch.tensor(slots, dtype=torch.int32, device="cuda")
    equal = (c.h1, c.w1) == (c.h2, c.w2)
    if equal:
        cb = CorrBlock(t1, t2, num_levels=c.levels, capacity=cap)
        assert cb.layout == "sheared"
        g1, g2 = cb._take_pending()
        cb._stores, cb._slots, cb._slots_host, cb._identity = views, slots_t, list(slots), False
        cb._build_into(g1, g2, slots_t)
        got = [_host(v) for v in cb.corr_pyramid]
        plain = CorrBlock(t1, t2, num_levels=c.levels, capacity=cap).build()      # ... and the public way, slot k for edge k
        assert plain.capacity == cap
        for a, b in zip(got, plain.corr_pyramid):
            real = S.real_entries(c.h1, c.w1, grid)
            assert np.array_equal(a[..., real], _host(b)[..., real])
    else:
        f1, f2 = t1[0].contiguous(), t2[0].contiguous()
        sbytes = lib.dba_corr_volume_scratch_bytes(n, c.C, c.h1, c.w1, c.h2, c.w2)
        scratch = torch.empty(max(sbytes, 1), dtype=torch.uint8, device="cuda")
        ptrs = (ctypes.c_void_p * c.levels)(*[v.data_ptr() for v in views])
        L.check(lib.dba_corr_volume_build_sheared_slots(f1.data_ptr(), f2.data_ptr(), ptrs, slots_t.data_ptr(), n, c.C, c.h1, c.w1,
                                                        c.h2, c.w2, c.levels, scratch.data_ptr(), sbytes,
                                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "build_sheared_slots")
        got = [_host(v.index_select(0, slots_t.long())) for v in views]
    torch.cuda.synchronize()
    raw = alloc.cpu().numpy()
    edges = [0] + [x for o, sz in zip(offs, sizes) for x in (o, o + sz)] + [total]
    for a, b in zip(edges[0::2], edges[1::2]):
        assert (raw[a:b] == PATTERN).all(), "guard bytes [%d, %d) were written" % (a, b)
    pad = ~S.real_entries(c.h1, c.w1, grid)
    for l, (o, sz, sh) in enumerate(zip(offs, sizes, shapes)):
        store = raw[o:o + sz].view(np.uint16).reshape(sh)
        assert (store[spare] == PATTERN * 0x0101).all(), "the spare slot of level %d was written" % l
        if _supported(c) and pad.any():      # (the unfused path copies whole planes into the store, their padding included)
            assert (store[..., pad] == PATTERN * 0x0101).all(), "the plane padding of level %d was written" % l
    return got


# ---- the classes' rules -----------------------------------------------------------------------------------------------
def _first_bad(got, want, real):
    bad = np.argwhere((got != want) & real[None, None, None, :])
    return None if len(bad) == 0 else bad[0]


def _forced_bit_for_bit(c, cls, seed, f1, f2, ways, grid):
    pyr = S.pyramid(f1, f2, c.levels)
    real = S.real_entries(c.h1, c.w1, grid)
    for l in range(c.levels):
        want = S.sheared(_bits(pyr[l]), l, c.h1, c.w1, grid)
        for name, got in ways.items():
            assert got[l].shape == want.shape, (name, l, got[l].shape)
            bad = _first_bad(got[l], want, real)
            if bad is not None:
                share = float(((got[l] != want) & real).mean())
                if cls == "naming" and l == 0:
                    pytest.fail("%s: %s (%.3g of the entries differ)" % (name, S.naming_report(
                        got[l][tuple(bad)], want[tuple(bad)], bad, c.C, c.h1, c.w1, c.h2, c.w2, grid, seed), share))
                pytest.fail("%s, level %d: entry %s holds 0x%04x, the statement 0x%04x (%.3g of the entries differ)" % (
                    name, l, tuple(int(v) for v in bad), got[l][tuple(bad)], want[tuple(bad)], share))


def _pooled_from_own_level_below(c, ways, grid, float32=False):
    """every level above the first is the pooling of the device's OWN level below, bit for bit.  float32 (the range class): against
    the reference's float32 accumulation (corr_build_cases.pool_float32), NaNs as one pattern, and with inf and NaN exactly where
    the float64 statement has them"""
    real = S.real_entries(c.h1, c.w1, grid)
    for name, got in ways.items():
        for l in range(1, c.levels):
            below = S.unsheared(got[l - 1], l - 1, c.h1, c.w1, grid).view(np.float16)
            want = S.sheared(_bits(S.pool_float32(below) if float32 else S.pool(below)), l, c.h1, c.w1, grid)
            g = got[l]
            if float32:
                g, want = _canon(g), _canon(want)
                ieee = _canon(S.sheared(_bits(S.pool(below)), l, c.h1, c.w1, grid))
                special = ((g & 0x7C00) == 0x7C00) | ((ieee & 0x7C00) == 0x7C00)
                bad = _first_bad(g * special, ieee * special, real)
                assert bad is None, "%s, level %d: entry %s holds 0x%04x, the statement 0x%04x" % (
                    name, l, tuple(int(v) for v in bad), g[tuple(bad)], ieee[tuple(bad)])
            bad = _first_bad(g, want, real)
            assert bad is None, "%s, level %d: entry %s holds 0x%04x, the pooled level below 0x%04x" % (
                name, l, tuple(int(v) for v in bad), g[tuple(bad)], want[tuple(bad)])


def _random(c, f1, f2, ways, grid):
    ex = S.sheared(S.exact(f1, f2), 0, c.h1, c.w1, grid)
    bd = S.sheared(S.bound(f1, f2), 0, c.h1, c.w1, grid, fill=1.0)
    real = S.real_entries(c.h1, c.w1, grid)
    for name, got in ways.items():
        use = (np.abs(got[0].view(np.float16).astype(np.float64) - ex) / bd)[..., real]
        worst = float(use.max())
        print("random %s %s: worst |err| / bound = %.4f" % (S.case_id(c), name, worst))
        key = c.route if name != "unfused" else "unfused"
        if not FORCED_NOW:
            WORST[key] = max(WORST.get(key, 0.0), worst)
        assert worst < 1.0, (name, worst)
    _pooled_from_own_level_below(c, ways, grid)


def _range(c, seed, f1, f2, ways, grid):
    lo, hi = S.interval(f1, f2)
    lo = S.sheared(lo.astype(np.float64), 0, c.h1, c.w1, grid)
    hi = S.sheared(hi.astype(np.float64), 0, c.h1, c.w1, grid)
    want = S.sheared(_bits(S.volume(f1, f2)), 0, c.h1, c.w1, grid)
    real = S.real_entries(c.h1, c.w1, grid)
    rows = np.zeros(real.shape, bool)
    if S.RANGE_VARIANTS[seed] == "overflow":     # these rows' sums are exact in float32 in any order: no freedom, ties included
        yy, xx = np.mgrid[0:c.h1, 0:c.w1]
        rows[S.pixel_index(yy, xx, c.w1, grid)[((yy * c.w1 + xx) % 5) == 0]] = True
    for name, got in ways.items():
        g = got[0].view(np.float16).astype(np.float64)
        with np.errstate(invalid="ignore"):
            ok = ((g >= lo) & (g <= hi)) | (np.isnan(lo) & np.isnan(g))
        bad = np.argwhere(~ok & real)
        assert len(bad) == 0, "%s %s: entry %s holds %r outside [%r, %r] (%d entries)" % (
            name, S.RANGE_VARIANTS[seed], tuple(bad[0]), g[tuple(bad[0])], lo[tuple(bad[0])], hi[tuple(bad[0])], len(bad))
        bad = _first_bad(_canon(got[0]) * rows, _canon(want) * rows, real)
        assert bad is None, "%s: exact row entry %s holds 0x%04x, the statement 0x%04x" % (
            name, tuple(bad), got[0][tuple(bad)], want[tuple(bad)])
        if S.RANGE_VARIANTS[seed] == "overflow":
            assert np.isinf(g[..., rows]).any() and (np.abs(g[..., rows]) == 65504).any()
        else:
            tiny = np.abs(g[..., real])
            assert ((tiny > 0) & (tiny < 2.0 ** -14)).any(), "no subnormal result came out"
    _pooled_from_own_level_below(c, ways, grid, float32=True)


SEEDS = {"exact": (0,), "naming": (0, 1), "random": (0,), "range": (0, 1, 2)}
LINES = [(c, cls) for c in S.CASES + S.UNEQUAL for cls in c.classes if cls != "poison"]


@pytest.mark.parametrize("case,cls", LINES, ids=["%s-%s" % (S.case_id(c), cls) for c, cls in LINES])
def test_every_line_matches_the_statement(case, cls):
    """fused (where the shape is supported), unfused and into a guarded store with a spare slot: all four levels against the
    statement under the class's rule -- bit for bit (exact, naming), within the derived bound and pooled from the device's own
    level below (random), inside the rounded interval with the exact rows bit for bit (range)"""
    c = case
    _check_route(c)
    grid = _grid(c.h1, c.w1)
    for seed in SEEDS[cls]:
        f1, f2 = S.CLASSES[cls](c.n, c.C, c.h1, c.w1, c.h2, c.w2, seed)
        t1, t2 = _dev(f1), _dev(f2)
        ways = {"unfused": _unfused(c, t1, t2), "store": _into_store(c, t1, t2, grid)}
        fused = _fused(c, t1, t2)
        assert (fused is None) == (c.route == "unfused")
        if fused is not None:
            ways["fused"] = fused
        if cls in ("exact", "naming"):
            _forced_bit_for_bit(c, cls, seed, f1, f2, ways, grid)
        elif cls == "random":
            _random(c, f1, f2, ways, grid)
        else:
            _range(c, seed, f1, f2, ways, grid)


POISONED = [c for c in S.CASES + S.UNEQUAL if "poison" in c.classes]


@pytest.mark.parametrize("case", POISONED, ids=[S.case_id(c) for c in POISONED])
@pytest.mark.parametrize("side", ["source", "target"])
def test_a_poisoned_pixel_stays_in_its_row_or_column(case, side):
    """one NaN or one inf in one channel of one pixel, a different pixel in each of three edges: the pixel's row (source) or its
    column and the column's pooled ancestors (target) are non-finite on every level, everything else is the clean build's bits"""
    c = case._replace(n=3)
    _check_route(c)
    grid = _grid(c.h1, c.w1)
    f1, f2 = S.cls_poison(3, c.C, c.h1, c.w1, c.h2, c.w2, 0)
    pix = S.poison_pixels(c.h1, c.w1, grid) if side == "source" else S.poison_pixels(c.h2, c.w2)
    p1, p2 = f1.copy(), f2.copy()
    where = []
    for e in range(3):
        y, x = pix[e % len(pix)]
        ch = (37 * e + 5) % c.C
        (p1 if side == "source" else p2)[e, ch, y, x] = [np.nan, -np.inf, np.inf][e]
        where.append((y, x))

    def build(a, b):
        t1, t2 = _dev(a), _dev(b)
        ways = {"unfused": _unfused(c, t1, t2)}
        fused = _fused(c, t1, t2)
        if fused is not None:
            ways["fused"] = fused
        return {k: [S.unsheared(v[l], l, c.h1, c.w1, grid) for l in range(c.levels)] for k, v in ways.items()}
    clean, dirty = build(f1, f2), build(p1, p2)
    for name in clean:
        for l in range(c.levels):
            d, k = dirty[name][l], clean[name][l]                       # [3, h1, w1, h2l, w2l] bits
            hit = np.zeros(d.shape, bool)
            for e, (y, x) in enumerate(where):
                if side == "source":
                    hit[e, y, x] = True
                elif (y >> l) < d.shape[3] and (x >> l) < d.shape[4]:    # (a last odd row or column has no ancestor: floored sizes)
                    hit[e, :, :, y >> l, x >> l] = True
            assert hit.any() or l > 0
            finite = (d & 0x7C00) != 0x7C00
            assert not finite[hit].any(), "%s level %d: %d entries of the poisoned %s are finite" % (
                name, l, int(finite[hit].sum()), "row" if side == "source" else "column")
            leak = np.argwhere((d != k) & ~hit)
            assert len(leak) == 0, "%s level %d: [edge, y1, x1, ty, tx] = %s holds 0x%04x, the clean build 0x%04x (%d entries)" % (
                name, l, tuple(int(v) for v in leak[0]), d[tuple(leak[0])], k[tuple(leak[0])], len(leak))


def test_subnormal_operands_against_the_reference_operation():
    """the arbiter the statement names for subnormals: torch.matmul on the same quartered halves on the device.  What it and the
    build's kernels do with subnormal operands and results is pinned here: both keep them, as the statement does."""
    C, h, w = 128, 8, 8
    f1, f2 = S.cls_range(1, C, h, w, h, w, 2)
    a = torch.from_numpy(S.quarter(f1).reshape(1, C, h * w)).cuda()
    b = torch.from_numpy(S.quarter(f2).reshape(1, C, h * w)).cuda()
    ref = torch.matmul(a.transpose(1, 2), b).cpu().numpy().reshape(1, h, w, h, w)
    lo, hi = S.interval(f1, f2)
    assert ((ref >= lo) & (ref <= hi)).all()
    a32 = torch.matmul(a.float().transpose(1, 2), b.float()).cpu().numpy()
    assert (np.abs(a32) > 0).mean() > 0.7        # subnormal x normal products are there to be kept or lost


def test_the_forms_behind_the_environment_switches(tmp_path):
    """DBA_BUILD_WAVES=8, DBA_BUILD_KERNEL=classic and DBA_BUILD_OPERANDS=copy are read once per process: one child session per
    setting, one after another, each under its own time limit, runs the exact and naming cases of the C = 128 lines; the reported
    route must show the forced form (corr_build_cases.FORCED).  The first child that does not exit 0 ends the test."""
    if FORCED_NOW:
        return      # (a child of this very test)
    me = os.path.abspath(__file__)
    for setting in S.FORCED:
        key, val = setting.split("=")
        env = dict(os.environ)
        env[key] = val
        cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
               me + "::test_every_line_matches_the_statement", "-k", "C128- and (exact or naming)"]
        log = os.path.join(str(tmp_path), key + ".log")
        with open(log, "w+") as f:
            try:
                rc = subprocess.run(cmd, env=env, stdout=f, stderr=subprocess.STDOUT, timeout=CHILD_LIMIT).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            f.seek(0)
            tail = f.read()[-3000:]
        assert rc == 0, "%s: child session ended with %d\n%s" % (setting, rc, tail)
        assert " passed" in tail and "failed" not in tail, tail


def test_worst_use_of_the_bound_per_route():
    """what the random cases of this session used of the derived bound, per route (all below 1: asserted where measured)"""
    for route in sorted(WORST):
        print("worst |err| / bound on %-26s %.4f" % (route, WORST[route]))
        assert WORST[route] < 1.0
