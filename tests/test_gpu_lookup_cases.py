"""GPU: every lookup kernel at every window position of the atlas (tests/lookup_cases.py), bit for bit against the C
oracle's lookup on the reference pyramid the GPU built.  No tolerance anywhere: every comparison is np.array_equal on the
uint16 (float32: uint32) views.

The maps are tiny, so BATCH tensors of the series go into one launch: the edges (and their feature maps) are repeated
BATCH times -- the volumes depend on the feature maps only -- and launch k looks tensors [k BATCH, (k + 1) BATCH) up.  The
oracle's answer for a map is computed once and shared by the reference layout, the three selections of the sheared
kernels and the slot-addressed lookup.

  * reference layout      corr_lookup_rows_kernel (coords [n, h, w, 2]); under DBA_REF_LOOKUP_KERNEL=generic, in a child
                          session, the half radius-3 instance of corr_lookup_kernel with its Half8 interior loads
  * sheared layout        corr_lookup_resident_kernel under every selection of the `lookup_kernel` fixture (these maps'
                          rows are no whole 64-pixel segments, so their planes are linear and the rows-over-tiles form,
                          which reads tiled planes only, hands them to the resident one -- the selection must still not
                          change a bit)
  * slot-addressed        dba_corr_lookup_pyramid_slots: three edges in slots (4, 0, 2) of five, other volumes between
  * corr_index_forward    radii 1..4, float32 and float16 (coords [n, 2, h, w]): the Float8 interior path, the per-tap
                          path of every radius and the planar-coordinate instance of the row-load kernel"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lookup_cases as LC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BATCH = 128          # tensors of the series per launch
CHANNELS = 16
FORCE = "DBA_REF_LOOKUP_KERNEL"
CHILD_LIMIT = 600    # seconds; the child needs about as long as the three reference-layout tests plus its start


def _oracle():
    from oracle import oracle as orc
    return orc


def _launches(series):
    """[T, E, h, w, 2] -> list of (tensor indices [BATCH], coords [BATCH * E, h, w, 2]); the last launch wraps around"""
    T = series.shape[0]
    out = []
    for c0 in range(0, T, BATCH):
        idx = np.arange(c0, c0 + BATCH) % T
        out.append((idx, np.ascontiguousarray(series[idx].reshape((-1,) + series.shape[2:]))))
    return out


def _first_difference(got, ref, coords, radius, what):
    """level, edge, pixel, ix0, iy0 of the first differing output of a launch (got / ref [n, L * rd * rd, h, w])"""
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    bad = np.argwhere(got.view(bits) != ref.view(bits))
    k, ch, y, x = (int(v) for v in bad[0])
    rd2 = (2 * radius + 1) ** 2
    lvl = ch // rd2
    org, frac = LC.window_origin(coords[k, y, x], lvl, radius)
    return ("%s: %d of %d outputs differ; first: level %d, edge %d (launch row %d), pixel %d (y %d, x %d), channel %d, ix0 %d, "
            "iy0 %d, fraction (%g, %g), coordinate (%r, %r): got %r, oracle %r"
            % (what, len(bad), got.size, lvl, k % LC.EDGES, k, y * got.shape[3] + x, y, x, ch % rd2, org[0], org[1], frac[0],
               frac[1], float(coords[k, y, x, 0]), float(coords[k, y, x, 1]), float(got[k, ch, y, x]), float(ref[k, ch, y, x])))


def _assert_bits(got, ref, coords, radius, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype
    bits = np.uint16 if got.dtype == np.float16 else np.uint32
    assert np.array_equal(got.view(bits), ref.view(bits)), _first_difference(got, ref, coords, radius, what)


_CASES = {}
MAP_ID = lambda m: "%dx%d" % m  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _CASES.clear()


def _case(hw):
    """a map's series, its repeated feature maps, the reference pyramid the GPU builds from them and the oracle's lookups:
    made once per map and shared by the tests of this module"""
    if hw in _CASES:
        return _CASES[hw]
    from dbaf_amd.corr import CorrBlock
    h, w = hw
    rng = np.random.default_rng(1000 * h + w)
    f1 = rng.standard_normal((1, LC.EDGES, CHANNELS, h, w)).astype(np.float16)
    f2 = rng.standard_normal((1, LC.EDGES, CHANNELS, h, w)).astype(np.float16)
    t1 = torch.from_numpy(f1).cuda().repeat(1, BATCH, 1, 1, 1)            # edge k of a launch is edge k % 3 of the map
    t2 = torch.from_numpy(f2).cuda().repeat(1, BATCH, 1, 1, 1)
    pyr = CorrBlock.build_pyramid(t1, t2, LC.LEVELS)
    for p in pyr:                                                          # every repetition got the same volumes
        v = p.view(torch.int16).unflatten(0, (BATCH, LC.EDGES))
        assert torch.equal(v, v[:1].expand_as(v))
    pyr_np = [p.cpu().numpy() for p in pyr]
    orc = _oracle()
    launches = _launches(LC.series_array(h, w))
    refs = [orc.corr_lookup_pyramid(pyr_np, c, LC.RADIUS) for _, c in launches]
    for r in refs:
        r.setflags(write=False)
    assert all((r != 0).any() for r in refs)
    _CASES[hw] = dict(h=h, w=w, t1=t1, t2=t2, pyr=pyr, launches=launches, refs=refs)
    return _CASES[hw]


def _run_block(cb, case, what):
    h, w = case["h"], case["w"]
    for k, ((_, coords), ref) in enumerate(zip(case["launches"], case["refs"])):
        out = cb(torch.from_numpy(coords)[None].cuda()).cpu().numpy()[0]
        assert out.shape == (BATCH * LC.EDGES, LC.LEVELS * 49, h, w)
        _assert_bits(out, ref, coords, LC.RADIUS, "%s, %d x %d, launch %d" % (what, h, w, k))


@pytest.mark.parametrize("hw", LC.MAPS, ids=MAP_ID)
def test_reference_layout_atlas(hw):
    from dbaf_amd.corr import CorrBlock
    case = _case(hw)
    cb = CorrBlock(case["t1"], case["t2"], num_levels=LC.LEVELS, radius=LC.RADIUS, layout="reference")
    _run_block(cb, case, "reference layout" + (" (%s=%s)" % (FORCE, os.environ[FORCE]) if os.environ.get(FORCE) else ""))
    for a, b in zip(cb.corr_pyramid, case["pyr"]):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))     # the oracle read the volumes the lookup read


@pytest.mark.parametrize("hw", LC.MAPS, ids=MAP_ID)
def test_sheared_layout_atlas(hw, lookup_kernel):
    from dbaf_amd.corr import CorrBlock
    case = _case(hw)
    cb = CorrBlock(case["t1"], case["t2"], num_levels=LC.LEVELS, radius=LC.RADIUS, layout="sheared")
    _run_block(cb, case, "sheared layout, kernel selection %s" % lookup_kernel)


@pytest.mark.parametrize("hw", [(8, 8), (11, 13)], ids=MAP_ID)
def test_slot_addressed_atlas(hw):
    """dba_corr_lookup_pyramid_slots: the map's three edges live in slots (4, 0, 2) of a five-slot store whose other slots
    hold other volumes; every row of a launch goes through the slot table"""
    from dbaf_amd import _lib
    case = _case(hw)
    h, w = hw
    lib = _lib.load()
    where = (4, 0, 2)
    gen = torch.Generator(device="cuda").manual_seed(7)
    stores = []
    for p in case["pyr"]:
        s = torch.randn((5,) + tuple(p.shape[1:]), generator=gen, device="cuda").to(torch.float16)
        s[list(where)] = p[:LC.EDGES]
        stores.append(s.contiguous())
    slots = torch.tensor(where * BATCH, dtype=torch.int32, device="cuda")
    ptrs = (ctypes.c_void_p * LC.LEVELS)(*[s.data_ptr() for s in stores])
    n = BATCH * LC.EDGES
    for k, ((_, coords), ref) in enumerate(zip(case["launches"], case["refs"])):
        c = torch.from_numpy(coords).cuda()
        out = torch.empty(n, LC.LEVELS * 49, h, w, dtype=torch.float16, device="cuda")
        _lib.check(lib.dba_corr_lookup_pyramid_slots(ptrs, ctypes.c_void_p(slots.data_ptr()), ctypes.c_void_p(c.data_ptr()),
                                                     ctypes.c_void_p(out.data_ptr()), n, h, w, h, w, LC.LEVELS, LC.RADIUS,
                                                     _lib.DBA_F16, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "dba_corr_lookup_pyramid_slots")
        _assert_bits(out.cpu().numpy(), ref, coords, LC.RADIUS, "slots (4, 0, 2) of 5, %d x %d, launch %d" % (h, w, k))


def test_generic_half_kernel_on_the_reference_layout_atlas_in_a_child_session():
    """DBA_REF_LOOKUP_KERNEL=generic is read once per process: one fresh pytest session runs the
    reference-layout atlas tests of this file under it.  One child, under a time limit, its exit status asserted, no retry;
    a session that already runs under the variable (the child itself) starts nothing."""
    if os.environ.get(FORCE):
        pytest.skip("this session already runs under %s=%s" % (FORCE, os.environ[FORCE]))
    me = os.path.join(HERE, "test_gpu_lookup_cases.py")
    env = dict(os.environ)
    env[FORCE] = "generic"
    run = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                          me + "::test_reference_layout_atlas"], env=env, capture_output=True, text=True, timeout=CHILD_LIMIT,
                         cwd=os.path.dirname(HERE))
    assert run.returncode == 0, "exit %d\n%s\n%s" % (run.returncode, run.stdout[-4000:], run.stderr[-1000:])
    assert "%d passed" % len(LC.MAPS) in run.stdout, run.stdout[-1000:]


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", [(8, 8), (9, 10)], ids=MAP_ID)
def test_corr_index_forward_atlas(hw, radius, dtype):
    """droid_backends.corr_index_forward on the level-0 atlas of its radius: window side 2 r + 2, origins from -(2 r + 3) to
    w + 1 (h + 1), both fractions, then the extras"""
    import droid_backends
    from droid_backends import _SHADOWS
    orc = _oracle()
    h, w = hw
    rng = np.random.default_rng(100 * h + 10 * w + radius)
    vol3 = (rng.standard_normal((LC.EDGES, h, w, h, w)) * 4).astype(dtype)
    vol = np.ascontiguousarray(np.tile(vol3, (BATCH, 1, 1, 1, 1)))
    tvol = torch.from_numpy(vol).cuda()
    series = LC.series_array(h, w, radius=radius, levels=(0,))
    assert series.shape[0] == (h + 2 * radius + 5) * (w + 2 * radius + 5) * 2 + 36
    rd = 2 * radius + 1
    was = _SHADOWS.enabled
    _SHADOWS.enabled = False      # the kernel itself, at every call (a flow-aligned shadow would answer later ones)
    try:
        for k, (_, coords) in enumerate(_launches(series)):
            planar = np.ascontiguousarray(coords.transpose(0, 3, 1, 2))
            ref = orc.corr_index_forward(vol, planar, radius)
            out, = droid_backends.corr_index_forward(tvol, torch.from_numpy(planar).cuda(), radius)
            got = out.cpu().numpy()
            assert got.shape == ref.shape == (BATCH * LC.EDGES, rd, rd, h, w)
            _assert_bits(got.reshape(-1, rd * rd, h, w), ref.reshape(-1, rd * rd, h, w), coords, radius,
                         "corr_index_forward %s r = %d, %d x %d, launch %d" % (np.dtype(dtype).name, radius, h, w, k))
    finally:
        _SHADOWS.enabled = was
