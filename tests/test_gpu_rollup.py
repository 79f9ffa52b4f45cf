"""GPU: the window rollup in place (dbaf_amd.rollup, csrc/rollup.hip), through the C ABI.

Everything here moves bytes and subtracts integers, so every comparison is exact (bytes, compared on the device).

  - exact mode equals torch.roll(x, -roll, 0) for every (R, roll) of CASES at every row shape of ROW_SHAPES (vector
    widths 1 to 16, a row of several chunks, a base that is only 4-byte aligned); the no-op rolls launch nothing;
  - twelve different buffers in one call are one launch; a buffer past 2^31 bytes;
  - live mode equals the slice statement and leaves every other row as it was;
  - rollup_video equals the reference's statements said again in tests/rollup_model.py, keeps every data_ptr(),
    allocates nothing, is one launch and no host read; with cur_ii / cur_jj None as well;
  - rollup equals shift_edges and rollup_video applied separately;
  - the argument errors, each raised before any launch."""
import types

import numpy as np
import pytest
import torch

import factors_model as fm
import rollup_model as rm
from dbaf_amd import factors as fx
from dbaf_amd import rollup as ru

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [(8, 3), (12, 4), (12, 8), (37, 30), (80, 30), (8, 11), (8, -3), (7, 0), (7, 7), (7, 14), (1, 5)]
NO_OPS = {(7, 0), (7, 7), (7, 14), (1, 5)}   # (1, 5): a single row rolls onto itself
LIVE_CASES = [(80, 30, 67), (12, 4, 9), (12, 4, 4), (12, 4, 12), (8, 3, 3)]

# (name, dtype, row shape, rows sliced off the front of a larger buffer)
ROW_SHAPES = [("bool", torch.bool, (), 0), ("uint8x3", torch.uint8, (3,), 0), ("float64", torch.float64, (), 0),
              ("float32x7", torch.float32, (7,), 0), ("float32x4", torch.float32, (4,), 0),
              ("float16x5x9", torch.float16, (5, 9), 0), ("uint8x16400", torch.uint8, (16400,), 0),
              ("float32x7_base1", torch.float32, (7,), 1)]


def _random(dtype, shape, seed):
    """random bytes of the given dtype and shape on the device (bool: random 0 / 1)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    if dtype == torch.bool:
        return torch.randint(0, 2, shape, device=DEV, generator=gen).bool()
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device=DEV, generator=gen).view(dtype).reshape(shape)


def _buffer(R, dtype, row, front, seed):
    """(the buffer of R rows, the tensor that owns its memory)"""
    whole = _random(dtype, (R + front,) + row, seed)
    x = whole[front:]
    assert x.is_contiguous() and (front == 0 or x.data_ptr() % 8 == 4)
    return x, whole


def _bytes_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- exact mode -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,roll", CASES)
def test_exact_mode_is_torch_roll(R, roll):
    for k, (name, dtype, row, front) in enumerate(ROW_SHAPES):
        x, whole = _buffer(R, dtype, row, front, 100 * R + k)
        want, head = torch.roll(x, -roll, 0), whole[:front].clone()
        ptr, s0 = x.data_ptr(), dict(ru.stats)
        launches = ru.roll_rows([x], roll)
        assert launches == (0 if (R, roll) in NO_OPS else 1), name
        assert ru.stats["launches"] - s0["launches"] == launches and ru.stats["host_reads"] == s0["host_reads"], name
        assert x.data_ptr() == ptr and _bytes_equal(x, want), (name, R, roll)
        assert _bytes_equal(whole[:front], head), name   # the row in front of a sliced buffer is not the buffer's


def test_an_all_no_op_call_launches_nothing():
    bufs = [_random(torch.float32, (7, 4), 1), _random(torch.uint8, (1, 3), 2), _random(torch.float64, (14,), 3)]
    keep = [b.clone() for b in bufs]
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    s0 = dict(ru.stats)
    assert ru.roll_rows(bufs, 14, lists=[empty]) == 0 and ru.roll_rows(bufs, 0) == 0 and ru.roll_rows([], 3) == 0
    assert ru.stats == s0
    assert all(_bytes_equal(b, k) for b, k in zip(bufs, keep))


def test_twelve_different_buffers_are_one_launch():
    spec = [(80, torch.float64, ()), (80, torch.uint8, (3, 16, 24)), (37, torch.bool, ()), (12, torch.bool, ()),
            (80, torch.float32, (7,)), (40, torch.float32, (2, 3)), (8, torch.float32, (55, 55)), (9, torch.float32, (16, 24)),
            (80, torch.float32, (4,)), (7, torch.float16, (2, 128, 2, 3)), (30, torch.float16, (128, 2, 3)),
            (1, torch.float16, (5,))]
    bufs = [_random(dt, (R,) + row, 7 + k) for k, (R, dt, row) in enumerate(spec)]
    ii = torch.arange(40, 40 + 600, device=DEV)   # three workgroups of the list
    jj = torch.arange(50, 55, device=DEV)
    want = [torch.roll(b, -30, 0) for b in bufs]
    s0 = dict(ru.stats)
    assert ru.roll_rows(bufs, 30, lists=[ii, jj]) == 1
    assert ru.stats["launches"] - s0["launches"] == 1 and ru.stats["host_reads"] == s0["host_reads"]
    for k, (b, w) in enumerate(zip(bufs, want)):
        assert _bytes_equal(b, w), spec[k]
    assert torch.equal(ii, torch.arange(10, 610, device=DEV)) and torch.equal(jj, torch.arange(20, 25, device=DEV))


def test_four_lists_and_no_buffer():
    lists = [torch.arange(n, device=DEV) * 3 for n in (1, 256, 257, 1000)]
    want = [x + 4 for x in lists]
    assert ru.roll_rows([], -4, lists=lists) == 1
    assert all(torch.equal(x, w) for x, w in zip(lists, want))


def test_rows_past_two_to_the_31_bytes():
    x = _random(torch.uint8, (3, 2 ** 30), 5)   # row 2 starts at byte 2^31
    want = torch.roll(x, -1, 0)
    assert ru.roll_rows([x], 1) == 1
    assert torch.equal(x, want)


# ---- live mode ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R,roll,live", LIVE_CASES)
def test_live_mode_moves_the_live_rows_only(R, roll, live):
    for k, (name, dtype, row, front) in enumerate(ROW_SHAPES):
        x, whole = _buffer(R, dtype, row, front, 100 * R + live + k)
        old, head = x.clone(), whole[:front].clone()
        launches = ru.roll_rows([x], roll, live=live)
        assert launches == (1 if live > roll else 0), name
        assert _bytes_equal(x[:live - roll], old[roll:live]), (name, R, roll, live)
        assert _bytes_equal(x[live - roll:], old[live - roll:]), (name, R, roll, live)
        assert _bytes_equal(whole[:front], head), name


# ---- the reference's objects ----------------------------------------------------------------------------------------------

def _upload(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def host_video():
    """16 x 24 images (2 x 3 maps), buffer = 12; shared and never written: every test uploads its own clones"""
    return rm.make_video(11, buffer=12, ht=16, wd=24)


@pytest.mark.parametrize("lists", ["set", "none"])
def test_rollup_video_is_the_reference_statements_in_place(host_video, lists):
    roll = 5
    v, ref = rm.clone_video(host_video, _upload), rm.clone_video(host_video, _upload)
    if lists == "none":
        v.cur_ii = v.cur_jj = ref.cur_ii = ref.cur_jj = None
    rm.rollup_video_statements(ref, roll)
    objs = {nm: getattr(v, nm) for nm in rm.VIDEO_BUFFERS}
    ptrs = {nm: x.data_ptr() for nm, x in objs.items()}
    torch.cuda.synchronize()
    s0, mem0 = dict(ru.stats), torch.cuda.memory_allocated()
    res = ru.rollup_video(v, roll)
    mem1 = torch.cuda.memory_allocated()
    assert res == dict(launches=1)
    assert ru.stats["launches"] - s0["launches"] == 1 and ru.stats["host_reads"] == s0["host_reads"]
    assert mem1 == mem0
    for nm in rm.VIDEO_BUFFERS:
        assert getattr(v, nm) is objs[nm] and getattr(v, nm).data_ptr() == ptrs[nm], nm
        assert _bytes_equal(getattr(v, nm), getattr(ref, nm)), nm
    assert (v.counter.value, v.last_t0, v.last_t1) == (ref.counter.value, ref.last_t0, ref.last_t1)
    assert (v.counter.value, v.last_t0, v.last_t1) == (host_video.counter.value - roll, host_video.last_t0 - roll,
                                                       host_video.last_t1 - roll)
    if lists == "none":
        assert v.cur_ii is None and v.cur_jj is None
    else:
        assert torch.equal(v.cur_ii, ref.cur_ii) and torch.equal(v.cur_jj, ref.cur_jj)
        assert torch.equal(v.cur_ii, _upload(host_video.cur_ii) - roll)


def test_rollup_video_live_moves_the_frames_and_leaves_the_dead_rows(host_video):
    roll, live = 5, host_video.counter.value   # 9 frames: rows 5..8 become rows 0..3
    v = rm.clone_video(host_video, _upload)
    assert ru.rollup_video(v, roll, live=live) == dict(launches=1)
    for nm in rm.VIDEO_BUFFERS:
        old = _upload(getattr(host_video, nm))
        assert _bytes_equal(getattr(v, nm)[:live - roll], old[roll:live]), nm
        assert _bytes_equal(getattr(v, nm)[live - roll:], old[live - roll:]), nm
    assert v.counter.value == live - roll and torch.equal(v.cur_jj, _upload(host_video.cur_jj) - roll)


def _graph(st):
    g = types.SimpleNamespace(corr_impl="volume", corr=None)
    for k in fm.EDGE_KEYS:
        if k != "corr":
            setattr(g, k, None if st[k] is None else _upload(st[k]))
    return g


def test_rollup_is_shift_edges_and_rollup_video(host_video):
    roll = 5
    st = fm.random_state(21, 2, 3, n=14, n_inac=9, channels=16)
    both = types.SimpleNamespace(video=rm.clone_video(host_video, _upload), graph=_graph(st), t1=9, count=9)
    apart = types.SimpleNamespace(video=rm.clone_video(host_video, _upload), graph=_graph(st))
    res = ru.rollup(both, roll)
    want = fx.shift_edges(apart.graph, roll)
    want.update(ru.rollup_video(apart.video, roll))
    assert res == want and 0 < res["kept_inactive"] and 0 < res["dropped_inactive"] and res["launches"] == 1
    model = fm.shift_edges(st, roll)
    for k in fm.EDGE_KEYS:
        if k != "corr":
            a, b = getattr(both.graph, k), getattr(apart.graph, k)
            assert _bytes_equal(a, b), k
            assert a.cpu().numpy().tobytes() == np.ascontiguousarray(model[k]).tobytes(), k
    for nm in rm.VIDEO_BUFFERS + ("cur_ii", "cur_jj"):
        assert _bytes_equal(getattr(both.video, nm), getattr(apart.video, nm)), nm
    assert both.video.counter.value == apart.video.counter.value == host_video.counter.value - roll
    assert (both.t1, both.count) == (9, 9)   # the caller's


# ---- errors ---------------------------------------------------------------------------------------------------------------

def _bad_calls():
    x = _random(torch.float32, (8, 4), 1)
    lst = torch.arange(5, device=DEV)
    return {
        "a CPU tensor": lambda: ru.roll_rows([x, torch.zeros(8, 4)], 3),
        "a CPU list": lambda: ru.roll_rows([x], 3, lists=[torch.arange(5)]),
        "a non-contiguous buffer": lambda: ru.roll_rows([_random(torch.float32, (8, 6), 2)[:, :4]], 3),
        "13 buffers": lambda: ru.roll_rows([x] * 13, 3),
        "5 lists": lambda: ru.roll_rows([x], 3, lists=[lst] * 5),
        "a list that is not int64": lambda: ru.roll_rows([x], 3, lists=[lst.int()]),
        "live past the rows": lambda: ru.roll_rows([x], 3, live=9),
        "roll past live": lambda: ru.roll_rows([x], 5, live=4),
    }, x, lst


@pytest.mark.parametrize("what", ["a CPU tensor", "a CPU list", "a non-contiguous buffer", "13 buffers", "5 lists",
                                  "a list that is not int64", "live past the rows", "roll past live"])
def test_errors_are_raised_before_any_launch(what):
    calls, x, lst = _bad_calls()
    keep_x, keep_l = x.clone(), lst.clone()
    s0 = dict(ru.stats)
    with pytest.raises(ValueError, match="roll_rows"):
        calls[what]()
    assert ru.stats == s0
    assert _bytes_equal(x, keep_x) and torch.equal(lst, keep_l)
