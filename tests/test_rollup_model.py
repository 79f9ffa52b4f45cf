"""CPU: the walk decomposition behind the in-place window rollup (tests/rollup_model.py), for every (R, roll) with
1 <= R <= 40 and -R <= roll <= 2R and every live-mode (R, roll, live); the grid arithmetic of dbaf_amd.rollup against
the model's; and what needs no device of the new entry point: it is declared, exported, bound, importable, and refuses
bad arguments on the host before anything is enqueued."""
import ctypes
import os
import re

import numpy as np
import pytest

import rollup_model as rm

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EXACT = [(R, roll) for R in range(1, 41) for roll in range(-R, 2 * R + 1)]
LIVE = [(R, roll, live) for R in range(1, 41) for live in range(R + 1) for roll in range(live + 1)]


def _rows(R, width=3):
    return np.arange(R * width, dtype=np.int64).reshape(R, width) + 1000


def test_walks_are_disjoint_and_cover_every_row_once():
    for R, roll in EXACT:
        ws = rm.walks(R, roll)
        assert len(ws) == rm.n_walks(R, roll)
        seen = sorted(r for rows, _ in ws for r in rows)
        if rm.reduced(R, roll) == 0:
            assert ws == [], (R, roll)   # nothing moves: the buffer is left out of the grid
        else:
            assert seen == list(range(R)), (R, roll)
            assert all(closed and len(rows) == R // len(ws) >= 2 for rows, closed in ws), (R, roll)


def test_applying_the_walks_is_np_roll():
    for R, roll in EXACT:
        x = _rows(R)
        got = rm.apply_walks(x.copy(), roll)
        assert np.array_equal(got, np.roll(x, -roll, 0)), (R, roll)


def test_live_walks_are_disjoint_chains_below_live():
    for R, roll, live in LIVE:
        ws = rm.walks(R, roll, live)
        seen = [r for rows, _ in ws for r in rows]
        assert len(seen) == len(set(seen)) and all(0 <= r < live for r in seen), (R, roll, live)
        assert all(not closed and len(rows) >= 2 for rows, closed in ws), (R, roll, live)
        written = sorted(r for rows, _ in ws for r in rows[:-1])
        assert written == (list(range(live - roll)) if roll else []), (R, roll, live)


def test_live_mode_is_the_slice_statement_and_leaves_the_other_rows_alone():
    for R, roll, live in LIVE:
        x = _rows(R)
        got = rm.apply_walks(x.copy(), roll, live)
        assert np.array_equal(got, rm.live_statement(x, roll, live)), (R, roll, live)
        assert np.array_equal(got[live - roll:], x[live - roll:]), (R, roll, live)


def test_the_reference_case_has_ten_cycles_of_eight_and_live_moves_37_rows():
    ws = rm.walks(80, 30)
    assert len(ws) == 10 and all(len(rows) == rm.GROUP for rows, _ in ws)
    assert sum(len(rows) - 1 for rows, _ in rm.walks(80, 30, 67)) == 37


def test_grid_of_a_call():
    # images of 80 x 3 x 512 x 512 bytes at a 16-byte base: 10 cycles x 192 chunks of 256 x 16 bytes
    assert rm.workgroups([(4096, 80, 3 * 512 * 512)], 30) == 1920
    assert rm.workgroups([(4096, 80, 28)], 30) == 10 and rm.vector_width(4096, 28) == 4
    assert rm.workgroups([(4100, 80, 16400)], 30) == 10 * 17   # a 4-byte-aligned base: 4100 elements of 4 bytes
    assert rm.workgroups([(4096, 7, 8)], 14, list_lens=(5,)) == 1    # only the list
    assert rm.workgroups([(4096, 7, 8)], 0, list_lens=(5,)) == 0
    assert rm.workgroups([(4096, 80, 16)], 30, 67) == 30 and rm.workgroups([(4096, 12, 16)], 4, 4) == 0


def test_the_statements_model_on_numpy():
    v = rm.make_video(3)
    w = rm.rollup_video_statements(rm.clone_video(v), 5)
    for nm in rm.VIDEO_BUFFERS:
        assert np.array_equal(getattr(w, nm).view(np.uint8), np.roll(getattr(v, nm), -5, 0).view(np.uint8)), nm
    assert (w.counter.value, w.last_t0, w.last_t1) == (v.counter.value - 5, v.last_t0 - 5, v.last_t1 - 5)
    assert np.array_equal(w.cur_ii, v.cur_ii - 5) and np.array_equal(w.cur_jj, v.cur_jj - 5)


# ---- the entry point, as far as it goes without a device --------------------------------------------------------------------

def test_header_declares_and_library_exports_dba_roll_rows():
    text = open(os.path.join(ROOT, "include", "dba_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+dba_roll_rows\s*\(", text)
    assert re.search(r"#define\s+DBA_MAX_ROLL_LISTS\s+4\b", text)
    from dbaf_amd import _lib
    assert "dba_roll_rows" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dba_roll_rows")


def test_module_imports_without_a_device_and_sizes_the_grid_as_the_model():
    from dbaf_amd import rollup
    assert set(rollup.stats) == {"launches", "host_reads"}
    assert rollup.VIDEO_BUFFERS == rm.VIDEO_BUFFERS and (rollup.MAX_BUFS, rollup.MAX_LISTS) == (rm.MAX_BUFS, rm.MAX_LISTS)
    for R, roll in EXACT:
        assert rollup.walks(R, roll) == (rm.reduced(R, roll), rm.n_walks(R, roll)), (R, roll)
    for R, roll, live in LIVE:
        assert rollup.walks(R, roll, live) == (roll, rm.n_walks(R, roll, live)), (R, roll, live)


def _call(bases, row_bytes, rows, roll, live=-1, lists=(), list_lens=(), n_bufs=None, n_lists=None):
    from dbaf_amd import _lib
    lib = _lib.load()
    n, m = len(bases), len(lists)
    b = (ctypes.c_void_p * max(n, 1))(*bases)
    rb = (ctypes.c_int64 * max(n, 1))(*row_bytes)
    r = (ctypes.c_int64 * max(n, 1))(*rows)
    lp = (ctypes.c_void_p * max(m, 1))(*lists)
    ll = (ctypes.c_int64 * max(m, 1))(*list_lens)
    return lib.dba_roll_rows(b, rb, r, n if n_bufs is None else n_bufs, roll, live, lp, ll, m if n_lists is None else n_lists,
                             None)


BAD = {
    "null base with rows and bytes": dict(bases=[None], row_bytes=[16], rows=[8], roll=3),
    "negative row size": dict(bases=[4096], row_bytes=[-16], rows=[8], roll=3),
    "negative row count": dict(bases=[4096], row_bytes=[16], rows=[-8], roll=3),
    "negative list length": dict(bases=[], row_bytes=[], rows=[], roll=3, lists=[4096], list_lens=[-1]),
    "null list with entries": dict(bases=[], row_bytes=[], rows=[], roll=3, lists=[None], list_lens=[4]),
    "13 buffers": dict(bases=[4096] * 13, row_bytes=[16] * 13, rows=[8] * 13, roll=3),
    "negative buffer count": dict(bases=[4096], row_bytes=[16], rows=[8], roll=3, n_bufs=-1),
    "5 lists": dict(bases=[], row_bytes=[], rows=[], roll=3, lists=[4096] * 5, list_lens=[4] * 5),
    "live past the rows": dict(bases=[4096], row_bytes=[16], rows=[8], roll=3, live=9),
    "roll past live": dict(bases=[4096], row_bytes=[16], rows=[8], roll=5, live=4),
    "negative roll in live mode": dict(bases=[4096], row_bytes=[16], rows=[8], roll=-1, live=4),
    "live past the rows of the second buffer": dict(bases=[4096, 8192], row_bytes=[16, 16], rows=[12, 8], roll=3, live=9),
    "grid past 2^31 - 1 workgroups": dict(bases=[4096], row_bytes=[2 ** 43], rows=[2], roll=1),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_bad_arguments_are_refused_on_the_host(what):
    assert _call(**BAD[what]) == -1, what   # DBA_ERR_ARG, before anything is enqueued: the addresses are not memory


@pytest.mark.parametrize("roll", [0, 7, 14, -7])
def test_a_call_that_moves_nothing_launches_nothing(roll):
    # the address is not memory and there may be no device: DBA_OK can only come from the early return
    assert _call([4096], [16], [7], roll, lists=[4096], list_lens=[0]) == 0
    assert _call([4096, None], [0, 16], [7, 0], 3) == 0       # no bytes per row; no rows
    assert _call([4096], [16], [12], 4, live=4) == 0          # live == roll: no frame survives, no row moves
    assert _call([], [], [], 3) == 0
