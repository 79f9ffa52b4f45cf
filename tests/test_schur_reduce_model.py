"""The transposing tree of csrc/common.h (wave_sum_transpose) against the pairing of wave_sum_to_lane63, both restated in
numpy float32: every one of the wave's 27 / 36 / 42 sums must come out with the same bits, and every value must end in exactly
one lane.

wave_sum_to_lane63 (six DPP adds, result in lane 63):  row_shr:1, :2, :4, :8 fold each 16-lane row into its lane 15 -- a lane
adds the value of the lane 1, 2, 4, 8 below it in its row, lanes without such a source add 0 --, row_bcast:15 adds lane 15 of
row r to every lane of row r + 1 for r + 1 in {1, 3}, row_bcast:31 adds lane 31 to rows 2 and 3."""
import numpy as np
import pytest

f32 = np.float32


def lane63_model(x):
    """x: [64] float32 -> the float lane 63 holds after wave_sum_to_lane63"""
    x = x.astype(f32).copy()
    lane = np.arange(64)
    for sh in (1, 2, 4, 8):
        moved = np.zeros(64, f32)
        has = (lane % 16) >= sh
        moved[has] = x[lane[has] - sh]
        x = (x + moved).astype(f32)
    moved = np.zeros(64, f32)
    for row in (1, 3):                      # row_bcast:15, row mask 0xa
        moved[16 * row:16 * row + 16] = x[16 * row - 1]
    x = (x + moved).astype(f32)
    moved = np.zeros(64, f32)
    moved[32:] = x[31]                      # row_bcast:31, row mask 0xc
    x = (x + moved).astype(f32)
    return x[63]


def transpose_model(v):
    """v: [64 lanes, N] float32 -> (totals [64], idx [64]) as wave_sum_transpose leaves them: at level b a lane keeps the first
    half of its values (bit b of the lane clear) or the second half (set), and adds the kept half of lane ^ 2^b's other half"""
    lanes = np.arange(64)
    cur = v.astype(f32).copy()
    halves, ns = [], []
    for b in range(6):
        n = cur.shape[1]
        h = (n + 1) // 2
        pad = np.zeros((64, 2 * h), f32)
        pad[:, :n] = cur
        up = ((lanes >> b) & 1).astype(bool)
        keep = np.where(up[:, None], pad[:, h:], pad[:, :h])
        send = np.where(up[:, None], pad[:, :h], pad[:, h:])
        cur = (keep + send[lanes ^ (1 << b)]).astype(f32)
        halves.append(h), ns.append(n)
    assert cur.shape[1] == 1
    pos, ok = np.zeros(64, np.int64), np.ones(64, bool)
    for b in reversed(range(6)):
        up = ((lanes >> b) & 1).astype(bool)
        pos = np.where(up, halves[b] + pos, pos)
        ok &= pos < ns[b]
    return cur[:, 0], np.where(ok, pos, -1)


def _inputs(n):
    rng = np.random.default_rng(100 + n)
    yield "normal", rng.standard_normal((64, n))
    yield "spread_2^+-20", rng.standard_normal((64, n)) * np.exp2(rng.integers(-20, 21, size=(64, n)))
    alt = np.abs(rng.standard_normal((64, n))) + 1.0
    alt *= np.where(np.arange(64)[:, None] % 2 == 0, 1.0, -1.0)
    yield "alternating_signs", alt * np.exp2(rng.integers(-20, 21, size=(1, n)))
    yield "cancelling_rows", np.concatenate([alt[:32], -alt[:32] * (1 + 2.0 ** -20)])
    one = np.zeros((64, n))
    one[np.arange(n) % 64, np.arange(n)] = 1e20
    yield "one_huge_lane_each", one + rng.standard_normal((64, n))
    yield "zeros_and_denormals", rng.standard_normal((64, n)) * 1e-42


@pytest.mark.parametrize("n", [42, 36, 27, 1, 2, 3, 64])
def test_transposing_tree_gives_the_bits_of_wave_sum_to_lane63(n):
    for name, v in _inputs(n):
        v = v.astype(f32)
        tot, idx = transpose_model(v)
        held = idx[idx >= 0]
        assert sorted(held.tolist()) == list(range(n)), (name, "every value in exactly one lane")
        for lane in np.nonzero(idx >= 0)[0]:
            want = lane63_model(v[:, idx[lane]])
            assert tot[lane].view(np.uint32) == want.view(np.uint32), (name, n, int(idx[lane]), tot[lane], want)
