"""CPU: the statement of tests/upmask_cases.py against torch's own float32 convolution (which measures C_UPMASK), the band's
share on the cases' inputs, the constant frame, and the frame plan's statement."""
import math

import numpy as np
import pytest
import torch

import upmask_cases as MC


def _conv32(d):
    x, w, b = (torch.from_numpy(d[k].astype(np.float32)) for k in ("x", "w", "b"))
    return torch.nn.functional.conv2d(x, w.view(576, 128, 1, 1), b).numpy()


def test_c_upmask_is_four_times_torchs_own_float32_convolution():
    near = plain = 0.0
    for case in MC.CASES:
        for seed in MC.SEEDS:
            st = MC.statement(case, seed)
            n, p = MC.sum_ratio_f32(_conv32(MC.inputs(case, seed)), st["v"], st["a"], st["near"])
            near, plain = max(near, n), max(plain, p)
    print("torch float32 conv2d on the CPU against the float64 statement, in units of 2^-24 x A: at the planted pixel worst %.4g, "
          "4 x = %.4g, C_UPMASK = %.4g; elsewhere worst %.4g, 4 x = %.4g, C_UPMASK_PLAIN = %.4g"
          % (near, 4 * near, MC.C_UPMASK, plain, 4 * plain, MC.C_UPMASK_PLAIN))
    for worst, c in ((near, MC.C_UPMASK), (plain, MC.C_UPMASK_PLAIN)):
        assert worst > 0
        assert 4 * worst <= c <= math.ceil(4 * worst) + 1, "the constant is not 4 x the measurement rounded up"


@pytest.mark.parametrize("case", MC.CASES, ids=MC.case_id)
def test_band_share_and_statement(case):
    ht, wd, B, const = case
    for seed in MC.SEEDS:
        d, st = MC.inputs(case, seed), MC.statement(case, seed)
        share = float(st["band"].mean())
        print("%s seed %d: in-band share %.4f of %d entries, max A / |v| %.3g" % (
            MC.case_id(case), seed, share, st["band"].size, float((st["a"] / np.abs(st["v"])).max())))
        assert share <= MC.MAX_SHARE
        assert np.isfinite(st["mask"]).all() and st["up"].shape == (B, 8 * ht, 8 * wd)
        # torch's float32 convolution rounded to half obeys checks 1 and 2 itself
        MC.check_mask("torch conv32", _conv32(d).astype(np.float16), st)
        # a convex combination: inside the hull of the taps, up to the weights' half rounding
        t = MC.taps(d["disps"])
        hi = MC.lay(np.broadcast_to(t.max(1)[:, None, None], (B, 8, 8, ht, wd)))
        assert (st["up"] <= hi * (1 + 9 * 2.0 ** -11)).all() and (st["up"] >= 0).all()
        if const is not None:
            m = st["mask"][const].reshape(9, 64, ht, wd)
            assert (m == m[:1]).all(), "the constant frame's nine taps differ"
            want = MC.lay((MC.rnd(1.0 / 9.0, np.float16) * t[const:const + 1]).sum(1)[:, None, None]
                          * np.ones((1, 8, 8, 1, 1)))
            assert np.allclose(st["up"][const], want[0], rtol=0, atol=1e-12)


def test_planted_value_is_there_and_finite():
    for case in MC.CASES:
        d, st = MC.inputs(case, 0), MC.statement(case, 0)
        assert (d["x"] == np.float16(65504.0)).sum() == 1
        assert np.abs(st["v"]).max() < 65504.0


def test_plan_statement():
    names = [c[0] for c in MC.plan_cases()]
    assert {"sorted", "unsorted", "repeated", "n1", "single_frame", "every_row"} <= set(names)
    for name, ii, buffer in MC.plan_cases():
        uniq, inv = MC.plan_ref(ii)
        assert np.array_equal(uniq[inv], ii) and (np.diff(uniq) > 0).all() and uniq.max() < buffer and uniq.min() >= 0
        tu, ti = torch.unique(torch.from_numpy(ii), return_inverse=True)
        assert np.array_equal(tu.numpy(), uniq) and np.array_equal(ti.numpy(), inv)
        if name == "every_row":
            assert len(uniq) == buffer
        if name == "single_frame":
            assert len(uniq) == 1
