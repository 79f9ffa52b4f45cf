"""CPU half of tests/test_gpu_lookup_reproject.py: what the cases of tests/lookup_reproject_cases.py cover, measured on the
float64 statement alone; that a kernel which mixed up its intrinsics would sit at least 100 x outside the bound the device
is held to; and the shape check that CorrBlock.lookup_reprojected / lookup_motion run in front of their launch.  Runs
without a GPU; `pytest -s` shows every figure next to its assertion."""
import numpy as np
import pytest
import torch

import geom_cases as G
import lookup_reproject_cases as L

ALL_SHAPES = L.SHAPES + [L.PADDED_SHAPE]
IDS = lambda s: "%dx%d" % s   # noqa: E731


def test_the_edge_list():
    assert len(L.II) == len(L.JJ) == 14
    assert sorted(L.II[:12]) == sorted(L.JJ[:12]) == list(range(12))         # every frame a source once and a target once
    assert (L.II[:12] != L.JJ[:12]).all() and (L.II[12:] == L.JJ[12:]).all() and L.N_STEREO == 2
    used = set(L.II[L.SUBSET]) | set(L.JJ[L.SUBSET])
    assert used == set(range(L.USED_FRAMES)) and len(L.SUBSET) == 9 and (L.II[L.SUBSET[-2:]] == L.JJ[L.SUBSET[-2:]]).all()


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_cases_cross_the_depth_cuts_with_one_k_per_frame(shape):
    c = L.case(*shape)
    got = L.conditions(c)
    print("lookup reproject case %dx%d: %s" % (shape + (got,)))
    assert c["checked"]["intr"].shape == (12, 4) and c["checked"]["disps"].shape == (12,) + shape
    assert got["finite"] and got["k_rows_differ"]
    assert 0.1 <= got["invalid_share"] <= 0.35
    assert got["substituted"] >= 100
    assert got["in_band"] == 0              # no valid or Z < 0.1 decision inside geom_cases.BAND: nothing is exempt on the device
    if c["tiled"]:
        # a tile that streams whole whatever reference pixel the kernel picks, and one that must hand a pixel to the gather phase
        assert got["inlier_tiles"] >= 1 and got["outlier_tiles"] >= 1
        assert got["tiles"] == len(L.II) * -(-shape[0] // L.TILE_H) * -(-shape[1] // L.TILE_W)


def test_the_tiles_that_stream_whole_are_the_stereo_edges():
    """a stereo edge moves every pixel by 0.1 f d <= about 9 pixels sideways and not at all vertically; the other edges turn
    and move the camera.  The all-inlier tiles come from there: the edge list must keep its stereo edges."""
    for shape in L.TILED_SHAPES:
        all_px, _, any_touch = L.tile_spreads(L.case(*shape)["ref"]["coords"], *shape)
        whole = ((all_px <= L.SH_BAND) & any_touch).reshape(len(L.II), -1).sum(1)
        assert whole[-L.N_STEREO:].sum() >= 1, (shape, whole)


def test_tile_spreads_on_a_made_up_flow():
    ht, wd = 8, 32
    y, x = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    flat = np.stack([x + 2.5, y - 1.25], -1)[None]                            # one shear for every pixel
    a, t, any_touch = L.tile_spreads(flat, ht, wd)
    assert a.shape == (1, 2, 2) and (a == 0).all() and (t == 0).all() and any_touch.all()
    torn = flat.copy()
    torn[0, 5, 20, 0] += 9.0                                                  # one pixel thrown 9 columns away: tile (1, 1)
    a, t, _ = L.tile_spreads(torn, ht, wd)
    assert a[0, 1, 1] == 9 and t[0, 1, 1] == 9 and (np.delete(a.ravel(), 3) == 0).all()
    torn[0, 5, 20, 0] = 1e5                                                   # ... out of the plane: it takes no part any more
    a, t, _ = L.tile_spreads(torn, ht, wd)
    assert a[0, 1, 1] > 1e4 and t[0, 1, 1] == 0
    assert L.tile_counts(flat, ht, wd) == (4, 0, 4) and L.tile_counts(torn, ht, wd) == (3, 0, 4)
    a, _, any_touch = L.tile_spreads(flat[:, :7, :30], 7, 30)                 # a map that is no multiple of the tile
    assert a.shape == (1, 2, 2) and (a == 0).all() and any_touch.all()


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=IDS)
def test_a_kernel_with_the_wrong_k_is_100_bounds_away(shape):
    """The device comparison (assert_coords with C_COORD) can tell the three mix-ups apart from the right statement: each
    lies more than 100 * C_COORD * 2^-24 * A away on at least half the pixels of every edge on which it is a different
    statement at all.  On a stereo edge Ki IS Kj, so `Kj := Ki` and the swap are the right statement there (asserted);
    K[0] for every frame is wrong there too, because neither stereo frame is frame 0."""
    c = L.case(*shape)
    shares = L.wrong_k_shares(c)
    for nm, per_edge in shares.items():
        print("wrong K, %dx%d, %s: share of pixels > 100 bounds away per edge: %s" % (shape + (nm, np.round(per_edge, 3).tolist())))
    assert set(shares) == {"K[0] for every frame", "Kj := Ki", "Ki and Kj swapped"}
    ns = L.N_STEREO
    assert (shares["K[0] for every frame"] >= 0.5).all()
    for nm in ("Kj := Ki", "Ki and Kj swapped"):
        assert (shares[nm][:-ns] >= 0.5).all(), nm
        assert np.array_equal(L.wrong_k_variants(c)[nm][-ns:], c["ref"]["coords"][-ns:]), nm


# ---- the shape check of the wrapper ----------------------------------------------------------------------------------------

def _check_args(n_slots, ht, wd, shapes):
    return (n_slots, ht, wd, shapes["poses"], shapes["disps"], shapes["K"], shapes["ii"], shapes["jj"],
            getattr(torch, shapes["ii_dtype"]), getattr(torch, shapes["jj_dtype"]))


def test_shape_check_refuses_every_row_of_the_error_table():
    from dbaf_amd.corr import _check_reproject_shapes
    n, ht, wd = 14, 8, 12
    good = L.good_reproject_shapes(n, ht, wd)
    assert _check_reproject_shapes(*_check_args(n, ht, wd, good)) is None
    rows = L.reproject_arg_errors(n, ht, wd)
    assert len(rows) >= 20 and len({w for w, _ in rows}) == len(rows)
    for what, over in rows:
        assert set(over) <= set(good), what
        with pytest.raises(ValueError) as err:
            _check_reproject_shapes(*_check_args(n, ht, wd, dict(good, **over)))
        named = [k.split("_")[0] for k in over]                # the message names an operand the row changed
        names = dict(K="intrinsics")
        assert any(names.get(k, k) in str(err.value) for k in named), (what, str(err.value))
    # what the wrapper has always taken stays good: a shared K in three forms, leading 1s, any integer index dtype, longer poses
    for over in (dict(K=(4,)), dict(K=(1, 4)), dict(K=(1, 1, 4)), dict(K=(1, 12, 4)), dict(poses=(1, 12, 7)), dict(poses=(15, 7)),
                 dict(disps=(1, 12, ht, wd)), dict(ii_dtype="int32", jj_dtype="int32"), dict(ii_dtype="uint8")):
        assert _check_reproject_shapes(*_check_args(n, ht, wd, dict(good, **over))) is None
    # torch.Size and lists are shapes too
    assert _check_reproject_shapes(n, ht, wd, torch.Size([12, 7]), [12, ht, wd], torch.Size([4]), torch.Size([n]), [n],
                                   torch.int64, torch.int64) is None


def test_the_wrapper_checks_before_it_builds_or_launches():
    """CorrBlock._lookup_reprojected on a block whose build would raise: every row of the table is refused with ValueError in
    front of it, from both entry points; the good shapes get as far as the build"""
    from dbaf_amd.corr import CorrBlock

    class Reached(Exception):
        pass

    class Block(CorrBlock):
        def __init__(self, n, h1, w1):
            self.layout, self.n, self.h1, self.w1 = "sheared", n, h1, w1

        def _materialise(self):
            raise Reached()

    n, ht, wd = 14, 8, 12
    blk = Block(n, ht, wd)
    good = L.good_reproject_shapes(n, ht, wd)

    def tensors(shapes):
        t = {k: torch.zeros(shapes[k]) for k in ("poses", "disps", "K")}
        t.update({k: torch.zeros(shapes[k], dtype=getattr(torch, shapes[k + "_dtype"])) for k in ("ii", "jj")})
        return t["poses"], t["disps"], t["K"], t["ii"], t["jj"]

    for what, over in L.reproject_arg_errors(n, ht, wd):
        with pytest.raises(ValueError):
            blk._lookup_reprojected(*tensors(dict(good, **over)), None, None)
    with pytest.raises(Reached):
        blk._lookup_reprojected(*tensors(good), None, None)
