"""Plain numpy restatement of the reference's edge retirement, statement by statement, on a state held as a dict of
arrays:

  rm_factors   <- CovisibleGraph.rm_factors (dbaf/covisible_graph.py:152-176)
  retire_mask  <- the mask of dbaf/dbaf_frontend.py:235-239
  rm_keyframe  <- CovisibleGraph.rm_keyframe (dbaf/covisible_graph.py:180-211)
  shift_edges  <- the edge statements of DBAFusionFrontend.__rollup (dbaf/dbaf_frontend.py:106-118)

A state has ii, jj, age, target, weight, net, inp (net / inp may be None), ii_inac, jj_inac, target_inac, weight_inac,
ii_bad, jj_bad, corr (the CorrBlock's rows as a 1-D array of slot ids, or None) and, for rm_keyframe, the nine video
buffers under their reference names.  Every function returns a NEW state and leaves its input alone.
Test infrastructure: tests/test_factors_model.py holds it against states recorded from the reference's own code
(tests/golden/factor_edits.npz); tests/test_gpu_factors.py holds the device against it."""
import numpy as np

EDGE_KEYS = ("ii", "jj", "age", "target", "weight", "net", "inp", "ii_inac", "jj_inac", "target_inac", "weight_inac",
             "ii_bad", "jj_bad", "corr")
VIDEO_KEYS = ("images", "poses", "disps", "disps_sens", "intrinsics", "nets", "inps", "fmaps", "tstamp")


def copy_state(st):
    return {k: (None if v is None else np.array(v, copy=True)) for k, v in st.items()}


def rm_factors(st, mask, store=False):
    st = copy_state(st)
    mask = np.asarray(mask, dtype=bool)
    if store:   # :157-161
        st["ii_inac"] = np.concatenate([st["ii_inac"], st["ii"][mask]], 0)
        st["jj_inac"] = np.concatenate([st["jj_inac"], st["jj"][mask]], 0)
        st["target_inac"] = np.concatenate([st["target_inac"], st["target"][:, mask]], 1)
        st["weight_inac"] = np.concatenate([st["weight_inac"], st["weight"][:, mask]], 1)
    for k in ("ii", "jj", "age"):   # :163-165
        st[k] = st[k][~mask]
    if st.get("corr") is not None:   # :167-168
        st["corr"] = st["corr"][~mask]
    for k in ("net", "inp", "target", "weight"):   # :170-176
        if st[k] is not None:
            st[k] = st[k][:, ~mask]
    return st


def retire_mask(st, max_age, oldest, mode="or"):
    """dbaf_frontend.py:235-239"""
    old = (st["ii"] < oldest) | (st["jj"] < oldest)
    aged = st["age"] > max_age
    return (aged | old) if mode == "or" else (aged & old)


def retire_edges(st, max_age, oldest, mode="or"):
    return rm_factors(st, retire_mask(st, max_age, oldest, mode), store=True)


def rm_keyframe(st, ix):
    st = copy_state(st)
    for k in VIDEO_KEYS:   # :185-195
        st[k][ix] = st[k][ix + 1]
    m = (st["ii_inac"] == ix) | (st["jj_inac"] == ix)   # :197
    st["ii_inac"][st["ii_inac"] >= ix] -= 1
    st["jj_inac"][st["jj_inac"] >= ix] -= 1
    if m.any():   # :201-205
        st["ii_inac"], st["jj_inac"] = st["ii_inac"][~m], st["jj_inac"][~m]
        st["target_inac"], st["weight_inac"] = st["target_inac"][:, ~m], st["weight_inac"][:, ~m]
    m = (st["ii"] == ix) | (st["jj"] == ix)   # :207
    st["ii"][st["ii"] >= ix] -= 1
    st["jj"][st["jj"] >= ix] -= 1
    return rm_factors(st, m, store=False)


def shift_edges(st, roll):
    st = copy_state(st)
    for k in ("ii", "jj", "ii_inac", "jj_inac"):   # :106-109
        st[k] = st[k] - roll
    keep = (st["ii_inac"] >= 0) & (st["jj_inac"] >= 0)   # :110
    st["ii_inac"], st["jj_inac"] = st["ii_inac"][keep], st["jj_inac"][keep]
    st["target_inac"], st["weight_inac"] = st["target_inac"][:, keep], st["weight_inac"][:, keep]
    st["ii_bad"], st["jj_bad"] = st["ii_bad"] - roll, st["jj_bad"] - roll   # :116-117
    return st


# ---- seeded random states (shared by the CPU and the GPU tests) ---------------------------------------------------------

def random_state(seed, h, w, n=None, n_inac=None, frames=12, channels=128, with_net=True, with_video=False,
                 image_hw=None):
    """a graph state shaped like the reference's: edges among `frames` keyframes, payloads of random bits"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(6, 28)) if n is None else n
    n_inac = int(rng.integers(3, 14)) if n_inac is None else n_inac

    def f32(*shape):   # random bits (NaN patterns included: everything here only moves bytes)
        return rng.integers(0, 2 ** 32, shape, dtype=np.uint32).view(np.float32)

    def f16(*shape):
        return rng.integers(0, 2 ** 16, shape, dtype=np.uint16).view(np.float16)

    # (the index lists are drawn first, so that they do not depend on the map shape)
    st = dict(ii=rng.integers(0, frames, n).astype(np.int64), jj=rng.integers(0, frames, n).astype(np.int64),
              age=rng.integers(0, 30, n).astype(np.int64),
              ii_inac=rng.integers(0, frames, n_inac).astype(np.int64),
              jj_inac=rng.integers(0, frames, n_inac).astype(np.int64),
              ii_bad=rng.integers(0, frames, 3).astype(np.int64), jj_bad=rng.integers(0, frames, 3).astype(np.int64),
              corr=rng.permutation(n).astype(np.int64))
    st.update(target=f32(1, n, h, w, 2), weight=f32(1, n, h, w, 2),
              net=f16(1, n, channels, h, w) if with_net else None, inp=f16(1, n, channels, h, w) if with_net else None,
              target_inac=f32(1, n_inac, h, w, 2), weight_inac=f32(1, n_inac, h, w, 2))
    if with_video:
        B = frames + 1
        ih, iw = image_hw if image_hw is not None else (8 * h, 8 * w)
        st.update(images=rng.integers(0, 256, (B, 3, ih, iw)).astype(np.uint8), poses=f32(B, 7), disps=f32(B, h, w),
                  disps_sens=f32(B, h, w), intrinsics=f32(B, 4), nets=f16(B, channels, h, w), inps=f16(B, channels, h, w),
                  fmaps=f16(B, 1, channels, h, w), tstamp=rng.integers(0, 2 ** 40, B).astype(np.float64))
    return st


# the parametrisation of the random-state tests: the four config map shapes and the seeds of each
SHAPES = [(64, 64), (55, 55), (28, 107), (48, 64)]
SEEDS = list(range(8))
RETIRE_MAX_AGE, RETIRE_OLDEST = 15, 5   # ages are uniform in [0, 30), frames in [0, 12)
ROLL = 3


def state_seed(h, w, seed):
    return 1000 * h + w + 7919 * seed


def mask_for(st, seed):
    return np.random.default_rng(seed + 99).random(st["ii"].shape[0]) < 0.3


def keyframe_for(st, seed):
    """a frame that an active edge touches (as t1 - 2 always is), below the last video row"""
    return int(st["ii"][seed % st["ii"].shape[0]])
