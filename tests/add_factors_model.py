"""Plain numpy restatement of CovisibleGraph.add_factors (dbaf/covisible_graph.py:102-149), statement by statement, on a
state held as a dict of arrays (as tests/factors_model.py does for the retirement calls):

  add_factors  <- :102-149 with __filter_repeated_edges (:61-72) and rm_factors(mask, store=True) (:152-176)

A state has ii, jj, age, target, weight, net, inp, ii_inac, jj_inac, target_inac, weight_inac, the video's nets, inps and
fmaps [B, cams, C, h, w], and the CorrBlock as the two map operands it was given, corr_f1 / corr_f2 [1, n, C, h, w] (what
a recorder bound to the module's CorrBlock name holds after cat / __getitem__); net, inp, corr_f1, corr_f2 may be None.
`reproject(ii, jj)` stands for video.reproject: it returns the new target rows [1, n, h, w, 2] float32.

The one rule the reference leaves open is fixed here as the device fixes it: argsort(age) is STABLE (equal ages keep
their positions' order).  tests/test_add_factors_model.py holds this model against states recorded from the reference's
own code (tests/golden/add_factors.npz); tests/test_gpu_add_factors.py holds the device against it."""
import numpy as np

GRAPH_KEYS = ("ii", "jj", "age", "target", "weight", "net", "inp", "ii_inac", "jj_inac", "target_inac", "weight_inac",
              "corr_f1", "corr_f2")
VIDEO_KEYS = ("nets", "inps", "fmaps")


def copy_state(st):
    return {k: (None if v is None else np.array(v, copy=True)) for k, v in st.items()}


def filter_repeated_edges(st, ii, jj):   # :61-72
    eset = set(zip(st["ii"].tolist(), st["jj"].tolist())) | set(zip(st["ii_inac"].tolist(), st["jj_inac"].tolist()))
    keep = np.array([(int(i), int(j)) not in eset for i, j in zip(ii, jj)], dtype=bool).reshape(ii.shape)
    return ii[keep], jj[keep]


def eviction_mask(age, limit):
    """:121-122: ix = arange(len(age))[argsort(age)]; the mask over POSITIONS is ix >= limit"""
    return np.argsort(age, kind="stable") >= limit


def add_factors(st, ii, jj, remove, max_factors, reproject, corr_impl="volume"):
    """-> (the new state, dict(added, filtered, evicted)); the input is left alone"""
    st = copy_state(st)
    ii, jj = np.asarray(ii, dtype=np.int64).reshape(-1), np.asarray(jj, dtype=np.int64).reshape(-1)
    proposed = ii.shape[0]
    ii, jj = filter_repeated_edges(st, ii, jj)                                               # :112
    info = dict(added=int(ii.shape[0]), filtered=int(proposed - ii.shape[0]), evicted=0)
    if ii.shape[0] == 0:                                                                     # :114-115
        return st, info
    if max_factors > 0 and st["ii"].shape[0] + ii.shape[0] > max_factors and st["corr_f1"] is not None and remove:
        mask = eviction_mask(st["age"], max_factors - ii.shape[0])                           # :121-122
        info["evicted"] = int(mask.sum())
        st["ii_inac"] = np.concatenate([st["ii_inac"], st["ii"][mask]], 0)                   # :157-160
        st["jj_inac"] = np.concatenate([st["jj_inac"], st["jj"][mask]], 0)
        st["target_inac"] = np.concatenate([st["target_inac"], st["target"][:, mask]], 1)
        st["weight_inac"] = np.concatenate([st["weight_inac"], st["weight"][:, mask]], 1)
        for k in ("ii", "jj", "age"):                                                        # :162-164
            st[k] = st[k][~mask]
        for k in ("corr_f1", "corr_f2", "net", "inp", "target", "weight"):                   # :166-176
            if st[k] is not None and (corr_impl == "volume" or not k.startswith("corr")):
                st[k] = st[k][:, ~mask]
    net = st["nets"][ii][None]                                                               # :124
    if corr_impl == "volume":                                                                # :127-135
        c = (ii == jj).astype(np.int64)
        f1, f2 = st["fmaps"][ii, 0][None], st["fmaps"][jj, c][None]
        st["corr_f1"] = f1 if st["corr_f1"] is None else np.concatenate([st["corr_f1"], f1], 1)
        st["corr_f2"] = f2 if st["corr_f2"] is None else np.concatenate([st["corr_f2"], f2], 1)
        inp = st["inps"][ii][None]
        st["inp"] = inp if st["inp"] is None else np.concatenate([st["inp"], inp], 1)
    target = np.asarray(reproject(ii, jj), dtype=np.float32)                                 # :138-139
    weight = np.zeros_like(target)
    st["ii"] = np.concatenate([st["ii"], ii], 0)                                             # :141-143
    st["jj"] = np.concatenate([st["jj"], jj], 0)
    st["age"] = np.concatenate([st["age"], np.zeros_like(ii)], 0)
    st["net"] = net if st["net"] is None else np.concatenate([st["net"], net], 1)            # :146
    st["target"] = np.concatenate([st["target"], target], 1)                                 # :148-149
    st["weight"] = np.concatenate([st["weight"], weight], 1)
    return st, info


def make_golden_reproject(h, w):
    """the deterministic stand-in for video.reproject that tests/golden/make_add_factors_golden.py binds (small integers
    that name the edge and the pixel)"""
    def reproject(ii, jj):
        ii, jj = np.asarray(ii, dtype=np.int64), np.asarray(jj, dtype=np.int64)
        pix = np.arange(h * w * 2, dtype=np.int64).reshape(1, 1, h, w, 2)
        return (100 * ii + 10 * jj).reshape(1, -1, 1, 1, 1).astype(np.float32) + (pix % 7).astype(np.float32)
    return reproject


# ---- seeded random cases (shared by the CPU and the GPU tests) ---------------------------------------------------------

SHAPES = [(64, 64), (55, 55), (28, 107), (48, 64), (5, 7)]   # the four config map shapes and 5 x 7
SEEDS = list(range(8))
FRAMES = 12
BRANCHES = ("some_filtered", "none_filtered", "all_filtered", "eviction", "more_new_than_max_factors", "first_call",
            "stereo_edge", "over_limit_without_remove")


def case_seed(h, w, seed):
    return 1000 * h + w + 7919 * seed


def random_case(seed, h, w, scenario, channels=32, fmap_channels=128):
    """-> dict(state, ii, jj, remove, max_factors, cams, poses, disps, intrinsics).  `scenario` (0..7) picks the branch
    the case is built to take; the index lists are drawn before the payloads, so they do not depend on the map shape."""
    rng = np.random.default_rng(seed)
    first = scenario == 4
    cams = 2 if scenario in (5, 7) else 1
    n = 0 if first else int(rng.integers(6, 12))
    n_inac = 0 if first else int(rng.integers(2, 7))
    # distinct existing edges, drawn without replacement from the off-diagonal pairs
    pairs = [(i, j) for i in range(FRAMES) for j in range(FRAMES) if i != j]
    pick = rng.permutation(len(pairs))
    act = [pairs[k] for k in pick[:n]]
    inac = [pairs[k] for k in pick[n:n + n_inac]]
    free = [pairs[k] for k in pick[n + n_inac:]]
    age = rng.integers(0, 6 if scenario == 7 else 30, n).astype(np.int64)    # scenario 7: tied ages
    if scenario == 1 and n:
        age = rng.permutation(40)[:n].astype(np.int64)                       # pairwise distinct
    if scenario == 2:
        prop = [act[0], inac[0], act[-1]]
    elif scenario in (0, 7):
        prop = [free[0], act[1], free[1], inac[-1], free[2], free[1]]        # a duplicate inside the proposal stays
    else:
        prop = free[:int(rng.integers(3, 7))]
    if scenario in (5, 7):
        prop = prop + [(3, 3), (7, 7)]
    n_new = len([e for e in prop if e not in act and e not in inac])
    remove = scenario in (1, 3, 7)
    if scenario in (1, 6, 7):
        max_factors = n + n_new - int(rng.integers(1, min(4, n) + 1))        # a few over the limit
    elif scenario == 3:
        max_factors = max(n_new - 1, 1)                                      # n_new > max_factors: a negative limit
    else:
        max_factors = 48
    prop = np.array(prop, dtype=np.int64).reshape(-1, 2)

    def f32(*shape):   # random bits (NaN patterns included): these rows are only moved
        return rng.integers(0, 2 ** 32, shape, dtype=np.uint32).view(np.float32)

    def f16(*shape):
        return rng.integers(0, 2 ** 16, shape, dtype=np.uint16).view(np.float16)

    B = FRAMES + 1
    e = lambda lst, k: np.array([x[k] for x in lst], dtype=np.int64)  # noqa: E731
    fmaps = (rng.standard_normal((B, cams, fmap_channels, h, w)) * 0.5).astype(np.float16)
    st = dict(ii=e(act, 0), jj=e(act, 1), age=age, ii_inac=e(inac, 0), jj_inac=e(inac, 1),
              target=f32(1, n, h, w, 2), weight=f32(1, n, h, w, 2),
              net=None if first else f16(1, n, channels, h, w), inp=None if first else f16(1, n, channels, h, w),
              target_inac=f32(1, n_inac, h, w, 2), weight_inac=f32(1, n_inac, h, w, 2),
              nets=f16(B, channels, h, w), inps=f16(B, channels, h, w), fmaps=fmaps)
    c = (st["ii"] == st["jj"]).astype(np.int64)
    st["corr_f1"] = None if first else fmaps[st["ii"], 0][None]
    st["corr_f2"] = None if first else fmaps[st["jj"], c][None]
    # a plausible camera track: small motions, unit quaternions, positive inverse depths, one K per frame
    q = np.concatenate([0.05 * rng.standard_normal((B, 3)), np.ones((B, 1))], 1)
    poses = np.concatenate([0.2 * rng.standard_normal((B, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], 1)
    disps = rng.uniform(0.3, 2.0, (B, h, w))
    K = np.stack([w * rng.uniform(0.9, 1.1, B), w * rng.uniform(0.9, 1.1, B), w / 2 + rng.uniform(-1, 1, B),
                  h / 2 + rng.uniform(-1, 1, B)], 1)
    return dict(state=st, ii=prop[:, 0].copy(), jj=prop[:, 1].copy(), remove=remove, max_factors=int(max_factors), cams=cams,
                poses=poses.astype(np.float32), disps=disps.astype(np.float32), intrinsics=K.astype(np.float32))


def branches_taken(case, info):
    """which of BRANCHES the case took, from the model's (or the device's) counts"""
    st = case["state"]
    n, proposed = st["ii"].shape[0], case["ii"].shape[0]
    over = case["max_factors"] > 0 and n + info["added"] > case["max_factors"] and info["added"] > 0
    return {
        "some_filtered": 0 < info["filtered"] < proposed,
        "none_filtered": info["filtered"] == 0,
        "all_filtered": info["added"] == 0,
        "eviction": info["evicted"] > 0,
        "more_new_than_max_factors": info["added"] > case["max_factors"] > 0 and info["evicted"] == n > 0,
        "first_call": st["corr_f1"] is None and info["added"] > 0,
        "stereo_edge": info["added"] > 0 and bool((case["ii"] == case["jj"]).any()),
        "over_limit_without_remove": over and not case["remove"] and info["evicted"] == 0 and st["corr_f1"] is not None,
    }
