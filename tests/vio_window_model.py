"""A numpy restatement of the window split of DepthVideo.ba's IMU branch (dbaf/depth_video.py:348-367, :388-390, :470-475):
the t0 rule, the marginalised selection over the old window's lists and the active selection over the call's lists.
Integers and copies only: every result is exact."""
import numpy as np

INPUT_KEYS = ("target", "weight", "eta", "ii", "jj")
CUR_KEYS = ("cur_ii", "cur_jj", "cur_target", "cur_weight", "cur_eta")


def window_start(lo, t1, last_t0, last_t1):
    """:348-356 -> (t0, entered)"""
    t0 = lo
    if last_t1 != t1 or last_t0 != t0:
        if last_t0 > t0:
            t0 = last_t0
        elif last_t0 == t0:
            t0 = last_t0
        else:
            return t0, True
    return t0, False


def marg_mask(cur_ii, cur_jj, last_t0, last_t1, t0):
    """:360-364"""
    return (cur_ii >= last_t0) & (cur_ii < t0) & (cur_ii < last_t1 - 2) & (cur_jj < last_t1 - 2)


def active_mask(ii, jj, t0):
    """:470"""
    return (ii >= t0) & (jj >= t0)


def split(st, lo, t1, last_t0, last_t1):
    """st: target, weight [N, 2, ht, wd], eta [n_kx, ht, wd], ii, jj [N] and, where the branch is entered, cur_ii, cur_jj,
    cur_target, cur_weight, cur_eta -> dict(t0, entered, marg (None or dict(ii, jj, target, weight, eta, t0, t1)),
    cur dict(ii, jj, target, weight, eta), ii_min)"""
    t0, entered = window_start(lo, t1, last_t0, last_t1)
    marg = None
    if entered:
        m = marg_mask(st["cur_ii"], st["cur_jj"], last_t0, last_t1, t0)
        m_ii, m_jj = st["cur_ii"][m], st["cur_jj"][m]
        marg = dict(ii=m_ii, jj=m_jj, target=st["cur_target"][m], weight=st["cur_weight"][m], eta=None, t0=last_t0, t1=t0 + 1)
        if len(m_ii) > 0:                                                       # :370-372, :390
            marg["t1"] = int(m_jj.max()) + 1
            marg["eta"] = st["cur_eta"][0:marg["t1"] - marg["t0"]]
    a = active_mask(st["ii"], st["jj"], t0)
    ii_min = int(st["ii"].min())
    cur = dict(ii=st["ii"][a], jj=st["jj"][a], target=st["target"][a], weight=st["weight"][a], eta=st["eta"][(t0 - ii_min):])
    return dict(t0=t0, entered=entered, marg=marg, cur=cur, ii_min=ii_min)


MODES = ("moved", "moved_alternate", "moved_none", "standing", "ahead_mixed", "ahead_alternate", "ahead_none")


def random_state(n, n_cur, h, w, seed, mode, frames=40):
    """n call edges and n_cur edges of the old window over `frames` keyframes, small payloads
    -> (st, dict(lo, t1, last_t0, last_t1)) with lo = min(min ii, min jj), t1 = max + 1 as ba_inputs returns them.
      moved            branch entered, every call edge active; the marginalised selection random
      moved_alternate  ... every other edge of the old window selected
      moved_none       ... none selected
      standing         last_t0 == lo, last_t1 == t1: no branch, every edge active
      ahead_mixed      last_t0 > lo: t0 = last_t0, the active selection random
      ahead_alternate  ... every other call edge active
      ahead_none       ... none active"""
    assert mode in MODES
    r = np.random.default_rng(seed)
    lo, t1 = 12, frames
    ii, jj = r.integers(lo, t1, n), r.integers(lo, t1, n)
    if mode.startswith("moved"):
        last_t0, last_t1 = 4, t1 - 1
    elif mode == "standing":
        last_t0, last_t1 = lo, t1
    else:
        last_t0, last_t1 = (t1 + 3 if mode == "ahead_none" else 20), t1
        if mode == "ahead_alternate":
            ii[0::2], jj[0::2] = r.integers(last_t0, t1, len(ii[0::2])), r.integers(last_t0, t1, len(ii[0::2]))
            k = len(ii[1::2])
            ii[1::2], jj[1::2] = r.integers(lo, last_t0, k), r.integers(lo, t1, k)
    ii[1], jj[0] = lo, t1 - 1                            # the list spans [lo, t1); (position 1 stays outside an `ahead` window)
    cur_ii, cur_jj = r.integers(0, last_t1, n_cur), r.integers(0, last_t1, n_cur)
    if mode == "moved_alternate":
        k = len(cur_ii[0::2])
        cur_ii[0::2], cur_jj[0::2] = r.integers(last_t0, lo, k), r.integers(0, last_t1 - 2, k)
        cur_ii[1::2] = r.integers(lo, last_t1, len(cur_ii[1::2]))
    elif mode == "moved_none":
        cur_ii = r.integers(lo, last_t1, n_cur)
    f = lambda *s: r.standard_normal(s).astype(np.float32)  # noqa: E731
    st = dict(ii=ii.astype(np.int64), jj=jj.astype(np.int64), target=f(n, 2, h, w), weight=np.abs(f(n, 2, h, w)) + 0.5,
              eta=f(t1 - lo, h, w))
    if mode.startswith("moved"):
        st.update(cur_ii=cur_ii.astype(np.int64), cur_jj=cur_jj.astype(np.int64), cur_target=f(n_cur, 2, h, w),
                  cur_weight=np.abs(f(n_cur, 2, h, w)) + 0.5, cur_eta=f(last_t1 - last_t0, h, w))
    sc = dict(lo=int(min(st["ii"].min(), st["jj"].min())), t1=int(max(st["ii"].max(), st["jj"].max())) + 1,
              last_t0=last_t0, last_t1=last_t1)
    assert (sc["lo"], sc["t1"]) == (lo, t1)
    return st, sc


def load_fixture(path):
    """-> [(name, input dict (INPUT_KEYS and, where video.cur_* was set, CUR_KEYS), scalars dict(lo, t1, last_t0, last_t1),
    recorded dict)]; recorded: t0, marg (None or the marginal init's arguments), cur (the active init's arguments),
    video_cur (video.cur_* afterwards), last_t0_after, last_t1_after"""
    out = []
    with np.load(path) as z:
        assert int(z["schema_version"]) == 1
        for name in [str(s) for s in z["states"]]:
            g = lambda k: z["%s__%s" % (name, k)]  # noqa: E731
            has = lambda k: "%s__%s" % (name, k) in z.files  # noqa: E731
            st = {k: g("in_" + k) for k in INPUT_KEYS}
            if has("in_cur_ii"):
                st.update({k: g("in_" + k) for k in CUR_KEYS})
            sc = {k: int(g(k)) for k in ("lo", "t1", "last_t0", "last_t1")}
            rec = dict(t0=int(g("out_t0")), marg=None, last_t0_after=int(g("last_t0_after")), last_t1_after=int(g("last_t1_after")),
                       entered=bool(g("entered")))
            if has("marg_ii"):
                rec["marg"] = dict(ii=g("marg_ii"), jj=g("marg_jj"), target=g("marg_target"), weight=g("marg_weight"),
                                   eta=g("marg_eta"), t0=int(g("marg_t0")), t1=int(g("marg_t1")))
            rec["cur"] = dict(ii=g("cur_ii"), jj=g("cur_jj"), target=g("cur_target"), weight=g("cur_weight"), eta=g("cur_eta"))
            rec["video_cur"] = dict(ii=g("video_cur_ii"), jj=g("video_cur_jj"), target=g("video_cur_target"),
                                    weight=g("video_cur_weight"), eta=g("video_cur_eta"))
            out.append((name, st, sc, rec))
    return out
