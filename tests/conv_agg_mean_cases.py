"""conv1 + ReLU + the frame mean in one launch (csrc/conv3x3_mean.hip: dba_conv3x3_mean_f16, dba_frame_members): the cases and a
float64 numpy statement.

The statement: c = half(conv(x) + bias) per edge (tests/conv3x3_cases.conv_c), r = relu(c), and per slot s the sum of r over the
edges e with inverse[e] == s divided by max(count, 1); entries of inverse outside [0, F) belong to no slot; an empty slot is 0.
In the exact cases x and w are small integers and the bias is an integer: every product and every sum, per edge and over a
slot's edges, is an integer below 2^24 and exact in float32 in any order, and |c| <= 2048 is exact in half.  A count of 1, 2
or 4 then divides exactly in float32, so the kernel's result is the statement rounded ONCE to half; a count of 3 is
half(float32(s) / float32(3)), the division the kernel makes."""
import functools

import numpy as np

import conv3x3_cases as CC

MAPS = [(5, 7), (16, 16), (17, 33), (3, 40)]          # one partial tile; one full tile; partial tiles both ways; a wide strip
CHANNELS = [(128, 128), (32, 64)]                      # GraphAgg's conv1; the smallest pair the BIAS variant takes
# (name, inverse, dim_size)
EDGE_LISTS = [
    ("n1", (0,), 1),
    ("one_frame", (0, 0, 0, 0), 1),
    ("interleaved", (2, 0, 2, 1, 0, 2, 3), 4),         # torch.unique's inverse of ii = [3, 0, 3, 1, 0, 3, 7]: counts 2, 1, 3, 1
    ("minus_one", (1, 0, -1, 1, 0), 2),
    ("empty_tail", (0, 1, 0), 3),                      # dim_size one larger than the highest slot in use
]
INTERLEAVED_II = (3, 0, 3, 1, 0, 3, 7)
MAX_N = max(len(e[1]) for e in EDGE_LISTS)
# the windows of the module tests: (edges, frames, ht, wd, ii)
WINDOWS = [(7, 4, 17, 33, INTERLEAVED_II), (12, 5, 5, 7, (0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 2, 2))]
WIN_IDS = ["n7_f4_17x33", "n12_f5_5x7"]
# member tables beyond one round of 256 edges and beyond 256 slots: (n, F, seed)
TABLE_CASES = [(1, 1, 0), (7, 4, 1), (256, 3, 2), (257, 300, 3), (600, 300, 4), (1000, 7, 5)]


def map_id(m):
    return "%dx%d" % m


def chan_id(c):
    return "c%d_o%d" % c


def members_ref(inverse, F):
    """-> (seg_start [F + 1], members [n]) int32: each slot's edges ascending, the tail behind seg_start[F] -1"""
    inverse = np.asarray(inverse, np.int64)
    seg, mem = [0], []
    for s in range(F):
        mem += [e for e in range(len(inverse)) if inverse[e] == s]
        seg.append(len(mem))
    mem += [-1] * (len(inverse) - len(mem))
    return np.array(seg, np.int32), np.array(mem, np.int32)


def table_case(n, F, seed):
    """an inverse of n entries over F slots with some entries outside [0, F)"""
    rng = np.random.default_rng(seed)
    inv = rng.integers(0, F, n).astype(np.int64)
    if n > 4:
        inv[rng.integers(0, n, max(1, n // 50))] = -1
        inv[rng.integers(0, n, max(1, n // 100))] = F
    inv.setflags(write=False)
    return inv


def frame_mean_ref(x, w, bias, inverse, F):
    """-> (mean [F, c_out, h, w] float64, sum of relu(c) per slot, count [F], c [n, c_out, h, w])"""
    c, _, _ = CC.conv_c(x, w, bias)
    r = CC.relu_ref(c)
    s = np.zeros((F,) + c.shape[1:], np.float64)
    count = np.zeros(F, np.int64)
    for e, slot in enumerate(inverse):
        if 0 <= slot < F:
            s[slot] += r[e]
            count[slot] += 1
    return s / np.maximum(count, 1).reshape(-1, 1, 1, 1).astype(np.float64), s, count, c


def half_of_division(s, count):
    """half(float32(s) / float32(max(count, 1))): what the kernel stores for a float32 sum s"""
    d = np.maximum(count, 1).astype(np.float32).reshape(-1, 1, 1, 1)
    q = s.astype(np.float32) / d
    assert q.dtype == np.float32
    return q.astype(np.float16)


@functools.lru_cache(maxsize=None)
def random_inputs(hw, channels):
    """x [MAX_N, c_in, h, w], w [c_out, c_in, 3, 3], bias [c_out] as half arrays; an edge list reads its first n rows"""
    (h, wd), (ci, co) = hw, channels
    rng = np.random.default_rng(1000 * h + 10 * wd + ci)
    x = rng.standard_normal((MAX_N, ci, h, wd)).astype(np.float16)
    w = (rng.standard_normal((co, ci, 3, 3)) / np.sqrt(9 * ci)).astype(np.float16)
    b = (0.1 * rng.standard_normal(co)).astype(np.float16)
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


EXACT_CHANNELS = (32, 64)
EXACT_MAP = (17, 33)
# counts 2, 1, 3, 1 and a frame of 4
EXACT_LISTS = [EDGE_LISTS[2], EDGE_LISTS[1]]


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """integers in [-2, 2]: 288 products of magnitude <= 4 per output, |c| <= 1152 + 3"""
    (h, wd), (ci, co) = EXACT_MAP, EXACT_CHANNELS
    rng = np.random.default_rng(77)
    x = rng.integers(-2, 3, (MAX_N, ci, h, wd)).astype(np.float16)
    w = rng.integers(-2, 3, (co, ci, 3, 3)).astype(np.float16)
    b = rng.integers(-3, 4, co).astype(np.float16)
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    """the statement of one exact edge list, computed once and shared"""
    _, inverse, F = [e for e in EXACT_LISTS if e[0] == name][0]
    x, w, b = exact_inputs()
    mean, s, count, c = frame_mean_ref(x[:len(inverse)], w, b, inverse, F)
    for a in (mean, s, count, c):
        a.setflags(write=False)
    return dict(mean=mean, sum=s, count=count, c=c, inverse=inverse, F=F)
