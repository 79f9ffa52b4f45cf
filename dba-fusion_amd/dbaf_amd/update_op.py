"""The update operator on the MI355X: the reference's UpdateModule and GraphAgg (dbaf/droid_net.py:40-142) with everything
around the ConvGRU that is not a convolution of 64 outputs or more in this project's own launches (csrc/update_op.hip,
csrc/gru.hip).

  heads(*specs)        the checked wrapper of dba_upd_heads: one or two 3x3 convolutions with one or two output channels in
                       ONE launch, each with an optional ReLU on its input, its bias, and nothing / sigmoid / softplus-and-
                       scale behind it, written as [n, ht, wd, k]
  Head(...)            one head of such a call
  clear_cast_cache(m)  forget the half copies of the small convolutions' parameters (after a write through `.data`)
  GraphAgg()           the reference's constructors, submodule names, nn.Sequential indices and forward parameter lists: a
  UpdateModule()       state dict of the reference loads unchanged.  GradientClip stays in place as a parameter-free module
                       (the identity in forward)

UpdateModule.forward, fused route: the two encoders run their convolutions and their FIRST ReLU as torch; their last ReLU
is applied by the GRU's pack while it copies (ConvGRU.forward_relu); delta[0] and weight[0] run as torch, and ONE heads call
reads their two outputs once: ReLU, the 128 -> 2 convolutions, the sigmoid and the [b, n, h, w, 2] layout.  GraphAgg's eta
head is the same kernel with one output, softplus and the factor .01.  forward_statements is the reference's chain in plain
torch ops, on any device.

Every fused piece routes on its own facts, as ConvGRU._fusable does: contiguous device tensors of one dtype in {float16,
float32}, the convolution answering in that dtype, nothing asking for a gradient; otherwise that piece runs the statements.
One more fact for eta: torch's autocast runs softplus in float32, so under autocast the statements answer in float32 from
a half convolution, and the piece runs them (the kernel rounds to the tensor dtype; it would lose those bits).  CPU tensors
raise.  No host synchronisation on the upsample=False path, work is enqueued on torch.cuda.current_stream(), memory comes
from torch's allocator only, and a forward can be captured into a hipGraph.

Upsample mode (upsample=True).  GraphAgg takes the frames of its edge list from frame_plan(ii, buffer) (csrc/upmask.hip,
dba_frame_plan) in place of torch.unique, and sizes the segmented mean by it: the first forward on an edge list reads the
plan's count once, every later forward on the same list reads nothing and can be captured.  `last_uniq` keeps the plan's
frames for the caller's `self.damping[uniq] = damping` and `video.upsample(uniq, upmask)`.  With `fuse_upmask` set (default
off: then nothing changes) and a half hidden state, the fifth return value is an UpmaskSource -- the operands of the mask's
1x1 convolution, not its result -- which dbaf_amd.upsample.upsample_disps_ consumes in ONE launch (dba_upmask_upsample_disp);
`.materialize()` gives the stock convolution's tensor to a caller that wants it.  Float32 modules, a gradient, a
non-contiguous state keep the two launches.

fuse_conv (default off: then nothing changes) forwards to the GRU (ConvGRU.fuse_conv) and routes corr_encoder[2],
flow_encoder[2] (their ReLUs stay deferred into pack) and GraphAgg.conv1 / conv2 (ReLU in the epilogue) through
dbaf_amd.conv.conv3x3 where its conditions hold.  corr_encoder[0] with its ReLU is one conv1x1 launch (196 channels: the
last chunk of 32 is filled with zeros).  The heads' first convolutions delta[0] / weight[0] with their ReLUs are ONE
conv3x3_pair launch that writes two plain contiguous [n, 128, ht, wd] tensors, which is what heads() reads (relu_in off: the
ReLU of half(c) is the reference's in-place ReLU).  With the flag, a forward with upsample=False then makes one stock
convolution call, the 7x7 flow stem.  Each piece routes on its own facts; where they fail, that piece alone keeps the
stock route.

fuse_flow_stem (default off: then nothing changes; independent of fuse_conv) routes flow_encoder[0] with its ReLU through
dbaf_amd.conv.conv7x7: ONE launch in place of the stem on MIOpen, the in-place ReLU behind it and, where the caller hands a
float32 flow under autocast (CorrBlock.lookup_motion does), autocast's cast in front of it -- the kernel rounds the float32
values to half as it reads them.  With both switches a forward with upsample=False makes no stock convolution call.

fuse_agg (default off: then nothing changes; GraphAgg's switch, UpdateModule.fuse_agg forwards to it; independent of the three
others) finishes upsample mode: conv1 / conv2 with their ReLUs go through conv3x3 as under fuse_conv; under autocast, eta is
ONE heads launch with Head.out_dtype = torch.float32 (v = s + b rounded once to half, softplus and the factor .01 in float32,
the dtype the statements return); the 128 -> 576 mask convolution is conv1x1 wherever forward called self.upmask(net), and
an UpmaskSource made under the switch materializes through conv1x1 too.  With fuse_conv and fuse_flow_stem as well, a forward
with upsample=True makes no stock convolution call, under autocast or not.  Each piece routes on its own facts.

fuse_mean (default off: then nothing changes; GraphAgg's switch, UpdateModule.fuse_mean forwards to it; independent of the four
others): conv1, its ReLU and the mean over each frame's edges are ONE launch (dbaf_amd.conv.conv3x3_frame_mean), with the bytes
of conv3x3(relu=True) + scatter_mean(dim_size=F); the [N, 128, ht, wd] tensor between them is never written.  It takes effect
where conv3x3's own facts hold for conv1 (contiguous half device tensors, nothing asking for a gradient) and batch == 1;
everything else keeps its present route, and so does a window whose frames x tiles grid conv.frame_mean_pays sends back to
the two launches (measured slower there).  The member table of an edge list is kept with its plan (frame_members): a standing
list launches nothing for it and reads nothing from the host.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import conv as _conv
from .gru import ConvGRU
from .upsample import UpmaskSource

ACTS = {"none": 0, "sigmoid": 1, "softplus": 2}   # DBA_UPD_ACT_* of include/dba_hip.h
_DTYPES = {torch.float32: _lib.DBA_F32, torch.float16: _lib.DBA_F16}


def _require(cond, msg):
    if not cond:
        raise ValueError("update_op (MI355X): " + msg)


def _overlap(x, y):
    a, b = x.data_ptr(), y.data_ptr()
    return a < b + y.numel() * y.element_size() and b < a + x.numel() * x.element_size()


class Head:
    """one head of a heads() call.  x [n, c, ht, wd]; weight [k, c, 3, 3], k in {1, 2}; bias [k] or None; relu_in: x is
    still before its ReLU; act: "none" | "sigmoid" | "softplus" (then out = scale * softplus(v), rounded after each);
    out: where to write [n, ht, wd, k] (default: a new tensor); want_sum: also return the float32 s + b; out_dtype: None
    (x's dtype) or torch.float32 -- then v = s + b is still rounded ONCE to x's dtype, and the activation and the scale
    behind it stay in float32, unrounded: what autocast's float32 softplus makes of a half convolution"""

    def __init__(self, x, weight, bias=None, relu_in=False, act="none", scale=1.0, out=None, want_sum=False, out_dtype=None):
        self.x, self.weight, self.bias, self.relu_in, self.act, self.scale = x, weight, bias, bool(relu_in), act, float(scale)
        self.out, self.want_sum, self.out_dtype = out, bool(want_sum), out_dtype


def tile():
    """(rows, cols) of the kernel's tile"""
    r, c = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().dba_upd_heads_tile(ctypes.byref(r), ctypes.byref(c)), "dba_upd_heads_tile")
    return r.value, c.value


def heads(*specs):
    """one launch for one or two Heads that share n, c, ht, wd, device and dtype -> a list, per head `out` [n, ht, wd, k], or
    (out, sum) where want_sum.  Raises ValueError before anything is enqueued."""
    _require(1 <= len(specs) <= 2 and all(isinstance(h, Head) for h in specs), "one or two Head specs, got %d" % len(specs))
    x0 = specs[0].x
    _require(isinstance(x0, torch.Tensor) and x0.is_cuda, "heads[0].x must be a HIP device tensor; no CPU path")
    _require(x0.dtype in _DTYPES, "heads[0].x must be float16 or float32, got %s" % x0.dtype)
    _require(x0.dim() == 4 and x0.numel() > 0, "heads[0].x must be a non-empty [n, c, ht, wd], got %s" % (tuple(x0.shape),))
    n, c, ht, wd = (int(s) for s in x0.shape)
    _require(n * c * ht * wd < 2 ** 31, "n * c * ht * wd must stay below 2^31, got %d" % (n * c * ht * wd))
    arr = (_lib.UpdHead * len(specs))()
    results, written, read = [], [], []
    for i, h in enumerate(specs):
        nm = "heads[%d]" % i
        _require(h.act in ACTS, "%s.act must be one of %s, got %r" % (nm, sorted(ACTS), h.act))
        for t, what in ((h.x, "x"), (h.weight, "weight")) + (((h.bias, "bias"),) if h.bias is not None else ()):
            _require(isinstance(t, torch.Tensor) and t.is_cuda, "%s.%s must be a HIP device tensor; no CPU path" % (nm, what))
            _require(t.device == x0.device and t.dtype == x0.dtype,
                     "%s.%s must be on %s in %s, got (%s, %s)" % (nm, what, x0.device, x0.dtype, t.device, t.dtype))
            _require(t.is_contiguous(), "%s.%s must be contiguous" % (nm, what))
            read.append((t, "%s.%s" % (nm, what)))
        _require(tuple(h.x.shape) == (n, c, ht, wd), "%s.x must be %s as heads[0].x, got %s" % (nm, (n, c, ht, wd), tuple(h.x.shape)))
        _require(h.weight.dim() == 4 and h.weight.shape[0] in (1, 2) and tuple(h.weight.shape[1:]) == (c, 3, 3),
                 "%s.weight must be [1 or 2, %d, 3, 3], got %s" % (nm, c, tuple(h.weight.shape)))
        k = int(h.weight.shape[0])
        _require(h.bias is None or tuple(h.bias.shape) == (k,), "%s.bias must be [%d]" % (nm, k))
        _require(h.out_dtype in (None, x0.dtype, torch.float32), "%s.out_dtype must be None, %s or torch.float32, got %r"
                 % (nm, x0.dtype, h.out_dtype))
        odt = x0.dtype if h.out_dtype is None else h.out_dtype
        if h.out is None:
            out = torch.empty((n, ht, wd, k), dtype=odt, device=x0.device)
        else:
            out = h.out
            _require(isinstance(out, torch.Tensor) and out.is_cuda and out.device == x0.device and out.dtype == odt
                     and out.is_contiguous() and tuple(out.shape) == (n, ht, wd, k),
                     "%s.out must be a contiguous [%d, %d, %d, %d] of %s on %s" % (nm, n, ht, wd, k, odt, x0.device))
        s = torch.empty((n, ht, wd, k), dtype=torch.float32, device=x0.device) if h.want_sum else None
        written.append((out, nm + ".out"))
        arr[i] = _lib.UpdHead(h.x.data_ptr(), h.weight.data_ptr(), h.bias.data_ptr() if h.bias is not None else None,
                              out.data_ptr(), s.data_ptr() if s is not None else None, k, int(h.relu_in), ACTS[h.act], h.scale,
                              int(odt != x0.dtype))
        results.append((out, s) if h.want_sum else out)
    for i, (o, onm) in enumerate(written):
        for t, tnm in read:
            _require(not _overlap(o, t), "%s overlaps %s" % (onm, tnm))
        for o2, onm2 in written[i + 1:]:
            _require(not _overlap(o, o2), "%s overlaps %s" % (onm, onm2))
    stream = ctypes.c_void_p(torch.cuda.current_stream(x0.device).cuda_stream)
    with torch.cuda.device(x0.device):
        _lib.check(_lib.load().dba_upd_heads(arr, len(specs), n, c, ht, wd, _DTYPES[x0.dtype], stream), "dba_upd_heads")
    return results


class _ClipGrad(torch.autograd.Function):
    """the identity; on the way back a gradient entry that is NaN or larger than 0.01 in magnitude becomes 0"""

    @staticmethod
    def forward(ctx, x):
        return x

    @staticmethod
    def backward(ctx, g):
        return g.masked_fill((g.abs() > 0.01) | torch.isnan(g), 0.0)


class GradientClip(nn.Module):
    """parameter-free; the identity in forward"""

    def forward(self, x):
        return _ClipGrad.apply(x)


def _asks_gradient(module, tensors):
    return torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters()))


def _dense(t):
    """a contiguous non-empty [n, c, ht, wd] device tensor of a supported dtype"""
    return t.is_cuda and t.dtype in _DTYPES and t.dim() == 4 and t.is_contiguous() and t.numel() > 0 and t.numel() < 2 ** 31


def _head_fusable(module, conv, x):
    """x: what the head's 3x3 convolution `conv` would read"""
    if not _dense(x) or _asks_gradient(module, (x,)):
        return False
    want = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else conv.weight.dtype
    return want == x.dtype and conv.weight.is_cuda and conv.weight.device == x.device


def _params(conv, dtype):
    """the convolution's weight and bias as the kernel reads them: contiguous, in x's dtype.  Under autocast that is a cast
    of the float32 parameters; it is made once and kept on the convolution (the stand-in for autocast's own weight cache,
    which lives only inside one autocast region).  The kept copy is replaced when a parameter is replaced, moved or
    written in place (its _version changes: optimizer steps, load_state_dict, copy_ under no_grad).  A write through
    `p.data` changes neither: after one, call clear_cast_cache(module).  During a stream capture nothing is kept: a copy made
    there would live in the graph's private pool, so the cast is recorded into the graph (it then follows the parameters on
    every replay) unless an eager call has made the copy before."""
    w, b = conv.weight, conv.bias
    if w.dtype == dtype and w.is_contiguous():
        return w.detach(), (b.detach() if b is not None else None)
    key = (dtype, w.data_ptr(), w._version, None if b is None else (b.data_ptr(), b._version))
    kept = conv.__dict__.get("_dba_cast")
    if kept is None or kept[0] != key:
        kept = (key, w.detach().to(dtype).contiguous(), None if b is None else b.detach().to(dtype).contiguous())
        if not torch.cuda.is_current_stream_capturing():
            conv.__dict__["_dba_cast"] = kept
    return kept[1], kept[2]


def clear_cast_cache(module):
    """forget the half copies of parameters kept by the fused heads of `module` and its submodules (needed only after a
    parameter was written through `.data`)"""
    for m in module.modules():
        m.__dict__.pop("_dba_cast", None)


PLAN_MAX_EDGES = 8192    # per list, the limit of dbaf_amd.factors
plan_stats = dict(launches=0, host_reads=0)   # of frame_plan since import, as dbaf_amd.update_inputs.stats
_PLAN_MEMO = _lib.EdgeSetMemo()   # edge lists whose n_uniq is known: key (buffer,), value n_uniq
_MEMBERS_MEMO = _lib.EdgeSetMemo()   # edge lists whose member table is made: key (n_uniq,), value (seg_start, members)


def plan_max_rows():
    """the most buffer rows a frame plan covers (the kernel's presence flags)"""
    return int(_lib.load().dba_frame_plan_max_rows())


def frame_plan(ii, buffer):
    """`torch.unique(ii, return_inverse=True)` for an edge list over `buffer` video rows, in one launch (dba_frame_plan):
    -> (uniq [n_uniq] int64 ascending, inverse [n] int64), byte-equal to torch's.

    The FIRST call on an edge list reads the launch's result words once (one device-to-host copy) and raises ValueError if
    an entry lies outside [0, buffer).  LATER calls on the same tensor object at the same in-place version read nothing:
    the results are sized with the remembered n_uniq, which the launch checks against what it finds; on a mismatch (the
    list was written behind torch's version counter) it raises a pinned host word that makes the next call raise
    RuntimeError.  Such a call can be recorded into a hipGraph."""
    op = "frame_plan"
    _lib.edge_list(op, ii, "ii", None, PLAN_MAX_EDGES)
    _lib.require(int(buffer) == buffer and 0 < int(buffer) <= plan_max_rows(), op,
                 "buffer must be an integer in 1 .. %d, got %r" % (plan_max_rows(), buffer))
    buffer, n, dev = int(buffer), int(ii.shape[0]), ii.device
    lib = _lib.load()
    c = (ctypes.c_int * 6)()
    if lib.dba_frame_plan_poll(c):
        _PLAN_MEMO.clear()
        _MEMBERS_MEMO.clear()
        raise RuntimeError("frame_plan (MI355X): an earlier call found n_uniq = %d with %d entries out of range (first at %d) "
                           "on the device, its results were sized for n_uniq = %d: the edge list was written without torch "
                           "noticing" % (c[0], c[1], c[2], c[3]))
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    cap = min(n, buffer)
    expect = _PLAN_MEMO.lookup((ii,), (buffer,))
    with torch.cuda.device(dev):
        uniq = torch.empty(cap, dtype=torch.int64, device=dev)
        inverse = torch.empty(n, dtype=torch.int64, device=dev)
        res = torch.empty(4, dtype=torch.int32, device=dev)
        _lib.check(lib.dba_frame_plan(_lib.ptr(ii), n, buffer, cap, _lib.ptr(uniq), _lib.ptr(inverse), _lib.ptr(res),
                                      -1 if expect is None else expect, _lib.stream(dev)), "dba_frame_plan")
        plan_stats["launches"] += 1
        if expect is None:
            host = res.cpu().tolist()   # the one host synchronisation of a first call
            plan_stats["host_reads"] += 1
            _lib.require(host[1] == 0, op, "%d entries of ii lie outside [0, %d), the first at position %d" % (host[1], buffer, host[2]))
            expect = host[0]
            _PLAN_MEMO.remember((ii,), (buffer,), expect)
    return uniq[:expect], inverse


def frame_members(ii, inverse, dim_size):
    """conv.frame_members(inverse, dim_size) for the edge list `ii` whose plan gave `inverse`, kept with the list as
    frame_plan keeps its count: the same tensor object at the same in-place version finds its table again, launches nothing
    and reads nothing from the host.  Nothing is kept during a stream capture (the table would live in the graph's pool)
    unless an eager call has made it before; a report of the plan's guard forgets every table."""
    kept = _MEMBERS_MEMO.lookup((ii,), (int(dim_size),))
    if kept is None:
        kept = _conv.frame_members(inverse, dim_size)
        if not torch.cuda.is_current_stream_capturing():
            _MEMBERS_MEMO.remember((ii,), (int(dim_size),), kept)
    return kept


def _scatter_mean_plain(src, ix, dim_size):
    """scatter_mean(src [b, n, ...], ix [n], dim=1) in plain torch ops, on any device"""
    out = torch.zeros((src.shape[0], dim_size) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    out.index_add_(1, ix, src)
    count = torch.zeros(dim_size, dtype=src.dtype, device=src.device).index_add_(0, ix, torch.ones_like(ix, dtype=src.dtype))
    return out / count.clamp(min=1).view(1, -1, *([1] * (src.dim() - 2)))


class GraphAgg(nn.Module):
    """fuse_upmask (default False): hand out an UpmaskSource in place of `upmask` where the fused route's conditions hold
    (a contiguous float16 hidden state, nothing asking for a gradient), for dbaf_amd.upsample.upsample_disps_ to run the
    mask's convolution inside its own launch.  plan_rows: the video buffer's rows, the range of the frame plan.
    last_uniq: the frames of the last forward, ascending (what torch.unique(ii) gives), for the caller's statements."""
    fuse_upmask = False
    fuse_conv = False    # conv1 / conv2 with their ReLUs through dbaf_amd.conv.conv3x3 where its conditions hold
    fuse_agg = False     # conv1 / conv2 as under fuse_conv, eta under autocast in one launch, the mask convolution as conv1x1
                         # (module docstring); independent of the three other switches
    fuse_mean = False    # conv1, its ReLU and the frame mean in ONE launch (conv.conv3x3_frame_mean) where conv3x3's facts hold
                         # for conv1 and batch == 1; independent of the four other switches
    plan_rows = None     # None: the most the plan kernel covers
    last_uniq = None

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(128, 128, 3, padding=1)
        self.conv2 = nn.Conv2d(128, 128, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.eta = nn.Sequential(nn.Conv2d(128, 1, 3, padding=1), GradientClip(), nn.Softplus())
        self.upmask = nn.Sequential(nn.Conv2d(128, 8 * 8 * 9, 1, padding=0))

    def _plan(self, ii, plain):
        """(uniq, inverse) of the edge list: one launch of this project and, on a standing list, no host read; the
        statements (and a list the plan kernel does not take) keep torch.unique"""
        if (plain or not ii.is_cuda or ii.dtype != torch.int64 or ii.dim() != 1 or not ii.is_contiguous()
                or ii.shape[0] > PLAN_MAX_EDGES):
            return torch.unique(ii, return_inverse=True)
        return frame_plan(ii, plan_max_rows() if self.plan_rows is None else self.plan_rows)

    def _aggregate(self, net, ii, plain):
        batch, num, ch, ht, wd = net.shape
        net = net.view(batch * num, ch, ht, wd)
        uniq, ix = self._plan(ii, plain)
        self.last_uniq = uniq
        if self._mean_fusable(net, ix, uniq, batch, plain):
            net = _conv.conv3x3_frame_mean(net, _conv.pack_weights(self.conv1), ix, int(uniq.shape[0]),
                                           table=frame_members(ii, ix, int(uniq.shape[0])))
            return self._conv_relu(self.conv2, net, plain), batch, ht, wd
        net = self._conv_relu(self.conv1, net, plain)
        net = net.view(batch, num, 128, ht, wd)
        if plain:
            net = _scatter_mean_plain(net, ix, int(uniq.numel()))
        else:
            from torch_scatter import scatter_mean
            net = scatter_mean(net, ix, dim=1, dim_size=int(uniq.shape[0]))   # sized by the plan: no index.max() read
        net = net.view(-1, 128, ht, wd)
        return self._conv_relu(self.conv2, net, plain), batch, ht, wd

    def _mean_fusable(self, net, ix, uniq, batch, plain):
        """fuse_mean's facts: conv3x3's own for conv1 on net, one batch, a plan with at least one frame on net's device"""
        return (self.fuse_mean and not plain and batch == 1 and _conv.conv_fusable(self.conv1, net)
                and not _asks_gradient(self, (net,)) and ix.is_cuda and ix.device == net.device and ix.dtype == torch.int64
                and ix.dim() == 1 and ix.is_contiguous() and ix.shape[0] == net.shape[0]
                and 1 <= uniq.shape[0] <= _conv.frame_members_max_slots()
                and _conv.frame_mean_pays(uniq.shape[0], net.shape[2], net.shape[3],
                                          torch.cuda.get_device_properties(net.device).multi_processor_count))

    def _conv_relu(self, conv, x, plain):
        if (not plain and (self.fuse_conv or self.fuse_agg) and _conv.conv_fusable(conv, x)
                and not _asks_gradient(self, (x,))):
            return _conv.conv3x3(x, _conv.pack_weights(conv), relu=True)
        return self.relu(conv(x))

    def _mask(self, net, batch, ht, wd):
        """the mask's 1x1 convolution as a tensor: under fuse_agg one conv1x1 launch (576 = 9 * 64 outputs) where its facts
        hold, else the stock convolution"""
        if self.fuse_agg and _conv.pointwise_fusable(self.upmask[0], net) and not _asks_gradient(self, (net,)):
            return _conv.conv1x1(net, _conv.pack_pointwise(self.upmask[0])).view(batch, -1, 8 * 8 * 9, ht, wd)
        return self.upmask(net).view(batch, -1, 8 * 8 * 9, ht, wd)

    def forward_statements(self, net, ii):
        """the reference's chain in plain torch ops, on any device"""
        net, batch, ht, wd = self._aggregate(net, ii, True)
        eta = self.eta(net).view(batch, -1, ht, wd)
        upmask = self.upmask(net).view(batch, -1, 8 * 8 * 9, ht, wd)
        return .01 * eta, upmask

    def _upmask_fusable(self, net):
        """the fused launch is half only: anything else keeps the stock convolution and the two launches"""
        # maps whose planes are whole multiples of 4096 pixels keep the two launches: measured slower fused at 25 frames of
        # 64x64 (144 against 136 us, profiles/upsample_fused_bench.json), faster on the three other config shapes; the
        # supposed cause is the staging's channel stride of a power of two (8 KB), not examined further
        return (self.fuse_upmask and net.dtype == torch.float16 and _head_fusable(self, self.upmask[0], net)
                and net.shape[1] == 128 and (net.shape[2] * net.shape[3]) % 4096 != 0)

    def forward(self, net, ii):
        _require(isinstance(net, torch.Tensor) and net.is_cuda, "net must be a HIP device tensor; no CPU path")
        if _asks_gradient(self, (net,)):
            return self.forward_statements(net, ii)
        net, batch, ht, wd = self._aggregate(net, ii, False)
        # conv2's ReLU stays a torch launch (upmask's convolution reads it too), so eta reads it with relu_in off.
        # Under autocast torch's softplus answers in float32: then the statements run.
        # Under fuse_agg and a half state the kernel answers in float32 as they do (Head.out_dtype): v rounded once to half,
        # softplus and the factor in float32.
        if _head_fusable(self, self.eta[0], net) and not torch.is_autocast_enabled():
            w, b = _params(self.eta[0], net.dtype)
            eta = heads(Head(net, w, b, relu_in=False, act="softplus", scale=.01))[0].view(batch, -1, ht, wd)
        elif self.fuse_agg and net.dtype == torch.float16 and _head_fusable(self, self.eta[0], net):
            w, b = _params(self.eta[0], net.dtype)
            eta = heads(Head(net, w, b, relu_in=False, act="softplus", scale=.01, out_dtype=torch.float32))[0].view(batch, -1, ht, wd)
        else:
            eta = .01 * self.eta(net).view(batch, -1, ht, wd)
        if self._upmask_fusable(net):
            w, b = _params(self.upmask[0], net.dtype)
            return eta, UpmaskSource(net, w, b, uniq=self.last_uniq, batch=batch, matrix_cores=self.fuse_agg)
        return eta, self._mask(net, batch, ht, wd)


class UpdateModule(nn.Module):
    def __init__(self):
        super().__init__()
        cor_planes = 4 * (2 * 3 + 1) ** 2
        self.corr_encoder = nn.Sequential(nn.Conv2d(cor_planes, 128, 1, padding=0), nn.ReLU(inplace=True),
                                          nn.Conv2d(128, 128, 3, padding=1), nn.ReLU(inplace=True))
        self.flow_encoder = nn.Sequential(nn.Conv2d(4, 128, 7, padding=3), nn.ReLU(inplace=True),
                                          nn.Conv2d(128, 64, 3, padding=1), nn.ReLU(inplace=True))
        self.weight = nn.Sequential(nn.Conv2d(128, 128, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(128, 2, 3, padding=1),
                                    GradientClip(), nn.Sigmoid())
        self.delta = nn.Sequential(nn.Conv2d(128, 128, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(128, 2, 3, padding=1),
                                   GradientClip())
        self.gru = ConvGRU(128, 128 + 128 + 64)
        self.agg = GraphAgg()

    # the fused mask route and the frame plan are GraphAgg's: these are its switches under the operator's name
    @property
    def fuse_upmask(self):
        return self.agg.fuse_upmask

    @fuse_upmask.setter
    def fuse_upmask(self, on):
        self.agg.fuse_upmask = bool(on)

    # GraphAgg's own switch under the operator's name: the aggregation, eta under autocast and the mask on this project's kernels
    @property
    def fuse_agg(self):
        return self.agg.fuse_agg

    @fuse_agg.setter
    def fuse_agg(self, on):
        self.agg.fuse_agg = bool(on)

    # GraphAgg's switch under the operator's name: conv1, its ReLU and the frame mean in one launch
    @property
    def fuse_mean(self):
        return self.agg.fuse_mean

    @fuse_mean.setter
    def fuse_mean(self, on):
        self.agg.fuse_mean = bool(on)

    # flow_encoder[0] with its ReLU as ONE dbaf_amd.conv.conv7x7 launch where stem_fusable holds; a switch of its own,
    # independent of fuse_conv
    fuse_flow_stem = False

    # the convolutions on the matrix cores (dbaf_amd.conv): the whole GRU, corr_encoder[0] / [2], flow_encoder[2], the
    # heads' delta[0] / weight[0] and the aggregation's conv1 / conv2; the 7x7 flow stem has its own switch, fuse_flow_stem
    @property
    def fuse_conv(self):
        return self.gru.fuse_conv

    @fuse_conv.setter
    def fuse_conv(self, on):
        self.gru.fuse_conv = bool(on)
        self.agg.fuse_conv = bool(on)

    def _conv3(self, conv, x, asks):
        """conv(x) without a ReLU: through conv3x3 under fuse_conv where its conditions hold"""
        if self.fuse_conv and not asks and _conv.conv_fusable(conv, x):
            return _conv.conv3x3(x, _conv.pack_weights(conv), relu=False)
        return conv(x)

    def _pair_route(self, net, asks):
        """delta[0] and weight[0] as one conv3x3_pair: both take conv3x3's route on net, agree in their channels and biases,
        and the heads launch behind them takes half tensors"""
        d0, w0 = self.delta[0], self.weight[0]
        return (self.fuse_conv and not asks and _conv.conv_fusable(d0, net) and _conv.conv_fusable(w0, net)
                and d0.out_channels == w0.out_channels and (d0.bias is None) == (w0.bias is None)
                and _head_fusable(self, self.delta[2], net) and _head_fusable(self, self.weight[2], net)
                and self.delta[2].in_channels == d0.out_channels and self.weight[2].in_channels == w0.out_channels)

    @property
    def last_uniq(self):
        """the frames of the last forward(upsample=True), ascending: torch.unique(ii) without the caller's own unique"""
        return self.agg.last_uniq

    @staticmethod
    def _flat(net, inp, corr, flow):
        batch, num, ch, ht, wd = net.shape
        if flow is None:
            flow = torch.zeros(batch, num, 4, ht, wd, device=net.device)
        shape = (batch * num, -1, ht, wd)
        return (net.view(shape), inp.view(shape), corr.view(shape), flow.view(shape)), (batch, num, -1, ht, wd)

    @staticmethod
    def _result(net, delta, weight, agg, ii, upsample):
        if ii is None:
            return net, delta, weight
        if upsample:
            eta, upmask = agg(net, ii.to(net.device))
            return net, delta, weight, eta, upmask
        return net, delta, weight, None, None

    def forward_statements(self, net, inp, corr, flow=None, ii=None, jj=None, upsample=False):
        """the reference's chain in plain torch ops, on any device"""
        (net, inp, corr, flow), dim = self._flat(net, inp, corr, flow)
        corr = self.corr_encoder(corr)
        flow = self.flow_encoder(flow)
        net = self.gru.forward_statements(net, inp, corr, flow)
        delta = self.delta(net).view(*dim)
        weight = self.weight(net).view(*dim)
        delta = delta.permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        weight = weight.permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        return self._result(net.view(*dim), delta, weight, self.agg.forward_statements, ii, upsample)

    def forward(self, net, inp, corr, flow=None, ii=None, jj=None, upsample=False):
        for t, nm in ((net, "net"), (inp, "inp"), (corr, "corr")) + (((flow, "flow"),) if flow is not None else ()):
            _require(isinstance(t, torch.Tensor) and t.is_cuda, "%s must be a HIP device tensor; no CPU path" % nm)
        (net, inp, corr, flow), dim = self._flat(net, inp, corr, flow)
        asks = _asks_gradient(self, (net, inp, corr, flow))

        # the encoders without their last ReLU; the GRU's pack applies it while it copies
        ce, fe = self.corr_encoder, self.flow_encoder
        if self.fuse_conv and not asks and _conv.pointwise_fusable(ce[0], corr):
            corr = _conv.conv1x1(corr, _conv.pack_pointwise(ce[0]), relu=True)
        else:
            corr = ce[1](ce[0](corr))
        corr = self._conv3(ce[2], corr, asks)
        if self.fuse_flow_stem and not asks and _conv.stem_fusable(fe[0], flow):
            flow = _conv.conv7x7(flow, _conv.pack_stem(fe[0]), relu=True)   # a float32 flow under autocast: rounded as it is read
        else:
            flow = fe[1](fe[0](flow))
        flow = self._conv3(fe[2], flow, asks)
        if (not asks and _dense(net) and corr.dtype == net.dtype and flow.dtype == net.dtype and inp.dtype == net.dtype
                and inp.is_contiguous()):
            net = self.gru.forward_relu(net, (inp, corr, flow), relu=(False, True, True))
        else:
            net = self.gru(net, inp, ce[3](corr), fe[3](flow))

        # the heads: the two first convolutions as torch (under fuse_conv: ONE conv3x3_pair launch with their ReLUs, the
        # reference's in-place ReLU of half(c)), everything behind them in one launch
        if self._pair_route(net, asks):
            hd, hw = _conv.conv3x3_pair(net, _conv.pack_weights((self.delta[0], self.weight[0])), relu=True)
            wd_, bd = _params(self.delta[2], hd.dtype)
            ww, bw = _params(self.weight[2], hw.dtype)
            delta, weight = heads(Head(hd, wd_, bd, relu_in=False, act="none"), Head(hw, ww, bw, relu_in=False, act="sigmoid"))
            delta, weight = delta.view(dim[0], dim[1], dim[3], dim[4], 2), weight.view(dim[0], dim[1], dim[3], dim[4], 2)
            return self._result(net.view(*dim), delta, weight, self.agg, ii, upsample)
        hd, hw = self.delta[0](net), self.weight[0](net)
        if (not asks and hd.dtype == hw.dtype and _head_fusable(self, self.delta[2], hd) and _head_fusable(self, self.weight[2], hw)
                and _dense(hw)):
            wd_, bd = _params(self.delta[2], hd.dtype)
            ww, bw = _params(self.weight[2], hw.dtype)
            delta, weight = heads(Head(hd, wd_, bd, relu_in=True, act="none"), Head(hw, ww, bw, relu_in=True, act="sigmoid"))
            delta, weight = delta.view(dim[0], dim[1], dim[3], dim[4], 2), weight.view(dim[0], dim[1], dim[3], dim[4], 2)
        else:
            d, w = self.delta, self.weight
            delta = d[3](d[2](d[1](hd))).view(*dim).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
            weight = w[4](w[3](w[2](w[1](hw)))).view(*dim).permute(0, 1, 3, 4, 2)[..., :2].contiguous()
        return self._result(net.view(*dim), delta, weight, self.agg, ii, upsample)
