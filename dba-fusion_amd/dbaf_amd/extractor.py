"""The feature and context encoders on the MI355X: the reference's modules (dbaf/modules/extractor.py) with everything between
their convolutions in HIP launches (csrc/extractor.hip), and the two statements their caller wraps around them
(dbaf/motion_filter.py:64-65, :35-36).

  norm(x, relu=True, out=None, eps=1e-5, return_stats=False)   relu(InstanceNorm2d(x)), one launch; out may be x
  norm_skip(x, skip=None, down=None, out=None, eps=1e-5)        relu(skip + relu(norm(x))), skip as it is or norm(down):
                                                                the tail of a residual block, one launch
  relu_skip(x, skip, out=None)                                  relu(skip + relu(x)): the tail with norm_fn='none'
  normalize_image(image, dtype=torch.float32)                   image[:, [2,1,0]] / 255.0, .sub_(MEAN), .div_(STDV)
  context_split(x, c_net)                                       net, inp = x.split(..); net.tanh(), inp.relu()
  ResidualBlock, BasicEncoder                                   the reference's constructors and submodule names: a state
                                                                dict of the reference loads unchanged

Every statement of the reference yields a tensor of the input dtype (half under autocast); the kernels round to that dtype
where a statement ends and compute in float32 in between.  One workgroup holds one plane in registers, so a plane has at
most MAX_PLANE = 65536 elements; the modules send larger ones to the statements.  The convolutions are the modules' own
nn.Conv2d calls (MIOpen) unless fuse_conv is set.

BasicEncoder.fuse_conv / ResidualBlock.fuse_conv (class attributes, default off: then nothing changes; the encoder's setter
forwards to its blocks) send the convolutions of the fused route to dbaf_amd.conv, each piece on its own facts:
  stem               conv7x7s2, its ReLU in the epilogue for norm_fn 'none'; a float32 image under autocast is read as it is
  a block's conv1    stride 2: conv3x3s_down, conv1 and downsample[0] in one launch; stride 1: THE RULE below; the ReLU in
                     the epilogue for norm_fn 'none'
  a block's conv2    THE RULE, no ReLU (the tail kernel applies it)
  the encoder's conv2   conv1x1
THE RULE for a stride-1 3x3: conv.conv3x3 where conv.conv_fusable holds (C_out % 64 == 0: the 64 -> 64 and 128 -> 128
convolutions, its 128-channel workgroups), else conv.conv3x3s where conv.strided_fusable holds (32 -> 32).  It reads the
module and the tensor's metadata only, never n.  A piece whose condition fails makes its stock call where it always did.
With the flag, under autocast or as a half module, a forward calls no stock convolution, packs float32 parameters to half
once per parameter version (no per-call casts) and returns the same bytes on every call.

forward takes the fused route for norm_fn 'instance' and 'none' when the tensors are contiguous device tensors of float16
or float32, every convolution answers in the dtype the statement before it produced, and nothing asks for a gradient;
otherwise it runs forward_statements, the reference's chain in plain torch ops ('batch' and 'group' always do).  The
wrappers check their arguments on the host without synchronising and raise ValueError before anything is enqueued; CPU
tensors raise.  Work is enqueued on torch.cuda.current_stream(), memory comes from torch's allocator only, and a forward
can be captured into a hipGraph.
"""
import torch
import torch.nn as nn

from . import _lib
from . import conv as _conv

MAX_PLANE = 65536
_DTYPES = {torch.float32: _lib.DBA_F32, torch.float16: _lib.DBA_F16}
_IMAGE_DTYPES = {torch.uint8: _lib.DBA_U8, torch.float32: _lib.DBA_F32}


def _require(cond, msg):
    if not cond:
        raise ValueError("extractor (MI355X): " + msg)


def _ptr(x):
    return x.data_ptr() if x is not None else None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _call(name, ref, *args):
    """one entry point of the library on ref's device and its current stream (the stream is the last argument).  The encoders
    are bound by the host's time per launch, so the common case -- ref's device is the current one -- takes no context manager"""
    fn = getattr(_lib.load(), name)
    index = ref.device.index
    if index == torch.cuda.current_device():
        stream = _raw_stream(index) if _raw_stream is not None else torch.cuda.current_stream(ref.device).cuda_stream
        rc = fn(*args, stream)
    else:
        with torch.cuda.device(ref.device):
            rc = fn(*args, torch.cuda.current_stream(ref.device).cuda_stream)
    if rc:
        _lib.check(rc, name)


def _maps(x, nm, dtypes=_DTYPES):
    """x [n, c, h, w] -> (planes, elements of a plane)"""
    _require(isinstance(x, torch.Tensor), "%s must be a tensor" % nm)
    _require(x.is_cuda, "%s must be a HIP device tensor; no CPU path" % nm)
    _require(x.dtype in dtypes, "%s must be one of %s, got %s" % (nm, ", ".join(str(d) for d in dtypes), x.dtype))
    _require(x.dim() == 4, "%s must be [n, c, h, w], got %s" % (nm, tuple(x.shape)))
    _require(x.is_contiguous(), "%s must be contiguous" % nm)
    _require(x.numel() > 0, "%s is empty: %s" % (nm, tuple(x.shape)))
    return int(x.shape[0]) * int(x.shape[1]), int(x.shape[2]) * int(x.shape[3])


def _like(x, nm, ref, refnm):
    _maps(x, nm)
    _require(x.device == ref.device and x.dtype == ref.dtype,
             "%s must be on %s's device in its dtype (%s, %s), got (%s, %s)" % (nm, refnm, ref.device, ref.dtype, x.device, x.dtype))
    _require(x.shape == ref.shape, "%s must have %s's shape %s, got %s" % (nm, refnm, tuple(ref.shape), tuple(x.shape)))


def _overlap(x, y):
    a, b = x.data_ptr(), y.data_ptr()
    return a < b + y.numel() * y.element_size() and b < a + x.numel() * x.element_size()


def _out(out, x, others):
    """the destination: a new tensor, x itself, or a tensor that shares no byte with any operand"""
    if out is None:
        return torch.empty_like(x)
    _like(out, "out", x, "x")
    _require(out.data_ptr() == x.data_ptr() or not _overlap(out, x), "out overlaps x without being x")
    for t, nm in others:
        _require(not _overlap(out, t), "out overlaps %s" % nm)
    return out


def _cap(hw, nm):
    _require(hw <= MAX_PLANE, "a plane of %s has %d elements, more than a workgroup holds (%d)" % (nm, hw, MAX_PLANE))


def _eps(eps):
    eps = float(eps)
    _require(eps >= 0.0, "eps must be >= 0, got %r" % eps)
    return eps


def _norm_unchecked(x, relu, out, eps, stats=None):
    """dba_enc_norm on operands the caller has checked: what the modules below call"""
    n, c, h, w = x.shape
    _call("dba_enc_norm", x, x.data_ptr(), n * c, h * w, eps, int(relu), _DTYPES[x.dtype], out.data_ptr(), _ptr(stats))
    return out


def _norm_skip_unchecked(x, skip, down, out, eps, stats=None, stats_d=None):
    n, c, h, w = x.shape
    _call("dba_enc_norm_skip", x, x.data_ptr(), _ptr(skip), _ptr(down), n * c, h * w, eps, _DTYPES[x.dtype], out.data_ptr(),
          _ptr(stats), _ptr(stats_d))
    return out


def _relu_skip_unchecked(x, skip, out):
    _call("dba_enc_relu_skip", x, x.data_ptr(), skip.data_ptr(), x.numel(), _DTYPES[x.dtype], out.data_ptr())
    return out


def _new_stats(x):
    return torch.empty((x.shape[0], x.shape[1], 2), dtype=torch.float32, device=x.device)


def norm(x, relu=True, out=None, eps=1e-5, return_stats=False):
    """x [n, c, h, w] -> relu((x - mean) * rstd) per plane (the ReLU only with relu=True), biased variance, float32 statistics.
    out: where to write; x itself is allowed.  return_stats: also the [n, c, 2] float32 (mean, rstd) the kernel multiplied with."""
    _, hw = _maps(x, "x")
    _cap(hw, "x")
    eps = _eps(eps)
    out = _out(out, x, ())
    stats = _new_stats(x) if return_stats else None
    _norm_unchecked(x, bool(relu), out, eps, stats)
    return (out, stats) if return_stats else out


def norm_skip(x, skip=None, down=None, out=None, eps=1e-5, return_stats=False):
    """the tail of a residual block: relu(s + relu(norm(x))) with s = skip as it is, or norm(down) (the 1x1 downsample branch).
    Exactly one of skip / down.  out may be x.  return_stats: also (mean, rstd) of x's planes and, with down, of down's."""
    _, hw = _maps(x, "x")
    _cap(hw, "x")
    eps = _eps(eps)
    _require((skip is None) != (down is None), "exactly one of skip and down must be given")
    side, nm = (skip, "skip") if down is None else (down, "down")
    _like(side, nm, x, "x")
    _require(not _overlap(side, x), "%s overlaps x" % nm)
    out = _out(out, x, ((side, nm),))
    stats = _new_stats(x) if return_stats else None
    stats_d = _new_stats(x) if return_stats and down is not None else None
    _norm_skip_unchecked(x, skip, down, out, eps, stats, stats_d)
    return (out, stats, stats_d) if return_stats else out


def relu_skip(x, skip, out=None):
    """relu(skip + relu(x)), elementwise; out may be x"""
    _maps(x, "x")
    _like(skip, "skip", x, "x")
    _require(not _overlap(skip, x), "skip overlaps x")
    return _relu_skip_unchecked(x, skip, _out(out, x, ((skip, "skip"),)))


def normalize_image(image, dtype=torch.float32):
    """image [n, 3, h, w], uint8 or float32, BGR -> [n, 3, h, w] RGB of dtype: ((image[:, [2,1,0]] / 255.0) - MEAN) / STDV in
    float32, rounded once when dtype is float16"""
    _maps(image, "image", _IMAGE_DTYPES)
    _require(image.shape[1] == 3, "image must have 3 channels, got %s" % (tuple(image.shape),))
    _require(dtype in _DTYPES, "dtype must be float16 or float32, got %s" % (dtype,))
    n, _, h, w = (int(s) for s in image.shape)
    out = torch.empty((n, 3, h, w), dtype=dtype, device=image.device)
    _call("dba_enc_image", image, image.data_ptr(), n, h, w, _IMAGE_DTYPES[image.dtype], _DTYPES[dtype], out.data_ptr())
    return out


def context_split(x, c_net):
    """x [..., c, h, w] (the context encoder's output) -> (tanh(x[..., :c_net, :, :]), relu(x[..., c_net:, :, :])), both contiguous"""
    _require(isinstance(x, torch.Tensor), "x must be a tensor")
    _require(x.is_cuda, "x must be a HIP device tensor; no CPU path")
    _require(x.dtype in _DTYPES, "x must be float16 or float32, got %s" % x.dtype)
    _require(x.dim() >= 3, "x must be [..., c, h, w], got %s" % (tuple(x.shape),))
    _require(x.is_contiguous() and x.numel() > 0, "x must be contiguous and not empty")
    c = int(x.shape[-3])
    _require(isinstance(c_net, int) and 0 < c_net < c, "c_net must be in (0, %d), got %r" % (c, c_net))
    lead, hw = tuple(x.shape[:-3]), int(x.shape[-2]) * int(x.shape[-1])
    n = 1
    for s in lead:
        n *= int(s)
    net = torch.empty(lead + (c_net,) + tuple(x.shape[-2:]), dtype=x.dtype, device=x.device)
    inp = torch.empty(lead + (c - c_net,) + tuple(x.shape[-2:]), dtype=x.dtype, device=x.device)
    _call("dba_enc_context_split", x, x.data_ptr(), n, c_net, c - c_net, hw, _DTYPES[x.dtype], net.data_ptr(), inp.data_ptr())
    return net, inp


# ---- the modules ------------------------------------------------------------------------------------------------------------

_FUSED_NORMS = ("instance", "none")


def _make_norm(norm_fn, channels, groups):
    if norm_fn == "group":
        return nn.GroupNorm(num_groups=groups, num_channels=channels)
    if norm_fn == "batch":
        return nn.BatchNorm2d(channels)
    if norm_fn == "instance":
        return nn.InstanceNorm2d(channels)
    if norm_fn == "none":
        return nn.Sequential()
    raise ValueError("extractor (MI355X): unknown norm_fn %r" % (norm_fn,))


def _no_grad_asked(module, x):
    return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters())))


def _maps_ok(x):
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype in _DTYPES and x.is_contiguous()
            and x.numel() > 0 and x.shape[2] * x.shape[3] <= MAX_PLANE)


class ResidualBlock(nn.Module):
    def __init__(self, in_planes, planes, norm_fn='group', stride=1):
        super().__init__()
        self.norm_fn = norm_fn
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1 = _make_norm(norm_fn, planes, planes // 8)
        self.norm2 = _make_norm(norm_fn, planes, planes // 8)
        if stride == 1:
            self.downsample = None
        else:
            self.norm3 = _make_norm(norm_fn, planes, planes // 8)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)

    def forward_statements(self, x):
        """the reference's chain in plain torch ops, on any device"""
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)

    fuse_conv = False    # conv1 (with downsample[0] at stride 2) and conv2 through dbaf_amd.conv where its conditions hold

    def _routed(self, conv, x, relu):
        """conv(x) under fuse_conv by the module docstring's RULE (through the ReLU when relu), or None: not routed"""
        if _conv.conv_fusable(conv, x):
            return _conv.conv3x3(x, _conv.pack_weights(conv), relu=relu)
        if _conv.strided_fusable(conv, x):
            return _conv.conv3x3s(x, _conv.pack_strided(conv), stride=conv.stride[0], relu=relu)
        return None

    def _fused(self, x):
        """the fused chain, or None as soon as a tensor is not what the kernels take (nothing of the caller's is written)"""
        instance = self.norm_fn == "instance"
        y = d = None
        if self.fuse_conv:
            if self.downsample is not None and _conv.down_fusable(self.conv1, self.downsample[0], x):
                y, d = _conv.conv3x3s_down(x, _conv.pack_down(self.conv1, self.downsample[0]), relu=not instance)
            else:
                y = self._routed(self.conv1, x, not instance)
        if y is None:
            y = self.conv1(x)
            if not _maps_ok(y) or y.dtype != x.dtype:
                return None
            if not instance:
                y = y.relu_()
        if instance:
            y = _norm_unchecked(y, True, y, self.norm1.eps)
        z = self._routed(self.conv2, y, False) if self.fuse_conv else None
        y = self.conv2(y) if z is None else z
        if not _maps_ok(y) or y.dtype != x.dtype:
            return None
        # y is this call's own tensor: it shares no byte with x or d, and out = y is the allowed in-place form
        if self.downsample is None:
            if x.shape != y.shape:
                return None
            return _norm_skip_unchecked(y, x, None, y, self.norm2.eps) if instance else _relu_skip_unchecked(y, x, y)
        if d is None:
            d = self.downsample[0](x)
        if not _maps_ok(d) or d.dtype != y.dtype or d.shape != y.shape:
            return None
        return _norm_skip_unchecked(y, None, d, y, self.norm2.eps) if instance else _relu_skip_unchecked(y, d, y)

    def forward(self, x):
        if self.norm_fn in _FUSED_NORMS and isinstance(x, torch.Tensor) and x.is_cuda and _maps_ok(x) and _no_grad_asked(self, x):
            if self.norm_fn != "instance" or (self.norm2.eps == self.norm1.eps and not self.norm1.affine
                                              and not self.norm1.track_running_stats):
                out = self._fused(x)
                if out is not None:
                    return out
        return self.forward_statements(x)


DIM = 32
# the trunk every forward runs: (submodule name, planes, stride of its first block)
_TRUNK = (("layer1", DIM, 1), ("layer2", 2 * DIM, 2), ("layer3", 4 * DIM, 2))
# what multidim=True adds to the state dict (no forward reads them): (name, planes its first block reads, planes, stride)
_MULTIDIM_LAYERS = (("layer4", 4 * DIM, 256, 2), ("layer5", 256, 512, 2), ("layer6", 256, 256, 1), ("layer7", 128, 128, 1))
_MULTIDIM_CONVS = (("up1", 512, 256), ("up2", 256, 128))


def _two_blocks(in_planes, planes, norm_fn, stride):
    return nn.Sequential(ResidualBlock(in_planes, planes, norm_fn, stride=stride), ResidualBlock(planes, planes, norm_fn, stride=1))


def _initialise(module):
    """the initialisation a state dict overwrites: He-normal convolution weights (fan out), unit affine norms"""
    if isinstance(module, nn.Conv2d):
        nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="relu")
    elif isinstance(module, (nn.BatchNorm2d, nn.GroupNorm, nn.InstanceNorm2d)):
        for param, value in ((module.weight, 1.0), (module.bias, 0.0)):
            if param is not None:
                nn.init.constant_(param, value)


class BasicEncoder(nn.Module):
    def __init__(self, output_dim=128, norm_fn='batch', dropout=0.0, multidim=False):
        super().__init__()
        self.norm_fn, self.multidim = norm_fn, multidim
        self.norm1 = _make_norm(norm_fn, DIM, 8)
        self.conv1 = nn.Conv2d(3, DIM, kernel_size=7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        width = DIM
        for name, planes, stride in _TRUNK:
            setattr(self, name, _two_blocks(width, planes, norm_fn, stride))
            width = planes
        self.conv2 = nn.Conv2d(width, output_dim, kernel_size=1)
        if multidim:
            for name, reads, planes, stride in _MULTIDIM_LAYERS:
                setattr(self, name, _two_blocks(reads, planes, norm_fn, stride))
            for name, reads, planes in _MULTIDIM_CONVS:
                setattr(self, name, nn.Conv2d(reads, planes, 1))
            self.conv3 = nn.Conv2d(128, output_dim, kernel_size=1)
        self.in_planes = 128 if multidim else width
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        self.apply(_initialise)

    def _trunk(self):
        return [blk for name, _, _ in _TRUNK for blk in getattr(self, name)]

    def forward_statements(self, x):
        """the reference's chain in plain torch ops, on any device"""
        b, n, c1, h1, w1 = x.shape
        x = x.view(b * n, c1, h1, w1)
        x = self.relu1(self.norm1(self.conv1(x)))
        for blk in self._trunk():
            x = blk.forward_statements(x)
        x = self.conv2(x)
        _, c2, h2, w2 = x.shape
        return x.view(b, n, c2, h2, w2)

    def _fusable(self, x):
        if self.norm_fn not in _FUSED_NORMS or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 5:
            return False
        if x.dtype not in _DTYPES or not x.is_contiguous() or x.numel() == 0:
            return False
        if ((int(x.shape[3]) + 1) // 2) * ((int(x.shape[4]) + 1) // 2) > MAX_PLANE:     # the stem's plane, the largest
            return False
        if self.norm_fn == "instance" and (self.norm1.affine or self.norm1.track_running_stats):
            return False
        return _no_grad_asked(self, x)

    # the convolutions on the matrix cores (dbaf_amd.conv): the stem, the blocks' (forwarded to them) and conv2
    @property
    def fuse_conv(self):
        return self.__dict__.get("_fuse_conv", False)

    @fuse_conv.setter
    def fuse_conv(self, on):
        self.__dict__["_fuse_conv"] = bool(on)
        for m in self.modules():
            if isinstance(m, ResidualBlock):
                m.fuse_conv = bool(on)

    def forward(self, x):
        if not self._fusable(x):
            return self.forward_statements(x)
        b, n, c1, h1, w1 = x.shape
        fuse, none = self.fuse_conv, self.norm_fn != "instance"
        x4 = x.view(b * n, c1, h1, w1)
        if fuse and _conv.encoder_stem_fusable(self.conv1, x4):
            y = _conv.conv7x7s2(x4, _conv.pack_encoder_stem(self.conv1), relu=none)
            if not _maps_ok(y):
                return self.forward_statements(x)
            if not none:
                y = _norm_unchecked(y, True, y, self.norm1.eps)
        else:
            y = self.conv1(x4)
            if not _maps_ok(y):
                return self.forward_statements(x)
            y = _norm_unchecked(y, True, y, self.norm1.eps) if self.norm_fn == "instance" else y.relu_()
        for blk in self._trunk():
            y = blk(y)
        if fuse and _conv.pointwise_fusable(self.conv2, y):
            y = _conv.conv1x1(y, _conv.pack_pointwise(self.conv2))
        else:
            y = self.conv2(y)
        _, c2, h2, w2 = y.shape
        return y.view(b, n, c2, h2, w2)
