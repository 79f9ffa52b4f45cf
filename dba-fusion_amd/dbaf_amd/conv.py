"""3x3 convolutions of half tensors on the MI355X's matrix cores (csrc/conv3x3.hip), with the ConvGRU's gate arithmetic in
the epilogue.  Opt-in: ConvGRU.fuse_conv / UpdateModule.fuse_conv route through here, and UpdateModule.fuse_flow_stem for
the 7x7 flow stem; nothing else does.

  pack_weights(conv_or_convs)        the parameters of one nn.Conv2d(C_in, C_out, 3, padding=1), or of several with one C_in
                                     one behind the other along C_out, as the kernels read them: Packed(w [9, C_out, C_in]
                                     half, tap-major, and bias [C_out] half or None).  Kept on the (first) module and rebuilt
                                     when a parameter's data_ptr() or _version changes; never rebuilt per call
  conv3x3(x, weight, bias, relu=False, x1=None, x1_first=0, x1_channels=None, out=None)
                                     F.conv2d(cat([x, x1[:, x1_first:x1_first + x1_channels]], 1), weight, bias, padding=1),
                                     optionally with torch.relu behind it; the cat is never written.  weight: a Packed or
                                     the module's [C_out, C_in, 3, 3] (then packed on the spot, not kept)
  conv3x3_gates(x, packed, gz, gr, net, ...)       -> (z, r * net): convz, convr and reset in one launch
  conv3x3_blend(x, packed, gq, z, net, ..., out)   -> (1 - z) net + z tanh(convq(.) + gq): convq and blend in one launch
  conv3x3_pair(x, packed, relu=False)              -> (conv_a(x), conv_b(x)) for pack_weights((conv_a, conv_b)): one launch,
                                     two contiguous tensors (the heads' delta[0] / weight[0])
  conv3x3_frame_mean(x, packed, inverse, dim_size, out=None, table=None)
                                     scatter_mean(conv3x3(x, packed, relu=True), inverse, dim=0, dim_size=dim_size) in ONE launch
                                     (csrc/conv3x3_mean.hip): the bytes of those two calls, the [n, C_out, h, w] tensor between
                                     them never written.  table: frame_members(inverse, dim_size), made here when not given
  frame_mean_pays(frames, h, w, compute_units)      the switch's routing rule on frames x tiles (measured; see its docstring)
  frame_members(inverse, dim_size)   -> (seg_start [dim_size + 1], members [n]) int32: each slot's edges, ascending; one launch
  supported(c0, c1, c_out)           the kernels' channel constraints: c0 % 32 == 0, c1 % 32 == 0, c_out % 64 == 0

and the 1x1 convolutions as a GEMM on the same matrix instruction (csrc/conv1x1.hip); C_in any positive count, C_out % 64 == 0:

  pack_pointwise(conv_or_convs)      Pointwise(w [C_out, ceil32(C_in)] half with a zero tail, bias, c_in), cached as above
  conv1x1(x, weight, bias=None, relu=False, out=None)
                                     F.conv2d(x, weight, bias) for a 1x1 weight, optionally torch.relu behind it
  conv1x1_context(net, packed_w, packed_glo)       -> (glo, gz, gr, gq): w(net), the ConvGRU's context mean and the three
                                     *_glo 1x1s in two launches; w(net) is never written

and the 7x7 flow stem, a convolution of FOUR channels, on the same matrix instruction (csrc/conv7x7.hip); C_out % 64 == 0:

  pack_stem(conv)                    Stem(w [7, C_out, 32] half: entry [ky, o, 4 kx + i] = weight[o, i, ky, kx], the eighth
                                     slot of a kernel row zero; bias), cached as above
  conv7x7(x, weight, bias=None, relu=False, out=None)
                                     F.conv2d(x.half(), weight, bias, padding=3) for x [n, 4, h, w] of float16 OR float32,
                                     optionally torch.relu behind it: a float32 x is rounded to half as the kernel reads it
                                     (the bytes of autocast's cast, without its launch)

  conv_fusable / pointwise_fusable / stem_fusable      the routing facts of one nn.Conv2d on x

and the encoders' convolutions (csrc/conv_enc.hip), behind BasicEncoder.fuse_conv / ResidualBlock.fuse_conv; C_in % 32 == 0
and C_out % 32 == 0 for the 3x3s, C_out % 32 == 0 for the stem:

  pack_strided(conv)                 Packed for one nn.Conv2d(C_in, C_out, 3, stride=1 or 2, padding=1), cached as above
  pack_down(conv1, down_conv)        PackedDown(w [10, C_out, C_in]: conv1's nine taps, then the 1x1 stride-2 weight; bias,
                                     bias_down) for a stride-2 block's conv1 and downsample[0], cached on conv1
  pack_encoder_stem(conv)            EncStem(w [7, C_out, 32]: entry [ky, o, 4 kx + i] = weight[o, i, ky, kx], the slots of
                                     kx = 7 and of i = 3 zero; bias) for nn.Conv2d(3, C_out, 7, stride=2, padding=3), cached
  conv3x3s(x, packed, stride=1, relu=False, out=None)      F.conv2d(x, weight, bias, stride=stride, padding=1)
  conv3x3s_down(x, packed, relu=False) -> (y, d)           conv1(x) (through torch.relu when relu) and downsample[0](x), one
                                     launch; d never takes the ReLU
  conv7x7s2(x, packed, relu=False, out=None)               F.conv2d(x.half(), weight, bias, stride=2, padding=3) for x
                                     [n, 3, h, w] of float16 OR float32
  strided_fusable / down_fusable / encoder_stem_fusable    the routing facts, pure functions of metadata
The packs turn float32 parameters into half ONCE per parameter version: under autocast that replaces the per-call casts.

Numerics: a float32 sum in one fixed order, plus the bias in float32, rounded ONCE to half; the gate statements behind it
round as dbaf_amd.gru.reset_ / blend do.  MIOpen's half convolution rounds differently, so results differ from nn.Conv2d's
in last half bits: the yardstick is the float64 statement (tests/conv3x3_cases.py).

Arguments are checked on the host without synchronising; work is enqueued on torch.cuda.current_stream(), memory comes from
torch's allocator only, and every call can be captured into a hipGraph.  CPU tensors raise.
"""
import collections

import torch
import torch.nn as nn

from . import _lib

Packed = collections.namedtuple("Packed", "w bias")
Pointwise = collections.namedtuple("Pointwise", "w bias c_in")   # w [C_out, ceil32(C_in)], the columns from c_in on zero
Stem = collections.namedtuple("Stem", "w bias")                  # w [7, C_out, 32]: [ky, o, 4 kx + i], the slots of kx = 7 zero
PackedDown = collections.namedtuple("PackedDown", "w bias bias_down")   # w [10, C_out, C_in]: nine taps, then the 1x1 slice
EncStem = collections.namedtuple("EncStem", "w bias")            # w [7, C_out, 32]: the slots of kx = 7 and of i = 3 zero


_p = _lib.ptr


def _require(cond, msg):
    _lib.require(cond, "conv3x3", msg)


def supported(c0, c1, c_out):
    return c0 > 0 and c0 % 32 == 0 and c1 >= 0 and c1 % 32 == 0 and c_out > 0 and c_out % 64 == 0


def tile():
    """the side of a workgroup's square pixel tile"""
    return int(_lib.load().dba_conv3x3_tile())


def _pack(weights, biases):
    w = torch.cat([t.detach() for t in weights], 0) if len(weights) > 1 else weights[0].detach()
    w = w.permute(2, 3, 0, 1).reshape(9, w.shape[0], w.shape[1]).to(torch.float16).contiguous()
    if all(b is None for b in biases):
        return Packed(w, None)
    _require(all(b is not None for b in biases), "concatenated convolutions must all have a bias, or none")
    b = torch.cat([t.detach() for t in biases], 0) if len(biases) > 1 else biases[0].detach()
    return Packed(w, b.to(torch.float16).contiguous())


# what pack_weights (k = 3), pack_pointwise (k = 1) and pack_stem (k = 7) say when they refuse a module
_KINDS = {3: ("pack_weights", "only 3x3, stride 1, zero padding 1, one group"),
          1: ("pack_pointwise", "only 1x1, stride 1, no padding, one group"),
          7: ("pack_stem", "only 7x7, stride 1, zero padding 3, one group")}


def _cached(conv_or_convs, slot, k, build):
    """build(weights, biases) of one plain k x k nn.Conv2d or a tuple of them with one C_in.  The result lives on the first
    module under `slot`, one entry per group of modules this one leads, and is rebuilt when any parameter's data_ptr() or
    _version changed.  During a stream capture nothing is kept (the copy would live in the graph's pool) unless an eager
    call has packed before."""
    convs = (conv_or_convs,) if isinstance(conv_or_convs, nn.Module) else tuple(conv_or_convs)
    _require(len(convs) >= 1 and all(isinstance(m, nn.Conv2d) for m in convs), "%s takes nn.Conv2d modules" % _KINDS[k][0])
    for m in convs:
        _require(_plain(m, k), _KINDS[k][1])
        _require(m.weight.is_cuda, "parameters must be on a HIP device; no CPU path")
        _require(m.in_channels == convs[0].in_channels, "concatenated convolutions must share C_in")
    return _keep(convs, slot, build)


def _keep(convs, slot, build):
    """build(weights, biases) for the modules `convs`, kept on the first one under `slot` as _cached says"""
    ids = tuple(id(m) for m in convs)
    key = tuple((m.weight.data_ptr(), m.weight._version) + ((None, None) if m.bias is None else
                                                            (m.bias.data_ptr(), m.bias._version)) for m in convs)
    kept = convs[0].__dict__.get(slot, {}).get(ids)
    if kept is None or kept[0] != key:
        kept = (key, build([m.weight for m in convs], [m.bias for m in convs]))
        if not torch.cuda.is_current_stream_capturing():
            convs[0].__dict__.setdefault(slot, {})[ids] = kept
    return kept[1]


def pack_weights(conv_or_convs):
    """-> Packed for one nn.Conv2d or a tuple of them (then concatenated along C_out).  The packed copy lives on the first
    module and is rebuilt when any parameter's data_ptr() or _version changed (optimizer steps, load_state_dict, copy_); a
    write through `.data` changes neither: call clear_pack_cache(module) after one.  During a stream capture nothing is
    kept (the copy would live in the graph's pool) unless an eager call has packed before."""
    return _cached(conv_or_convs, "_dba_conv3x3", 3, _pack)


def clear_pack_cache(module):
    for m in module.modules():
        m.__dict__.pop("_dba_conv3x3", None)
        m.__dict__.pop("_dba_conv1x1", None)
        m.__dict__.pop("_dba_conv7x7", None)
        m.__dict__.pop("_dba_conv_enc", None)


def pointwise_tile():
    """the pixels of a workgroup's tile of the 1x1 kernels"""
    return int(_lib.load().dba_conv1x1_tile())


def _pack_pointwise(weights, biases):
    w = torch.cat([t.detach().flatten(1) for t in weights], 0)
    c_out, c_in = int(w.shape[0]), int(w.shape[1])
    wp = torch.zeros((c_out, (c_in + 31) // 32 * 32), dtype=torch.float16, device=w.device)
    wp[:, :c_in] = w
    if all(b is None for b in biases):
        return Pointwise(wp, None, c_in)
    _require(all(b is not None for b in biases), "concatenated convolutions must all have a bias, or none")
    return Pointwise(wp, torch.cat([t.detach() for t in biases], 0).to(torch.float16).contiguous(), c_in)


def pack_pointwise(conv_or_convs):
    """-> Pointwise for one nn.Conv2d(C_in, C_out, 1) or a tuple of them with one C_in (then one behind the other along
    C_out): w [C_out, ceil32(C_in)] half with a zero tail, bias [C_out] half or None, c_in.  Kept and rebuilt as
    pack_weights keeps its copies: on the first module, under the parameters' data_ptr() and _version; nothing is kept
    during a stream capture; clear_pack_cache forgets it."""
    return _cached(conv_or_convs, "_dba_conv1x1", 1, _pack_pointwise)


def _half4(t, nm, dev=None):
    _require(isinstance(t, torch.Tensor) and t.is_cuda, "%s must be a HIP device tensor; no CPU path" % nm)
    _require(dev is None or t.device == dev, "%s must be on %s, got %s" % (nm, dev, t.device))
    _require(t.dtype == torch.float16, "%s must be float16, got %s" % (nm, t.dtype))
    _require(t.dim() == 4 and t.numel() > 0 and t.is_contiguous(), "%s must be a non-empty contiguous [n, c, h, w], got %s"
             % (nm, tuple(t.shape)))


def _overlap(x, y):
    a, b = x.data_ptr(), y.data_ptr()
    return a < b + y.numel() * y.element_size() and b < a + x.numel() * x.element_size()


def _bias_ok(bias, nm, c_out, dev):
    _require(bias is None or (bias.is_cuda and bias.device == dev and bias.dtype == torch.float16 and bias.is_contiguous()
                              and tuple(bias.shape) == (c_out,)), "%s must be a contiguous half [%d] on %s" % (nm, c_out, dev))


def _inputs(x, weight, bias, x1, x1_first, x1_channels, c_out_of=None):
    """the checks every entry shares -> (Packed, n, h, w, c0, c1, c1_total, first, c_out)"""
    _half4(x, "x")
    n, c0, h, w = (int(s) for s in x.shape)
    c1 = c1_total = first = 0
    if x1 is not None:
        _half4(x1, "x1", x.device)
        _require(x1.shape[0] == n and tuple(x1.shape[2:]) == (h, w), "x1 must be [%d, c, %d, %d], got %s" % (n, h, w, tuple(x1.shape)))
        c1_total, first = int(x1.shape[1]), int(x1_first)
        c1 = c1_total - first if x1_channels is None else int(x1_channels)
        _require(first >= 0 and c1 > 0 and first + c1 <= c1_total,
                 "x1 channels %d .. %d lie outside its %d" % (first, first + c1, c1_total))
    if isinstance(weight, Packed):
        pk = weight if bias is None else Packed(weight.w, bias)
    else:
        _require(isinstance(weight, torch.Tensor) and weight.is_cuda and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3),
                 "weight must be a Packed or a device tensor [C_out, C_in, 3, 3]")
        pk = _pack([weight], [bias])
    _require(pk.w.is_cuda and pk.w.device == x.device and pk.w.dtype == torch.float16 and pk.w.is_contiguous()
             and pk.w.dim() == 3 and pk.w.shape[0] == 9, "packed weights must be a contiguous half [9, C_out, C_in] on %s" % x.device)
    c_out = int(pk.w.shape[1])
    _require(int(pk.w.shape[2]) == c0 + c1, "the weights read %d channels, the input has %d + %d" % (pk.w.shape[2], c0, c1))
    _require(pk.w.data_ptr() % 16 == 0, "packed weights must be 16-byte aligned")
    _bias_ok(pk.bias, "bias", c_out, x.device)
    _require(supported(c0, c1, c_out), "channels must satisfy c0 %% 32 == 0, c1 %% 32 == 0, C_out %% 64 == 0; got %d, %d, %d"
             % (c0, c1, c_out))
    _require(h * w * max(c0 + c1, c1_total, c_out) < 2 ** 31, "one image's planes must stay below 2^31 elements")
    return pk, n, h, w, c0, c1, c1_total, first, c_out


def _src_args(x, c0, x1, c1, c1_total, first):
    return (_p(x), c0, _p(x1), c1, c1_total, first)


def _out(out, shape, x, reads):
    """where a launch writes: a new half tensor `shape` on x's device, or the caller's `out`, which must be that and share no
    byte with what the launch reads: `reads`, (tensor or None, its name) each"""
    if out is None:
        return torch.empty(shape, dtype=torch.float16, device=x.device)
    _half4(out, "out", x.device)
    _require(tuple(out.shape) == shape, "out must be %s, got %s" % (shape, tuple(out.shape)))
    for t, tnm in reads:
        _require(t is None or not _overlap(out, t), "out overlaps %s" % tnm)
    return out


def conv3x3(x, weight, bias=None, relu=False, x1=None, x1_first=0, x1_channels=None, out=None):
    pk, n, h, w, c0, c1, c1_total, first, c_out = _inputs(x, weight, bias, x1, x1_first, x1_channels)
    out = _out(out, (n, c_out, h, w), x, ((x, "x"), (x1, "x1"), (pk.w, "the weights"), (pk.bias, "the bias")))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv3x3_f16(*_src_args(x, c0, x1, c1, c1_total, first), _p(pk.w), _p(pk.bias), c_out, n, h, w,
                                               int(bool(relu)), _p(out), _lib.stream(x.device)), "dba_conv3x3_f16")
    return out


def frame_members_max_slots():
    """the most slots a member table covers (the frame plan's most rows)"""
    return int(_lib.load().dba_frame_members_max_slots())


def frame_mean_pays(frames, h, w, compute_units):
    """GraphAgg.fuse_mean's routing rule on frames x tiles, a pure function: does ONE launch of frames x tiles x 2 long
    workgroups (each runs all its slot's members) beat conv3x3 + scatter_mean?  The device holds 2 workgroups of this kernel
    per compute unit.  Measured (profiles/conv_agg_mean_bench.json, 256 compute units, five states): the launch met DESIGN
    4.17's bar where its last round of workgroups filled 0.75 and 0.75, 0.75 of the device (384, 384 and 896 workgroups) and
    missed it at 0.47 and 0.56 (240 and 800).  So: a last round under three quarters full keeps the two launches.  Grids of
    at most an eighth of a round (the tests' windows) were not timed; there one launch replaces two that are both bound by
    their launch, and they take the one launch."""
    t = 16
    grid = int(frames) * ((int(h) + t - 1) // t) * ((int(w) + t - 1) // t) * 2
    room = 2 * int(compute_units)
    if grid <= room // 8:
        return True
    last = grid % room
    return last == 0 or 4 * last >= 3 * room


def frame_members(inverse, dim_size):
    """the member table of a frame plan: (seg_start [dim_size + 1], members [n]) int32 on inverse's device, with
    members[seg_start[s]:seg_start[s + 1]] the positions e of inverse == s in ascending order (a stable counting sort in one
    small launch, dba_frame_members; no host read).  Entries of inverse outside [0, dim_size) belong to no slot, as
    scatter_mean(dim_size=) ignores them; the tail of members behind seg_start[dim_size] is -1."""
    op = "frame_members"
    _lib.dev_tensor(op, inverse, "inverse", None, torch.int64)
    _lib.require(inverse.dim() == 1 and inverse.shape[0] >= 1, op, "inverse must be a non-empty 1-D list, got %s" % (tuple(inverse.shape),))
    lib = _lib.load()
    most = int(lib.dba_frame_members_max_slots())
    _lib.require(int(dim_size) == dim_size and 1 <= int(dim_size) <= most, op, "dim_size must be an integer in 1 .. %d, got %r" % (most, dim_size))
    n, F, dev = int(inverse.shape[0]), int(dim_size), inverse.device
    with torch.cuda.device(dev):
        seg_start = torch.empty(F + 1, dtype=torch.int32, device=dev)
        members = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(lib.dba_frame_members(_p(inverse), n, F, _p(seg_start), _p(members), _lib.stream(dev)), "dba_frame_members")
    return seg_start, members


def conv3x3_frame_mean(x, packed, inverse, dim_size, out=None, table=None):
    """scatter_mean(conv3x3(x, packed, relu=True), inverse, dim=0, dim_size=dim_size) in ONE launch, byte for byte: per slot
    the members' convolutions in ascending edge order, each rounded to half through the ReLU as conv3x3 stores it, added as
    floats from 0, divided by max(count, 1) and rounded once.  x [n, C_in, h, w] half, packed: pack_weights(conv), inverse
    [n] int64 (frame_plan's; entries outside [0, dim_size) belong to no slot), table: frame_members(inverse, dim_size) when the
    caller keeps it with its plan.  -> [dim_size, C_out, h, w] half, an empty slot zeros.

    The result is allocated here; a caller's `out` must be a contiguous half [rows >= dim_size, C_out, h, w] on x's device
    that shares no byte with an input, else ValueError before anything is launched (then out[:dim_size] is returned).  The
    library is told the rows `out` really has (out.shape[0]), never dim_size again: it refuses dim_size > rows itself."""
    op = "conv3x3_frame_mean"
    _require(isinstance(packed, Packed), "conv3x3_frame_mean takes pack_weights' result")
    pk, n, h, w, c_in, _, _, _, c_out = _inputs(x, packed, None, None, 0, None)
    _lib.dev_tensor(op, inverse, "inverse", x.device, torch.int64)
    _lib.require(inverse.dim() == 1 and inverse.shape[0] == n, op, "inverse must be [%d], got %s" % (n, tuple(inverse.shape)))
    _lib.require(int(dim_size) == dim_size and int(dim_size) >= 1, op, "dim_size must be a positive integer, got %r" % (dim_size,))
    F = int(dim_size)
    if out is not None:   # refused here, before the library is touched
        _lib.require(isinstance(out, torch.Tensor) and out.is_cuda and out.device == x.device, op, "out must be a HIP device tensor on %s" % x.device)
        _lib.require(out.dtype == torch.float16, op, "out must be float16, got %s" % out.dtype)
        _lib.require(out.dim() == 4 and tuple(out.shape[1:]) == (c_out, h, w), op, "out must be [rows, %d, %d, %d], got %s"
                     % (c_out, h, w, tuple(out.shape)))
        _lib.require(out.shape[0] >= F, op, "out holds %d rows, dim_size is %d" % (out.shape[0], F))
        _lib.require(out.is_contiguous(), op, "out must be contiguous")
        for t, tnm in ((x, "x"), (pk.w, "the weights"), (pk.bias, "the bias"), (inverse, "inverse")):
            _lib.require(t is None or not _overlap(out, t), op, "out overlaps %s" % tnm)
    lib = _lib.load()
    most = int(lib.dba_frame_members_max_slots())
    _lib.require(F <= most, op, "dim_size must be at most %d, got %d" % (most, F))
    if out is None:
        out = torch.empty((F, c_out, h, w), dtype=torch.float16, device=x.device)
    if table is None:
        table = frame_members(inverse, F)
    seg_start, members = table
    for t, nm, size in ((seg_start, "seg_start", F + 1), (members, "members", n)):
        _lib.dev_tensor(op, t, "table: " + nm, x.device, torch.int32)
        _lib.require(tuple(t.shape) == (size,), op, "table: %s must be [%d], got %s" % (nm, size, tuple(t.shape)))
        _lib.require(not _overlap(out, t), op, "out overlaps the table")
    with torch.cuda.device(x.device):
        _lib.check(lib.dba_conv3x3_mean_f16(_p(x), c_in, _p(pk.w), _p(pk.bias), c_out, n, h, w, _p(seg_start), _p(members), F,
                                            _p(out), int(out.shape[0]), _lib.stream(x.device)), "dba_conv3x3_mean_f16")
    return out if out.shape[0] == F else out[:F]


def _gate_term(g, nm, x, n, c):
    _require(isinstance(g, torch.Tensor) and g.is_cuda and g.device == x.device and g.dtype == torch.float16
             and g.is_contiguous() and g.numel() == n * c and g.dim() >= 2 and tuple(g.shape[:2]) == (n, c),
             "%s must be a contiguous half [%d, %d, 1, 1] on %s" % (nm, n, c, x.device))


def conv3x3_gates(x, packed, gz, gr, net, x1=None, x1_first=0, x1_channels=None):
    """packed: pack_weights((convz, convr)).  -> (z, rnet) = (sigmoid(convz(.) + gz), sigmoid(convr(.) + gr) * net), new
    tensors [n, c, h, w]"""
    pk, n, h, w, c0, c1, c1_total, first, c_out = _inputs(x, packed, None, x1, x1_first, x1_channels)
    c = c_out // 2
    _half4(net, "net", x.device)
    _require(tuple(net.shape) == (n, c, h, w), "net must be %s, got %s" % ((n, c, h, w), tuple(net.shape)))
    _gate_term(gz, "gz", x, n, c)
    _gate_term(gr, "gr", x, n, c)
    z, rnet = torch.empty_like(net), torch.empty_like(net)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv3x3_gates_f16(*_src_args(x, c0, x1, c1, c1_total, first), _p(pk.w), _p(pk.bias), _p(gz),
                                                     _p(gr), _p(net), c, n, h, w, _p(z), _p(rnet), _lib.stream(x.device)),
                   "dba_conv3x3_gates_f16")
    return z, rnet


def conv3x3_blend(x, packed, gq, z, net, x1=None, x1_first=0, x1_channels=None, out=None):
    """packed: pack_weights(convq).  -> (1 - z) * net + z * tanh(convq(.) + gq); out may be net (in place)"""
    pk, n, h, w, c0, c1, c1_total, first, c = _inputs(x, packed, None, x1, x1_first, x1_channels)
    for t, nm in ((net, "net"), (z, "z")):
        _half4(t, nm, x.device)
        _require(tuple(t.shape) == (n, c, h, w), "%s must be %s, got %s" % (nm, (n, c, h, w), tuple(t.shape)))
    _gate_term(gq, "gq", x, n, c)
    given = out is not None
    out = _out(out, (n, c, h, w), x, ((x, "x"), (x1, "x1"), (pk.w, "the weights"), (pk.bias, "the bias")))
    if given:
        _require(not _overlap(out, z) and not _overlap(out, gq), "out overlaps z or gq")
        _require(out.data_ptr() == net.data_ptr() or not _overlap(out, net), "out overlaps net without being net")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv3x3_blend_f16(*_src_args(x, c0, x1, c1, c1_total, first), _p(pk.w), _p(pk.bias), _p(gq),
                                                     _p(z), _p(net), c, n, h, w, _p(out), _lib.stream(x.device)),
                   "dba_conv3x3_blend_f16")
    return out


def conv3x3_pair(x, packed, relu=False):
    """packed: pack_weights((conv_a, conv_b)), two convolutions of C_in -> c.  -> (conv_a(x), conv_b(x)), new contiguous
    tensors [n, c, h, w], each through torch.relu when relu: the two halves of conv3x3(x, packed) in ONE launch"""
    _require(isinstance(packed, Packed), "conv3x3_pair takes pack_weights' result")
    pk, n, h, w, c0, c1, c1_total, first, c_out = _inputs(x, packed, None, None, 0, None)
    _require(c_out % 2 == 0, "the packed weights must hold two convolutions of one C_out")
    c = c_out // 2
    out0 = torch.empty((n, c, h, w), dtype=torch.float16, device=x.device)
    out1 = torch.empty_like(out0)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv3x3_pair_f16(*_src_args(x, c0, None, c1, c1_total, first), _p(pk.w), _p(pk.bias), c, n, h, w,
                                                    int(bool(relu)), _p(out0), _p(out1), _lib.stream(x.device)),
                   "dba_conv3x3_pair_f16")
    return out0, out1


def _pointwise(weight, bias, dev, what="weight"):
    """a Pointwise, or the module's [C_out, C_in, 1, 1] / [C_out, C_in] (then packed on the spot, not kept), checked"""
    if isinstance(weight, Pointwise):
        pk = weight if bias is None else Pointwise(weight.w, bias, weight.c_in)
    else:
        _require(isinstance(weight, torch.Tensor) and weight.is_cuda and weight.dim() in (2, 4) and weight.numel() > 0
                 and tuple(weight.shape[2:]) in ((), (1, 1)), "%s must be a Pointwise or a device tensor [C_out, C_in, 1, 1]" % what)
        pk = _pack_pointwise([weight], [bias])
    c_out = int(pk.w.shape[0]) if isinstance(pk.w, torch.Tensor) and pk.w.dim() == 2 else 0
    _require(c_out > 0 and pk.w.is_cuda and pk.w.device == dev and pk.w.dtype == torch.float16 and pk.w.is_contiguous()
             and 0 < pk.c_in <= pk.w.shape[1] == (pk.c_in + 31) // 32 * 32,
             "packed %s must be a contiguous half [C_out, ceil32(C_in)] on %s" % (what, dev))
    _require(pk.w.data_ptr() % 16 == 0, "packed %s must be 16-byte aligned" % what)
    _bias_ok(pk.bias, "the bias of %s" % what, c_out, dev)
    _require(c_out % 64 == 0, "C_out must be a multiple of 64, got %d" % c_out)
    return pk, c_out


def conv1x1(x, weight, bias=None, relu=False, out=None):
    """F.conv2d(x, weight, bias) for a 1x1 weight, optionally with torch.relu behind it.  x [n, C_in, h, w] half, C_in any
    positive count; weight: a Pointwise (pack_pointwise) or the module's [C_out, C_in, 1, 1]; C_out % 64 == 0"""
    _half4(x, "x")
    n, c_in, h, w = (int(s) for s in x.shape)
    pk, c_out = _pointwise(weight, bias, x.device)
    _require(pk.c_in == c_in, "the weights read %d channels, the input has %d" % (pk.c_in, c_in))
    _require(h * w * max(c_in, c_out) < 2 ** 31, "one image's planes must stay below 2^31 elements")
    out = _out(out, (n, c_out, h, w), x, ((x, "x"), (pk.w, "the weights"), (pk.bias, "the bias")))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv1x1_f16(_p(x), c_in, _p(pk.w), _p(pk.bias), c_out, n, h * w, int(bool(relu)), _p(out),
                                               _lib.stream(x.device)), "dba_conv1x1_f16")
    return out


def conv1x1_context(net, packed_w, packed_glo):
    """packed_w: pack_pointwise(gru.w); packed_glo: pack_pointwise((gru.convz_glo, gru.convr_glo, gru.convq_glo)).
    -> (glo, gz, gr, gq), each [n, c, 1, 1] half: glo = mean_hw(sigmoid(w(net)) * net) statement by statement, gX =
    convX_glo(glo); w(net) itself is never written.  Two launches."""
    _half4(net, "net")
    n, c, h, w = (int(s) for s in net.shape)
    pk, c_out = _pointwise(packed_w, None, net.device, "w")
    pg, cg = _pointwise(packed_glo, None, net.device, "the *_glo weights")
    _require(pk.c_in == c and c_out == c, "w must be a 1x1 convolution of %d -> %d channels, got %d -> %d" % (c, c, pk.c_in, c_out))
    _require(pg.c_in == c and cg == 3 * c and pg.w.shape[1] == c,
             "the *_glo weights must be three 1x1 convolutions of %d -> %d channels one behind the other" % (c, c))
    _require(c <= 1024, "at most 1024 channels, got %d" % c)
    _require(h * w * c < 2 ** 31, "one image's planes must stay below 2^31 elements")
    lib = _lib.load()
    nbytes = int(lib.dba_conv1x1_context_workspace_bytes(n, c, h * w))
    outs = [torch.empty((n, c, 1, 1), dtype=torch.float16, device=net.device) for _ in range(4)]
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=net.device)
    with torch.cuda.device(net.device):
        _lib.check(lib.dba_conv1x1_context_f16(_p(net), _p(pk.w), _p(pk.bias), _p(pg.w), _p(pg.bias), c, n, h * w, _p(ws), nbytes,
                                               *[_p(t) for t in outs], _lib.stream(net.device)), "dba_conv1x1_context_f16")
    return tuple(outs)


def stem_tile():
    """the side of a workgroup's square pixel tile of the 7x7 kernel"""
    return int(_lib.load().dba_conv7x7_tile())


def _pack_stem(weights, biases):
    _require(len(weights) == 1, "pack_stem takes one convolution")
    w, b = weights[0].detach(), biases[0]
    _require(w.dim() == 4 and tuple(w.shape[1:]) == (4, 7, 7), "the stem's weight must be [C_out, 4, 7, 7], got %s" % (tuple(w.shape),))
    wp = torch.zeros((7, int(w.shape[0]), 8, 4), dtype=torch.float16, device=w.device)
    wp[:, :, :7, :] = w.permute(2, 0, 3, 1)        # [ky, o, kx, i]
    return Stem(wp.view(7, int(w.shape[0]), 32), None if b is None else b.detach().to(torch.float16).contiguous())


def pack_stem(conv):
    """-> Stem for one nn.Conv2d(4, C_out, 7, padding=3): w [7, C_out, 32] half with entry [ky, o, 4 kx + i] = weight[o, i,
    ky, kx] and the four slots of kx = 7 zero, bias [C_out] half or None.  Kept and rebuilt as pack_weights keeps its
    copies: on the module, under the parameters' data_ptr() and _version; nothing is kept during a stream capture;
    clear_pack_cache forgets it."""
    return _cached(conv, "_dba_conv7x7", 7, _pack_stem)


_STEM_DTYPES = {torch.float16: _lib.DBA_F16, torch.float32: _lib.DBA_F32}


def conv7x7(x, weight, bias=None, relu=False, out=None):
    """F.conv2d(x.half(), weight, bias, padding=3) for a [C_out, 4, 7, 7] weight, optionally with torch.relu behind it.
    x [n, 4, h, w] contiguous, float16 or float32 (then rounded to half as it is read: no cast launch); weight: a Stem
    (pack_stem) or the module's [C_out, 4, 7, 7]; C_out % 64 == 0.  -> half [n, C_out, h, w]"""
    _require(isinstance(x, torch.Tensor) and x.is_cuda, "x must be a HIP device tensor; no CPU path")
    _require(x.dtype in _STEM_DTYPES, "x must be float16 or float32, got %s" % x.dtype)
    _require(x.dim() == 4 and x.numel() > 0 and x.is_contiguous() and x.shape[1] == 4,
             "x must be a non-empty contiguous [n, 4, h, w], got %s" % (tuple(x.shape),))
    n, _, h, w = (int(s) for s in x.shape)
    if isinstance(weight, Stem):
        pk = weight if bias is None else Stem(weight.w, bias)
    else:
        _require(isinstance(weight, torch.Tensor) and weight.is_cuda and weight.dim() == 4 and tuple(weight.shape[1:]) == (4, 7, 7),
                 "weight must be a Stem or a device tensor [C_out, 4, 7, 7]")
        pk = _pack_stem([weight], [bias])
    _require(isinstance(pk.w, torch.Tensor) and pk.w.is_cuda and pk.w.device == x.device and pk.w.dtype == torch.float16
             and pk.w.is_contiguous() and pk.w.dim() == 3 and pk.w.shape[0] == 7 and pk.w.shape[2] == 32,
             "packed weights must be a contiguous half [7, C_out, 32] on %s" % x.device)
    c_out = int(pk.w.shape[1])
    _require(pk.w.data_ptr() % 16 == 0, "packed weights must be 16-byte aligned")
    _bias_ok(pk.bias, "bias", c_out, x.device)
    _require(c_out > 0 and c_out % 64 == 0, "C_out must be a multiple of 64, got %d" % c_out)
    _require(h * w * c_out < 2 ** 31, "one image's planes must stay below 2^31 elements")
    out = _out(out, (n, c_out, h, w), x, ((x, "x"), (pk.w, "the weights"), (pk.bias, "the bias")))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv7x7_f16(_p(x), _STEM_DTYPES[x.dtype], _p(pk.w), _p(pk.bias), c_out, n, h, w,
                                               int(bool(relu)), _p(out), _lib.stream(x.device)), "dba_conv7x7_f16")
    return out


def _plain(conv, k):
    """a k x k convolution of stride 1 with zero padding k // 2, no dilation, one group"""
    return (conv.kernel_size == (k, k) and conv.stride == (1, 1) and conv.padding == (k // 2, k // 2) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros")


def _answers_half(conv, dev):
    """the convolution's parameters lie on dev and it would answer in half there"""
    want = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else conv.weight.dtype
    return want == torch.float16 and conv.weight.is_cuda and conv.weight.device == dev


def _half_map(x):
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and x.is_contiguous()
            and x.numel() > 0)


def conv_fusable(conv, x):
    """the fuse_conv route's facts for one nn.Conv2d on x: a contiguous half device tensor, a plain 3x3 / padding 1
    convolution that would answer in half, channels the kernels take"""
    return (_half_map(x) and _answers_half(conv, x.device) and _plain(conv, 3)
            and supported(conv.in_channels, 0, conv.out_channels) and x.shape[1] == conv.in_channels)


def pointwise_fusable(conv, x):
    """conv_fusable for a 1x1 convolution: any C_in, C_out a multiple of 64"""
    return (_half_map(x) and _answers_half(conv, x.device) and _plain(conv, 1) and conv.out_channels % 64 == 0
            and x.shape[1] == conv.in_channels and x.shape[2] * x.shape[3] * max(x.shape[1], conv.out_channels) < 2 ** 31)


def stem_fusable(conv, x):
    """conv_fusable for the 7x7 flow stem: four input channels, C_out a multiple of 64; x half, or float32 while autocast to
    half is on (the kernel rounds it as autocast's cast would)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.is_contiguous() and x.numel() > 0):
        return False
    if not (_plain(conv, 7) and _answers_half(conv, x.device) and conv.in_channels == 4 and conv.out_channels % 64 == 0
            and x.shape[1] == 4):
        return False
    casts = x.dtype == torch.float32 and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.float16
    return (x.dtype == torch.float16 or casts) and x.shape[2] * x.shape[3] * conv.out_channels < 2 ** 31


# ---- the encoders' convolutions (csrc/conv_enc.hip) ------------------------------------------------------------------------

def _geometry(conv, k, strides):
    """a k x k convolution with zero padding k // 2 and a stride in `strides`, no dilation, one group"""
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (k, k) and conv.stride[0] == conv.stride[1]
            and conv.stride[0] in strides and conv.padding == (k // 2, k // 2) and conv.dilation == (1, 1) and conv.groups == 1
            and conv.padding_mode == "zeros")


def _on_device(convs, what):
    for m in convs:
        _require(m.weight.is_cuda, "%s: parameters must be on a HIP device; no CPU path" % what)


def strided_tile(stride):
    """(rows, columns) of a workgroup's tile of OUTPUT pixels of conv3x3s at this stride"""
    lib = _lib.load()
    return int(lib.dba_conv3x3s_tile_rows(int(stride))), int(lib.dba_conv3x3s_tile_cols())


def encoder_stem_tile():
    """the side of a workgroup's square tile of output pixels of conv7x7s2"""
    return int(_lib.load().dba_conv7x7s2_tile())


def pack_strided(conv):
    """-> Packed for one nn.Conv2d(C_in, C_out, 3, stride=1 or 2, padding=1): pack_weights' layout and cache rules (on the
    module, rebuilt when a parameter's data_ptr() or _version moves, nothing kept during a stream capture)"""
    _require(_geometry(conv, 3, (1, 2)), "pack_strided: only 3x3, stride 1 or 2, zero padding 1, one group")
    _on_device((conv,), "pack_strided")
    return _keep((conv,), "_dba_conv_enc", _pack)


def _pack_down(weights, biases):
    w3, w1 = (t.detach() for t in weights)
    c_out, c_in = int(w3.shape[0]), int(w3.shape[1])
    w = torch.empty((10, c_out, c_in), dtype=torch.float16, device=w3.device)
    w[:9] = w3.permute(2, 3, 0, 1).reshape(9, c_out, c_in)
    w[9] = w1.reshape(c_out, c_in)
    b3, b1 = (None if b is None else b.detach().to(torch.float16).contiguous() for b in biases)
    return PackedDown(w, b3, b1)


def pack_down(conv1, down_conv):
    """-> PackedDown for a stride-2 block's conv1 = nn.Conv2d(C_in, C_out, 3, stride=2, padding=1) and its downsample[0] =
    nn.Conv2d(C_in, C_out, 1, stride=2): w [10, C_out, C_in], conv1's nine taps and the 1x1 weight behind them; the two
    biases apart.  Kept on conv1 under pack_weights' rules, over the parameters of both."""
    _require(_geometry(conv1, 3, (2,)) and _geometry(down_conv, 1, (2,)),
             "pack_down: a 3x3 stride-2 padding-1 convolution and a 1x1 stride-2 one, one group each")
    _require(conv1.in_channels == down_conv.in_channels and conv1.out_channels == down_conv.out_channels,
             "pack_down: the two convolutions must share C_in and C_out")
    _on_device((conv1, down_conv), "pack_down")
    return _keep((conv1, down_conv), "_dba_conv_enc", _pack_down)


def _pack_encoder_stem(weights, biases):
    w, b = weights[0].detach(), biases[0]
    wp = torch.zeros((7, int(w.shape[0]), 8, 4), dtype=torch.float16, device=w.device)
    wp[:, :, :7, :3] = w.permute(2, 0, 3, 1)       # [ky, o, kx, i]
    return EncStem(wp.view(7, int(w.shape[0]), 32), None if b is None else b.detach().to(torch.float16).contiguous())


def pack_encoder_stem(conv):
    """-> EncStem for one nn.Conv2d(3, C_out, 7, stride=2, padding=3): w [7, C_out, 32] half with entry [ky, o, 4 kx + i] =
    weight[o, i, ky, kx], the slots of kx = 7 and of i = 3 zero; bias [C_out] half or None.  Cached as pack_weights' copies."""
    _require(_geometry(conv, 7, (2,)) and conv.in_channels == 3, "pack_encoder_stem: only 7x7, stride 2, zero padding 3, 3 -> C_out")
    _on_device((conv,), "pack_encoder_stem")
    return _keep((conv,), "_dba_conv_enc", _pack_encoder_stem)


def _enc_weights(pk, kind, slices, x, c_in):
    """the packed weights of conv3x3s (9 slices) / conv3x3s_down (10), checked -> c_out"""
    _require(isinstance(pk, kind), "the weights must be a %s" % kind.__name__)
    w = pk.w
    _require(isinstance(w, torch.Tensor) and w.is_cuda and w.device == x.device and w.dtype == torch.float16 and w.is_contiguous()
             and w.dim() == 3 and w.shape[0] == slices, "packed weights must be a contiguous half [%d, C_out, C_in] on %s"
             % (slices, x.device))
    c_out = int(w.shape[1])
    _require(int(w.shape[2]) == c_in, "the weights read %d channels, the input has %d" % (w.shape[2], c_in))
    _require(w.data_ptr() % 16 == 0, "packed weights must be 16-byte aligned")
    _require(c_in % 32 == 0 and c_out > 0 and c_out % 32 == 0, "channels must satisfy C_in %% 32 == 0, C_out %% 32 == 0; got %d, %d"
             % (c_in, c_out))
    return c_out


def _half_out(extent, stride):
    return (extent - 1) // stride + 1


def conv3x3s(x, packed, stride=1, relu=False, out=None):
    """F.conv2d(x, weight, bias, stride=stride, padding=1) for packed = pack_strided(conv) (or any Packed), stride 1 or 2,
    optionally with torch.relu behind it.  x [n, C_in, h, w] half, C_in % 32 == 0, C_out % 32 == 0.
    -> half [n, C_out, (h - 1) // stride + 1, (w - 1) // stride + 1]"""
    _half4(x, "x")
    _require(stride in (1, 2), "stride must be 1 or 2, got %r" % (stride,))
    n, c_in, h, w = (int(s) for s in x.shape)
    c_out = _enc_weights(packed, Packed, 9, x, c_in)
    _bias_ok(packed.bias, "bias", c_out, x.device)
    _require(h * w * max(c_in, c_out) < 2 ** 31, "one image's planes must stay below 2^31 elements")
    out = _out(out, (n, c_out, _half_out(h, stride), _half_out(w, stride)), x,
               ((x, "x"), (packed.w, "the weights"), (packed.bias, "the bias")))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv3x3s_f16(_p(x), _p(packed.w), _p(packed.bias), c_in, c_out, n, h, w, int(stride),
                                                int(bool(relu)), _p(out), _lib.stream(x.device)), "dba_conv3x3s_f16")
    return out


def conv3x3s_down(x, packed, relu=False):
    """packed: pack_down(conv1, downsample[0]) of a stride-2 block.  -> (y, d): y = conv1(x), through torch.relu when relu,
    the bytes of conv3x3s(x, ., stride=2, relu); d = downsample[0](x), never through the ReLU.  One launch, x read once; new
    contiguous tensors [n, C_out, (h - 1) // 2 + 1, (w - 1) // 2 + 1]"""
    _half4(x, "x")
    n, c_in, h, w = (int(s) for s in x.shape)
    c_out = _enc_weights(packed, PackedDown, 10, x, c_in)
    _bias_ok(packed.bias, "bias", c_out, x.device)
    _bias_ok(packed.bias_down, "bias_down", c_out, x.device)
    _require(h * w * max(c_in, c_out) < 2 ** 31, "one image's planes must stay below 2^31 elements")
    y = torch.empty((n, c_out, _half_out(h, 2), _half_out(w, 2)), dtype=torch.float16, device=x.device)
    d = torch.empty_like(y)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv3x3s_down_f16(_p(x), _p(packed.w), _p(packed.bias), _p(packed.bias_down), c_in, c_out, n,
                                                     h, w, int(bool(relu)), _p(y), _p(d), _lib.stream(x.device)),
                   "dba_conv3x3s_down_f16")
    return y, d


def conv7x7s2(x, packed, relu=False, out=None):
    """F.conv2d(x.half(), weight, bias, stride=2, padding=3) for packed = pack_encoder_stem(conv) (or any EncStem),
    optionally with torch.relu behind it.  x [n, 3, h, w] contiguous, float16 or float32 (then rounded to half as it is
    read: no cast launch); C_out % 32 == 0.  -> half [n, C_out, (h - 1) // 2 + 1, (w - 1) // 2 + 1]"""
    _require(isinstance(x, torch.Tensor) and x.is_cuda, "x must be a HIP device tensor; no CPU path")
    _require(x.dtype in _STEM_DTYPES, "x must be float16 or float32, got %s" % x.dtype)
    _require(x.dim() == 4 and x.numel() > 0 and x.is_contiguous() and x.shape[1] == 3,
             "x must be a non-empty contiguous [n, 3, h, w], got %s" % (tuple(x.shape),))
    n, _, h, w = (int(s) for s in x.shape)
    _require(isinstance(packed, EncStem), "the weights must be an EncStem")
    pw = packed.w
    _require(isinstance(pw, torch.Tensor) and pw.is_cuda and pw.device == x.device and pw.dtype == torch.float16
             and pw.is_contiguous() and pw.dim() == 3 and pw.shape[0] == 7 and pw.shape[2] == 32,
             "packed weights must be a contiguous half [7, C_out, 32] on %s" % x.device)
    c_out = int(pw.shape[1])
    _require(pw.data_ptr() % 16 == 0, "packed weights must be 16-byte aligned")
    _bias_ok(packed.bias, "bias", c_out, x.device)
    _require(c_out > 0 and c_out % 32 == 0, "C_out must be a multiple of 32, got %d" % c_out)
    _require(h * w * max(c_out, 3) < 2 ** 31, "one image's planes must stay below 2^31 elements")
    out = _out(out, (n, c_out, _half_out(h, 2), _half_out(w, 2)), x, ((x, "x"), (pw, "the weights"), (packed.bias, "the bias")))
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dba_conv7x7s2_f16(_p(x), _STEM_DTYPES[x.dtype], _p(pw), _p(packed.bias), c_out, n, h, w,
                                                 int(bool(relu)), _p(out), _lib.stream(x.device)), "dba_conv7x7s2_f16")
    return out


def strided_fusable(conv, x):
    """the encoders' fuse_conv facts for one 3x3 nn.Conv2d on x: a contiguous half device tensor, stride 1 or 2 with zero
    padding 1, a convolution that would answer in half, C_in % 32 == 0 and C_out % 32 == 0"""
    return (_half_map(x) and _geometry(conv, 3, (1, 2)) and _answers_half(conv, x.device) and conv.in_channels % 32 == 0
            and conv.out_channels % 32 == 0 and x.shape[1] == conv.in_channels
            and x.shape[2] * x.shape[3] * max(conv.in_channels, conv.out_channels) < 2 ** 31)


def down_fusable(conv1, down, x):
    """strided_fusable for a stride-2 block's conv1 together with its downsample[0], a 1x1 stride-2 convolution of the same
    channels that answers in half as well"""
    return (strided_fusable(conv1, x) and conv1.stride == (2, 2) and _geometry(down, 1, (2,)) and _answers_half(down, x.device)
            and down.in_channels == conv1.in_channels and down.out_channels == conv1.out_channels)


def encoder_stem_fusable(conv, x):
    """conv_fusable for the encoders' stem: 7x7, stride 2, zero padding 3, three input channels, C_out a multiple of 32; x
    half, or float32 while autocast to half is on (the kernel rounds it as autocast's cast would)"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.is_contiguous() and x.numel() > 0):
        return False
    if not (_geometry(conv, 7, (2,)) and _answers_half(conv, x.device) and conv.in_channels == 3 and conv.out_channels % 32 == 0
            and x.shape[1] == 3):
        return False
    casts = x.dtype == torch.float32 and torch.is_autocast_enabled() and torch.get_autocast_dtype("cuda") == torch.float16
    return (x.dtype == torch.float16 or casts) and x.shape[2] * x.shape[3] * max(conv.out_channels, 3) < 2 ** 31
