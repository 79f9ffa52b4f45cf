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
