"""The update operator's ConvGRU on the MI355X: the reference's module (dbaf/modules/gru.py) with the body of its forward
between the convolutions in four HIP launches (csrc/gru.hip).

  pack(net, *inputs, relu=())            torch.cat([net, torch.cat(inputs, 1)], 1), written once          (gru.py:20-21);
                                         relu: torch.relu on the marked sources while they are copied
  context(a, net)                        (sigmoid(a) * net).view(b, c, h*w).mean(-1).view(b, c, 1, 1)     (gru.py:24-25)
  reset_(buf, cr, gr, net)               buf[:, :c] = sigmoid(cr + gr) * net, in place: buf becomes
                                         cat([r*net, inp], 1) without r*net or the cat ever existing      (gru.py:28-29)
  blend(cz, gz, cq, gq, net, out=None)   z = sigmoid(cz + gz); q = tanh(cq + gq); (1-z) * net + z * q     (gru.py:27-31)
  ConvGRU(h_planes=128, i_planes=128)    the reference's constructor, submodule names and forward(net, *inputs): a
                                         state dict of the reference loads unchanged; forward_relu(net, inputs, relu) is
                                         forward with the marked inputs still before their ReLU (dbaf_amd.update_op)

Every statement of the reference yields a tensor of the input dtype (half under autocast); the kernels round to that dtype
where a statement ends and compute in float32 in between, so a result differs from torch's statements only where a
float32 transcendental or the float32 sum of the context lands on the other side of a rounding boundary.  The seven
convolutions are the module's own nn.Conv2d calls (MIOpen), on the same contiguous inputs as the reference's.

ConvGRU.forward takes the fused route when net and all inputs are contiguous device tensors of one dtype (float16 or
float32), the convolutions answer in that dtype and nothing asks for a gradient (grad mode off, or neither an input nor a
parameter requires one); otherwise it runs forward_statements, the reference's chain in plain torch ops.  CPU tensors
raise.  Inputs are checked on the host without synchronising; work is enqueued on torch.cuda.current_stream(), memory
comes from torch's allocator only, and a forward can be captured into a hipGraph.

ConvGRU.fuse_conv (class attribute, default False: then nothing changes).  Set, and with half tensors whose channel counts
dbaf_amd.conv takes, the fused route's three gate convolutions leave MIOpen: convz + convr + reset_ become one launch and
convq + blend another (csrc/conv3x3.hip).  Where w and the three *_glo are plain 1x1s of c -> c channels answering in half,
w(net), the context and the *_glo 1x1s are the two launches of dbaf_amd.conv.conv1x1_context (csrc/conv1x1.hip; w(net) is
never written), and the forward calls no stock convolution: pack, context (two launches), GATES, BLEND.  It then returns the
same bytes on every call.  Results differ from the default route in last half bits (a float32 sum rounded once against
MIOpen's half convolution).
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from . import conv as _conv

MAX_SOURCES = 8
_DTYPES = {torch.float32: _lib.DBA_F32, torch.float16: _lib.DBA_F16}


_ptr, _overlap = _lib.ptr, _conv._overlap


def _require(cond, msg):
    _lib.require(cond, "gru", msg)


def _planes(x, nm):
    """x [n, c, *plane] -> (n, c, elements of a plane)"""
    _require(isinstance(x, torch.Tensor), "%s must be a tensor" % nm)
    _require(x.is_cuda, "%s must be a HIP device tensor; no CPU path" % nm)
    _require(x.dtype in _DTYPES, "%s must be float16 or float32, got %s" % (nm, x.dtype))
    _require(x.dim() >= 3, "%s must be [n, c, h, w] (or [n, c, hw]), got %s" % (nm, tuple(x.shape)))
    _require(x.is_contiguous(), "%s must be contiguous" % nm)
    _require(x.numel() > 0, "%s is empty: %s" % (nm, tuple(x.shape)))
    return int(x.shape[0]), int(x.shape[1]), x[0, 0].numel()


def _like(x, nm, ref, refnm):
    _planes(x, nm)
    _require(x.device == ref.device and x.dtype == ref.dtype,
             "%s must be on %s's device in its dtype (%s, %s), got (%s, %s)" % (nm, refnm, ref.device, ref.dtype, x.device, x.dtype))
    _require(x.shape == ref.shape, "%s must have %s's shape %s, got %s" % (nm, refnm, tuple(ref.shape), tuple(x.shape)))


def _gate(g, nm, ref, n, c):
    """a per-plane term, convX_glo(glo): [n, c, 1, 1] or any contiguous tensor of n * c elements"""
    _require(isinstance(g, torch.Tensor) and g.is_cuda and g.device == ref.device,
             "%s must be a HIP device tensor on %s; no CPU path" % (nm, ref.device))
    _require(g.dtype == ref.dtype, "%s must be %s, got %s" % (nm, ref.dtype, g.dtype))
    _require(g.is_contiguous() and g.numel() == n * c and g.dim() >= 2 and tuple(g.shape[:2]) == (n, c),
             "%s must be a contiguous [%d, %d, 1, 1], got %s" % (nm, n, c, tuple(g.shape)))


def _stream(x):
    return _lib.stream(x.device)


def pack(net, *inputs, relu=()):
    """net [n, c0, h, w] and up to 7 inputs [n, c_k, h, w] -> [n, c0 + sum c_k, h, w]: torch.cat([net, torch.cat(inputs, 1)], 1).
    relu: one flag per source (net first), or empty; a marked source goes through torch.relu while it is copied (the
    encoders' last ReLUs, dbaf/droid_net.py:83, :89).  Empty, or no flag set: the plain copy, dba_gru_pack."""
    srcs = (net,) + tuple(inputs)
    _require(len(srcs) <= MAX_SOURCES, "at most %d sources (net and %d inputs), got %d" % (MAX_SOURCES, MAX_SOURCES - 1, len(srcs)))
    relu = tuple(bool(f) for f in relu)
    _require(len(relu) in (0, len(srcs)), "relu must be empty or one flag per source (%d), got %d" % (len(srcs), len(relu)))
    n, _, hw = _planes(net, "net")
    for k, x in enumerate(inputs):
        _planes(x, "inputs[%d]" % k)
        _require(x.device == net.device and x.dtype == net.dtype,
                 "inputs[%d] must be on net's device in net's dtype (%s, %s), got (%s, %s)" % (k, net.device, net.dtype, x.device, x.dtype))
        _require(x.shape[0] == n and x.shape[2:] == net.shape[2:],
                 "inputs[%d] must be [%d, c, %s], got %s" % (k, n, ", ".join(str(s) for s in net.shape[2:]), tuple(x.shape)))
    chans = [int(x.shape[1]) for x in srcs]
    dst = torch.empty((n, sum(chans)) + tuple(net.shape[2:]), dtype=net.dtype, device=net.device)
    ptrs = (ctypes.c_void_p * len(srcs))(*[x.data_ptr() for x in srcs])
    cs = (ctypes.c_int * len(srcs))(*chans)
    mask = sum(1 << k for k, f in enumerate(relu) if f)
    with torch.cuda.device(net.device):
        if mask:
            _lib.check(_lib.load().dba_gru_pack_relu(ptrs, cs, len(srcs), n, hw, _DTYPES[net.dtype], _ptr(dst), mask, _stream(net)),
                       "dba_gru_pack_relu")
        else:
            _lib.check(_lib.load().dba_gru_pack(ptrs, cs, len(srcs), n, hw, _DTYPES[net.dtype], _ptr(dst), _stream(net)), "dba_gru_pack")
    return dst


def context(a, net, glo_weights=None):
    """a = w(net), net [n, c, h, w] -> glo [n, c, 1, 1] = mean over the plane of sigmoid(a) * net, statement by statement.
    The context step of the fuse_conv route: with glo_weights = pack_pointwise((convz_glo, convr_glo, convq_glo)), `a` is
    pack_pointwise(w) in place of w's result, and w(net), the mean and the three *_glo 1x1s are
    dbaf_amd.conv.conv1x1_context's two launches -> (glo, gz, gr, gq); w(net) is never written (half only)."""
    if glo_weights is not None:
        return _conv.conv1x1_context(net, a, glo_weights)
    n, c, hw = _planes(net, "net")
    _like(a, "a", net, "net")
    glo = torch.empty((n, c) + (1,) * (net.dim() - 2), dtype=net.dtype, device=net.device)
    with torch.cuda.device(net.device):
        _lib.check(_lib.load().dba_gru_context(_ptr(a), _ptr(net), n, c, hw, _DTYPES[net.dtype], _ptr(glo), _stream(net)),
                   "dba_gru_context")
    return glo


def reset_(buf, cr, gr, net):
    """buf [n, C, h, w] (pack's result), cr = convr(buf), gr = convr_glo(glo) [n, c, 1, 1], net [n, c, h, w]:
    buf[:, :c] = sigmoid(cr + gr) * net in place; channels c .. C-1 are left as they are.  Returns buf."""
    n, c, hw = _planes(net, "net")
    _like(cr, "cr", net, "net")
    _gate(gr, "gr", net, n, c)
    nb, cb, hwb = _planes(buf, "buf")
    _require(buf.device == net.device and buf.dtype == net.dtype, "buf must be on net's device in net's dtype")
    _require(nb == n and cb >= c and buf.shape[2:] == net.shape[2:],
             "buf must be [%d, >= %d, %s], got %s" % (n, c, ", ".join(str(s) for s in net.shape[2:]), tuple(buf.shape)))
    for x, nm in ((cr, "cr"), (gr, "gr"), (net, "net")):
        _require(not _overlap(buf, x), "buf overlaps %s" % nm)
    with torch.cuda.device(net.device):
        _lib.check(_lib.load().dba_gru_reset(_ptr(buf), cb, _ptr(cr), _ptr(gr), _ptr(net), n, c, hw, _DTYPES[net.dtype],
                                             _stream(net)), "dba_gru_reset")
    return buf


def blend(cz, gz, cq, gq, net, out=None):
    """cz = convz(net_inp), cq = convq(cat([r*net, inp])) [n, c, h, w], gz, gq [n, c, 1, 1], net [n, c, h, w] -> the new net.
    out: where to write it; net itself is allowed (in place), any other overlap with an input is not."""
    n, c, hw = _planes(net, "net")
    _like(cz, "cz", net, "net")
    _like(cq, "cq", net, "net")
    _gate(gz, "gz", net, n, c)
    _gate(gq, "gq", net, n, c)
    if out is None:
        out = torch.empty_like(net)
    else:
        _like(out, "out", net, "net")
        for x, nm in ((cz, "cz"), (gz, "gz"), (cq, "cq"), (gq, "gq")):
            _require(not _overlap(out, x), "out overlaps %s" % nm)
        _require(out.data_ptr() == net.data_ptr() or not _overlap(out, net), "out overlaps net without being net")
    with torch.cuda.device(net.device):
        _lib.check(_lib.load().dba_gru_blend(_ptr(cz), _ptr(gz), _ptr(cq), _ptr(gq), _ptr(net), n, c, hw, _DTYPES[net.dtype],
                                             _ptr(out), _stream(net)), "dba_gru_blend")
    return out


# the seven convolutions: (submodule name, reads the inputs' channels next to the hidden state's, kernel size).  Names and
# order are what a state dict of the reference's module carries.
_CONVS = (("convz", True, 3), ("convr", True, 3), ("convq", True, 3), ("w", False, 1),
          ("convz_glo", False, 1), ("convr_glo", False, 1), ("convq_glo", False, 1))


class ConvGRU(nn.Module):
    # fuse_conv (default False: then nothing changes): on the fused route with half tensors and channel counts the kernels of
    # dbaf_amd.conv take, convz + convr + reset_ become ONE launch and convq + blend another (csrc/conv3x3.hip); cz, cr, cq
    # and the in-place reset_ no longer exist.  Results differ from the MIOpen route in last half bits (dbaf_amd.conv).
    fuse_conv = False

    def __init__(self, h_planes=128, i_planes=128):
        super().__init__()
        for name, with_inputs, k in _CONVS:
            setattr(self, name, nn.Conv2d(h_planes + (i_planes if with_inputs else 0), h_planes, k, padding=k // 2))

    def _statements(self, net, inputs, a):
        """glo = mean_hw(sigma(a) net); z = sigma(convz(x) + convz_glo(glo)), r likewise; q = tanh(convq([r net, inputs]) +
        convq_glo(glo)); the new state (1 - z) net + z q -- one torch op per h(.) of include/dba_hip.h, a = w(net) given"""
        n, c = net.shape[:2]
        x = torch.cat((net,) + inputs, 1)
        glo = (torch.sigmoid(a) * net).flatten(2).mean(2).reshape(n, c, 1, 1)
        z = torch.sigmoid(self.convz(x) + self.convz_glo(glo))
        r = torch.sigmoid(self.convr(x) + self.convr_glo(glo))
        q = torch.tanh(self.convq(torch.cat((r * net,) + inputs, 1)) + self.convq_glo(glo))
        keep = (1 - z) * net
        return keep + z * q

    def forward_statements(self, net, *inputs):
        """the same update in plain torch ops, on any device: the route of everything the fused one does not take, and
        what the fused route is compared with"""
        return self._statements(net, tuple(inputs), self.w(net))

    def _fusable(self, net, inputs):
        xs = (net,) + tuple(inputs)
        if net.dtype not in _DTYPES or net.dim() != 4 or len(xs) > MAX_SOURCES or net.numel() == 0:
            return False
        if any(x.dtype != net.dtype or x.device != net.device or not x.is_contiguous() or x.dim() != 4 or x.numel() == 0
               or x.shape[0] != net.shape[0] or x.shape[2:] != net.shape[2:] for x in xs):
            return False
        if torch.is_grad_enabled() and (any(x.requires_grad for x in xs) or any(p.requires_grad for p in self.parameters())):
            return False
        return True

    def _gate_convs(self, c, ct, dev):
        """what both fuse_conv routes ask of convz, convr and convq -> the three, or None: channel counts the kernels take
        (c of the state, ct of the packed input) and plain 3x3s of ct channels answering in half on dev"""
        gates = (self.convz, self.convr, self.convq)
        ok = (_conv.supported(ct, 0, 2 * c) and _conv.supported(c, ct - c, c)
              and all(_conv._plain(m, 3) and _conv._answers_half(m, dev) and m.in_channels == ct for m in gates))
        return gates if ok else None

    def _conv_route(self, net, net_inp, gz):
        """the facts of the fuse_conv route beyond _fusable: half tensors, the three gate convolutions answering in half,
        channel counts the kernels take"""
        gates = self._gate_convs(net.shape[1], net_inp.shape[1], net_inp.device)
        return (net.dtype == torch.float16 and gz.dtype == torch.float16 and _conv._half_map(net_inp) and gates is not None
                and all(m.out_channels % 64 == 0 for m in gates))

    def _pointwise_route(self, net, inputs):
        """the facts of the route that calls no stock convolution, known before anything is enqueued: _conv_route's (on the
        channel counts pack will give), and w and the three *_glo plain 1x1s of c -> c channels answering in half"""
        c, ct, dev = net.shape[1], net.shape[1] + sum(int(x.shape[1]) for x in inputs), net.device
        gates = self._gate_convs(c, ct, dev)
        if net.dtype != torch.float16 or gates is None or any(m.out_channels != c for m in gates) or c > 1024:
            return False
        if ct * net.shape[2] * net.shape[3] >= 2 ** 31:   # one image's packed planes: the kernels' int offsets
            return False
        for m in (self.w, self.convz_glo, self.convr_glo, self.convq_glo):
            if not (_conv._plain(m, 1) and _conv._answers_half(m, dev) and m.in_channels == c and m.out_channels == c):
                return False
        biases = [m.bias is None for m in (self.convz_glo, self.convr_glo, self.convq_glo)]
        return all(biases) or not any(biases)

    def _gates_blend(self, net, net_inp, gz, gr, gq):
        """the tail of both fuse_conv routes: convz + convr + reset in one launch, convq + blend in another"""
        c = net.shape[1]
        z, rnet = _conv.conv3x3_gates(net_inp, _conv.pack_weights((self.convz, self.convr)), gz, gr, net)
        return _conv.conv3x3_blend(rnet, _conv.pack_weights(self.convq), gq, z, net, x1=net_inp, x1_first=c,
                                   x1_channels=net_inp.shape[1] - c)

    def forward(self, net, *inputs):
        return self._forward(net, tuple(inputs), ())

    def forward_relu(self, net, inputs, relu):
        """forward(net, *inputs) with the inputs marked in `relu` (one flag per input) still BEFORE their ReLU: the fused route
        applies it inside pack, the statement route as torch.relu.  An empty `relu` is forward."""
        inputs, relu = tuple(inputs), tuple(bool(f) for f in relu)
        _require(len(relu) in (0, len(inputs)), "relu must be empty or one flag per input (%d), got %d" % (len(inputs), len(relu)))
        return self._forward(net, inputs, relu)

    def _forward(self, net, inputs, relu):
        _require(len(inputs) >= 1, "forward needs net and at least one input")
        for k, x in enumerate((net,) + inputs):
            _require(isinstance(x, torch.Tensor) and x.is_cuda, "%s must be a HIP device tensor; no CPU path"
                     % ("net" if k == 0 else "inputs[%d]" % (k - 1)))
        if self.fuse_conv and self._fusable(net, inputs) and self._pointwise_route(net, inputs):
            # no stock convolution: w(net), the context and the three *_glo 1x1s are conv1x1_context's two launches
            net_inp = pack(net, *inputs, relu=((False,) + relu) if any(relu) else ())
            glo, gz, gr, gq = context(_conv.pack_pointwise(self.w), net,
                                      _conv.pack_pointwise((self.convz_glo, self.convr_glo, self.convq_glo)))
            return self._gates_blend(net, net_inp, gz, gr, gq)
        a = self.w(net)
        # autocast may answer in another dtype than the inputs': then the statements' own promotion rules apply
        if not self._fusable(net, inputs) or a.dtype != net.dtype:
            if any(relu):
                inputs = tuple(torch.relu(x) if f else x for x, f in zip(inputs, relu))
            return self._statements(net, inputs, a)

        net_inp = pack(net, *inputs, relu=((False,) + relu) if any(relu) else ())
        glo = context(a, net)

        gz, gr, gq = self.convz_glo(glo), self.convr_glo(glo), self.convq_glo(glo)
        if self.fuse_conv and self._conv_route(net, net_inp, gz):
            return self._gates_blend(net, net_inp, gz, gr, gq)
        cz = self.convz(net_inp)
        cr = self.convr(net_inp)
        reset_(net_inp, cr, gr, net)    # net_inp is cat([r*net, inp], 1) from here on; convz and convr are enqueued
        cq = self.convq(net_inp)
        return blend(cz, gz, cq, gq, net)
