"""Generates tests/golden/extractor_surface.json, extractor_forward.npz and extractor_forward_cnet.npz by IMPORTING the
reference's encoders.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_extractor_golden.py <checkout of the reference project>
(the tests run without the reference tree, which is why the results are committed).  Data only, no reference source:

  extractor_surface.json       BasicEncoder(128, 'instance'), BasicEncoder(256, 'none') and ResidualBlock(32, 64, 'instance', 2):
                               the state dicts' keys with their shapes, and the constructors' parameter lists with defaults
  extractor_forward.npz        seeded weights, the two inputs, and the feature encoder's own CPU forward
  extractor_forward_cnet.npz   the context encoder's own CPU forward on the same inputs

An encoder has 0.7 M parameters, 2.8 MB in float32, and random mantissas do not compress: beyond what one committed file may
hold.  So the weights are the modules' own default initialisation under torch.manual_seed SNAPPED TO A GRID, w = code * 2^k
with int8 codes and one k per tensor (the grid step is about an eighth of the tensor's standard deviation), and they are
stored ONCE: the context encoder's trunk is the feature encoder's, only conv2 is its own.  The reference modules are loaded
with exactly these values before they run, so the recorded forwards belong to the stored weights bit for bit; codes are exact
in float16 as well.  The inputs are int8 codes / 32 (normal, sigma 1).  The float64 forward is stored as its float32 forward
plus the float32 of their difference: |out64 - (out32 + d)| < 2^-24 |out64 - out32|.
  w__<key>, k__<key>        fnet's state dict            wc__conv2.*, kc__conv2.*   cnet's own conv2
  x_<tag>                   the inputs, tag 40x56 ([1, 2, 3, 40, 56]) and 128x136 ([1, 1, 3, 128, 136])
  out32_<tag>, d64_<tag>    the forward in float32, and (float64 forward - float32 forward) as float32
"""
import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
INPUTS = {"40x56": (1, 2, 3, 40, 56), "128x136": (1, 1, 3, 128, 136)}


def _signature(fn):
    return [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(fn).parameters.items()]


def _snap(t):
    """-> (int8 codes, k) with t ~ codes * 2^k"""
    t = t.detach().double().numpy()
    sd = float(t.std()) if t.size > 1 and float(t.std()) > 0 else float(np.abs(t).max()) or 1.0
    k = int(np.round(np.log2(sd / 8.0)))
    return np.clip(np.round(t / 2.0 ** k), -127, 127).astype(np.int8), k


def main(ref_root):
    spec = importlib.util.spec_from_file_location("_ref_modules_extractor", os.path.join(ref_root, "dbaf", "modules", "extractor.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    torch.manual_seed(20240702)
    fnet = ref.BasicEncoder(128, "instance").eval()
    cnet = ref.BasicEncoder(256, "none").eval()
    block = ref.ResidualBlock(32, 64, "instance", 2)
    surface = {"fnet": {k: list(v.shape) for k, v in fnet.state_dict().items()},
               "cnet": {k: list(v.shape) for k, v in cnet.state_dict().items()},
               "fnet_multidim": {k: list(v.shape) for k, v in ref.BasicEncoder(128, "instance", multidim=True).state_dict().items()},
               "cnet_batch": {k: list(v.shape) for k, v in ref.BasicEncoder(256, "batch").state_dict().items()},
               "block": {k: list(v.shape) for k, v in block.state_dict().items()},
               "encoder_init_parameters": _signature(ref.BasicEncoder.__init__),
               "block_init_parameters": _signature(ref.ResidualBlock.__init__)}
    with open(os.path.join(HERE, "extractor_surface.json"), "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")

    out, out_c = {}, {}
    sd_f, sd_c = {}, {}
    for key, v in fnet.state_dict().items():
        codes, k = _snap(v)
        out["w__" + key], out["k__" + key] = codes, np.int32(k)
        sd_f[key] = torch.from_numpy(codes.astype(np.float32) * np.float32(2.0 ** k))
        sd_c[key] = sd_f[key]
    for key in ("conv2.weight", "conv2.bias"):
        codes, k = _snap(cnet.state_dict()[key])
        out["wc__" + key], out["kc__" + key] = codes, np.int32(k)
        sd_c[key] = torch.from_numpy(codes.astype(np.float32) * np.float32(2.0 ** k))
    fnet.load_state_dict(sd_f, strict=True)
    cnet.load_state_dict(sd_c, strict=True)
    fnet64 = ref.BasicEncoder(128, "instance").double().eval()
    cnet64 = ref.BasicEncoder(256, "none").double().eval()
    fnet64.load_state_dict({k: v.double() for k, v in sd_f.items()}, strict=True)
    cnet64.load_state_dict({k: v.double() for k, v in sd_c.items()}, strict=True)

    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for tag, shape in INPUTS.items():
            codes = torch.clamp(torch.round(32.0 * torch.randn(shape, generator=gen)), -127, 127)
            out["x_" + tag] = codes.numpy().astype(np.int8)
            x = codes / 32.0
            for net, net64, dst in ((fnet, fnet64, out), (cnet, cnet64, out_c)):
                o32 = net(x.clone()).numpy()
                o64 = net64(x.double()).numpy()
                dst["out32_" + tag] = o32
                dst["d64_" + tag] = (o64 - o32.astype(np.float64)).astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "extractor_forward.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "extractor_forward_cnet.npz"), **out_c)


if __name__ == "__main__":
    main(sys.argv[1])
