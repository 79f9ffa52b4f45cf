"""Generates tests/golden/gru_surface.json and tests/golden/gru_forward.npz by IMPORTING the reference's ConvGRU.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gru_golden.py <checkout of the reference project>
(the tests run without the reference tree, which is why the results are committed).  Data only, no reference source:

  gru_surface.json   ConvGRU(128, 320): the state dict's keys with their shapes, and forward's parameter list (names only)
  gru_forward.npz    ConvGRU(16, 40) with seeded weights (its own default initialisation under torch.manual_seed, every
                     parameter stored), seeded inputs net [3,16,h,w] and three inputs of 16, 16 and 8 channels at 5 x 7 and
                     16 x 17, and the reference module's own CPU forward in float32 and, after .double(), in float64.
                     (16, 40) keeps the file at a few hundred KB; 3 x 16 x (35 + 272) = 14736 output entries.
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
H_PLANES, I_SPLIT, N = 16, (16, 16, 8), 3
SHAPES = [(5, 7), (16, 17)]


def main(ref_root):
    spec = importlib.util.spec_from_file_location("_ref_modules_gru", os.path.join(ref_root, "dbaf", "modules", "gru.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    big = ref.ConvGRU(128, 320)
    surface = {"state_dict": {k: list(v.shape) for k, v in big.state_dict().items()},
               "forward_parameters": [[n, p.kind.name] for n, p in inspect.signature(ref.ConvGRU.forward).parameters.items()],
               "init_parameters": [[n, None if p.default is inspect.Parameter.empty else p.default]
                                   for n, p in inspect.signature(ref.ConvGRU.__init__).parameters.items()]}
    with open(os.path.join(HERE, "gru_surface.json"), "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")

    torch.manual_seed(20240611)
    gru = ref.ConvGRU(H_PLANES, sum(I_SPLIT)).eval()
    out = {"w__" + k: v.detach().numpy().copy() for k, v in gru.state_dict().items()}
    gru64 = ref.ConvGRU(H_PLANES, sum(I_SPLIT)).double().eval()
    gru64.load_state_dict({k: v.double() for k, v in gru.state_dict().items()})
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for ht, wd in SHAPES:
            tag = "%dx%d" % (ht, wd)
            net = torch.tanh(torch.randn(N, H_PLANES, ht, wd, generator=gen))
            inputs = [0.5 * torch.randn(N, c, ht, wd, generator=gen) for c in I_SPLIT]
            out["net_" + tag] = net.numpy()
            for k, x in enumerate(inputs):
                out["inp%d_%s" % (k, tag)] = x.numpy()
            out["out32_" + tag] = gru(net, *inputs).numpy()
            out["out64_" + tag] = gru64(net.double(), *[x.double() for x in inputs]).numpy()
    np.savez_compressed(os.path.join(HERE, "gru_forward.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
