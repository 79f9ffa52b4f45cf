"""Generates tests/golden/update_op_surface.json and tests/golden/update_op_heads.npz by IMPORTING the reference's
UpdateModule on the CPU.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_update_op_golden.py <checkout of the reference project>
(the tests run without the reference tree, which is why the results are committed).  Data only, no reference source:

  update_op_surface.json   UpdateModule() and GraphAgg(): the state dict's keys with their shapes, and the parameter lists
                           of __init__ and forward (names and defaults)
  update_op_heads.npz      of the seeded module (its own default initialisation under torch.manual_seed, these entries then
                           rounded to values a half holds, as are the inputs: the file stays below 1 MiB) the entries
                           delta.*, weight.* and agg.eta.* in float32; net [3, 128, 5, 7] and [3, 128, 16, 17]; the reference
                           module's own CPU outputs of self.delta(net) and self.weight(net), permuted as its forward permutes
                           them, in float32 and, after .double(), in float64; and .01 * agg.eta(x) on a recorded x
                           [2, 128, 5, 7], likewise.  The other 10 MB of the module's weights are not stored.
"""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.dont_write_bytecode = True
N = 3
SHAPES = [(5, 7), (16, 17)]


def _params(fn):
    return [[n, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for n, p in inspect.signature(fn).parameters.items()]


def main(ref_root):
    # the reference's droid_net imports lietorch and torch_scatter: this project's boundary modules stand in for them
    for p in (os.path.join(ROOT, "dba-fusion_amd"), os.path.join(ref_root, "dbaf")):
        sys.path.insert(0, p)
    import droid_net as ref

    torch.manual_seed(20240923)
    m = ref.UpdateModule().eval()
    with torch.no_grad():       # values a half holds exactly: the stored float32 arrays compress to half their size
        for k, v in m.state_dict().items():
            if k.startswith(("delta.", "weight.", "agg.eta.")):
                v.copy_(v.half().float())
    surface = {}
    for name, cls, inst in (("UpdateModule", ref.UpdateModule, m), ("GraphAgg", ref.GraphAgg, m.agg)):
        surface[name] = {"state_dict": {k: list(v.shape) for k, v in inst.state_dict().items()},
                         "init_parameters": _params(cls.__init__), "forward_parameters": _params(cls.forward)}
    with open(os.path.join(HERE, "update_op_surface.json"), "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")

    out = {"w__" + k: v.detach().numpy().copy() for k, v in m.state_dict().items()
           if k.startswith(("delta.", "weight.", "agg.eta."))}
    m64 = ref.UpdateModule().double().eval()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    gen = torch.Generator().manual_seed(11)
    perm = lambda t: t.view(1, N, 2, *t.shape[2:]).permute(0, 1, 3, 4, 2)[..., :2].contiguous()[0].numpy()  # noqa: E731
    with torch.no_grad():
        for ht, wd in SHAPES:
            tag = "%dx%d" % (ht, wd)
            net = torch.tanh(torch.randn(N, 128, ht, wd, generator=gen)).half().float()
            out["net_" + tag] = net.numpy()
            for head in ("delta", "weight"):
                out["%s32_%s" % (head, tag)] = perm(getattr(m, head)(net.clone()))
                out["%s64_%s" % (head, tag)] = perm(getattr(m64, head)(net.double()))
        x = torch.relu(torch.randn(2, 128, 5, 7, generator=gen)).half().float()
        out["eta_x"] = x.numpy()
        out["eta32"] = (.01 * m.agg.eta(x)).view(2, 5, 7).numpy()
        out["eta64"] = (.01 * m64.agg.eta(x.double())).view(2, 5, 7).numpy()
    np.savez_compressed(os.path.join(HERE, "update_op_heads.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
