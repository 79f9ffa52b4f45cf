"""Numpy statement of the two pieces of CovisibleGraph.update() that ride in the lookup launch and in the BA-inputs launch
(dbaf/covisible_graph.py:221-222 and :235-236).  float32 throughout; a float16 operator output widens to float32 exactly.

  motion(coords1, target)            motn = cat([coords1 - coords0, target - coords1], -1).permute(0,1,4,2,3).clamp(-64, 64)
  op_outputs(coords1, delta, weight) target = coords1 + delta.float(), weight = weight.float()
  assemble_op(st, coords1, delta, weight, **par)   op_outputs, then the BA inputs of update_inputs_model.assemble
"""
import numpy as np

import update_inputs_model as um

F = np.float32


def coords_grid(ht, wd):
    """pops.coords_grid: [ht, wd, 2], (x, y) of every pixel"""
    y, x = np.meshgrid(np.arange(ht, dtype=F), np.arange(wd, dtype=F), indexing="ij")
    return np.stack([x, y], -1)


def clamp64(v):
    """torch.clamp(v, -64, 64): a compare-select, a NaN passes"""
    v = np.asarray(v, F)
    return np.where(v < F(-64.0), F(-64.0), np.where(v > F(64.0), F(64.0), v)).astype(F)


def motion(coords1, target):
    """coords1, target [1, n, ht, wd, 2] float32 -> motn [1, n, 4, ht, wd] float32: one subtraction, then the clamp"""
    coords1, target = np.asarray(coords1, F), np.asarray(target, F)
    ht, wd = coords1.shape[2:4]
    with np.errstate(invalid="ignore"):
        m = np.concatenate([coords1 - coords_grid(ht, wd), target - coords1], -1).astype(F)
    return np.ascontiguousarray(clamp64(m.transpose(0, 1, 4, 2, 3)))


def op_outputs(coords1, delta, weight):
    """:235-236.  delta, weight float16 or float32 -> (target, weight) float32, one rounding in the sum"""
    assert delta.dtype in (np.float16, np.float32) and weight.dtype == delta.dtype
    return (np.asarray(coords1, F) + delta.astype(F)).astype(F), weight.astype(F)


def assemble_op(st, coords1, delta, weight, **par):
    """st: a state of update_inputs_model (its target / weight are NOT read) -> (model dict of assemble, target, weight)"""
    target, w = op_outputs(coords1, delta, weight)
    return um.assemble(dict(st, target=target, weight=w), **par), target, w
