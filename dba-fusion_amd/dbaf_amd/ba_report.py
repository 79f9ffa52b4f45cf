"""How well each edge of a BA window is explained: the weighted reprojection cost the BA minimises, per edge, on the device
(droid_backends.ba_cost / BACore.cost -> dba_ba_cost, csrc/ba_cost.hip).

A report is a float64 tensor [N + 1, 4]: row n < N is edge n, row N the window's total; the columns are
    COST    sum over the edge's used pixels of w_u r_u^2 + w_v r_v^2   (w = 0.001 x weight, r = target - projection)
    WSUM    sum of w_u + w_v
    N_USED  number of used pixels (not cut by z < 0.25, w_u + w_v != 0), exact
    R2MAX   largest r_u^2 + r_v^2
An edge whose ii or jj is not a frame of the buffer reads (NaN, NaN, -1, NaN).  Nothing here reads the device from the host.
"""
import torch

COST, WSUM, N_USED, R2MAX = 0, 1, 2, 3


def edge_cost(poses, disps, intrinsics, targets, weights, ii, jj, out=None):
    """the report of a window (droid_backends.ba_cost): two launches on the current stream, no host synchronisation"""
    import droid_backends
    return droid_backends.ba_cost(poses, disps, intrinsics, targets, weights, ii, jj, out=out)


def rms_px(report):
    """weighted root-mean-square residual in pixels per row, sqrt(cost / wsum); 0 where wsum == 0"""
    cost, wsum = report[..., COST], report[..., WSUM]
    return torch.where(wsum == 0, torch.zeros_like(cost), (cost / torch.where(wsum == 0, torch.ones_like(wsum), wsum)).sqrt())


def worst_edges(report, k):
    """indices [min(k, N)] (int64, on the report's device) of the edges with the largest cost per used pixel,
    cost / max(n_used, 1), largest first; the total row does not take part.  A NaN row (a refused edge, a NaN residual) ranks
    above every number: it is what a caller has to look at first."""
    edges = report[:-1]
    per_pixel = edges[:, COST] / edges[:, N_USED].clamp_min(1.0)
    return torch.topk(per_pixel, min(int(k), int(edges.shape[0]))).indices
