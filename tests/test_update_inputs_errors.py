"""CPU: dbaf_amd.update_inputs has no CPU path -- host tensors raise before the library is even asked."""
import pytest
import torch

from dbaf_amd import update_inputs as ux


def test_cpu_tensors_raise():
    n, m, h, w, B = 4, 3, 6, 8, 8
    ii = torch.arange(n)
    args = [ii, ii.clone(), torch.arange(m), torch.arange(m), torch.zeros(1, n, h, w, 2), torch.zeros(1, n, h, w, 2),
            torch.zeros(1, m, h, w, 2), torch.zeros(1, m, h, w, 2), torch.zeros(B, h, w), torch.zeros(B, 7), torch.ones(B, h, w)]
    before = dict(ux.stats)
    with pytest.raises(ValueError, match="no CPU path"):
        ux.assemble(*args, 3, 0.3, 0.2, True)
    with pytest.raises(ValueError, match="no CPU path"):
        ux.edge_counts(args[0], args[1], args[2], args[3], args[9], 3)
    assert ux.stats == before
    assert set(ux.stats) == {"edge_launches", "payload_launches", "host_reads"}
