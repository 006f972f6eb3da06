"""Host side of the device metrics (csrc/metrics.hip; no GPU): the binding table, the refusal of CPU tensors, the workspace
query, and the yardsticks the GPU tests compare the kernels with -- utils.metrics_utils.edit_distance against the oracle's, and
the CTC metric's composition (tests/ctc_metric_restated.py) against three hand-computed batches."""
import numpy as np
import pytest
import torch

from oracle import las_oracle as O
from phones_las_amd import hip
from phones_las_amd.utils import metrics_utils as mu
from tests import ctc_metric_restated as R

INF = float('inf')


def test_binding_table_holds_the_metric_entries():
    for name in ('las_edit_distance_batch', 'las_edit_distance_workspace_bytes', 'las_ctc_greedy_batch'):
        assert name in hip._SIGS and name in hip.EXPORTS
        assert hasattr(hip.lib(), name)
    assert hip.lib().las_version() == 105


def test_edit_distance_device_refuses_cpu_tensors():
    h = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(hip.LasError):
        mu.edit_distance_device(h, h, 2)
    with pytest.raises(hip.LasError):
        mu.edit_distance_on_device(h, h, 2)
    with pytest.raises(hip.LasError):
        hip.ctc_greedy_batch(torch.zeros(2, 5, 4), torch.zeros(2, dtype=torch.int32))


def test_workspace_queries_without_a_gpu():
    l = hip.lib()
    # tokens and the table row live in LDS up to a raw length of 1023; above it, three arrays of len_max + 1 ints per workgroup
    assert l.las_edit_distance_workspace_bytes(80, 64) == 0
    assert l.las_edit_distance_workspace_bytes(1023, 64) == 0
    assert l.las_edit_distance_workspace_bytes(1024, 64) == 64 * 3 * 1025 * 4
    assert l.las_edit_distance_workspace_bytes(8191, 100000) == 2048 * 3 * 8192 * 4      # bounded by the grid, not by the pairs
    assert l.las_edit_distance_workspace_bytes(0, 0) == 0
    assert l.las_attention_dtw_workspace_bytes(8, 16, 2) == 0                             # (the neighbour's, same convention)


def test_status_values_raise():
    hip.edit_distance_status([0, 3, 7])
    with pytest.raises(ValueError):
        hip.edit_distance_status([0, -1, 7])
    with pytest.raises(IndexError):
        hip.edit_distance_status([0, 3, -2])
    assert mu.normalised([0, 2, 1, 0], [0, 2, 1, 3], [0, 0, 4, 3]) == [0.0, INF, 0.25, 0.0]


def test_host_edit_distance_equals_the_oracles():
    rng = np.random.default_rng(5)
    mapping = [0, 1, 2, 3, 3, -1, 2]
    for _ in range(300):
        n, m = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        h = rng.choice([0, 1, 2, 3, 4, 5, 6, -1], n).tolist()
        t = rng.choice([0, 1, 2, 3, 4, 5, 6, -1], m).tolist()
        assert mu.edit_distance([h], [t], 2) == O.edit_distance([h], [t], 2)
        hm, tm = [v for v in h if v >= 0], [v for v in t if v >= 0]
        assert mu.edit_distance([hm], [tm], 2, mapping) == O.edit_distance([hm], [tm], 2, mapping)


C, EOS = 5, 2          # classes 0..3 and the blank 4


@pytest.mark.parametrize('classes, lens, targets, want, decoded', [
    # to_dense pads row 1 ([3]) with one 0: an extra <unk> token -> [3, 0] against [3]: one insertion
    ([[3, 3, 4, 1], [3, 1, 1, 1]], [4, 1], [[3, 1, 2], [3, 2, 2]], [0.0, 1.0], [[3, 1], [3, 0]]),
    # row 1 ends in id 0: the padding joins its run -> [3, 0, 0] is scored as [3, 0]
    ([[3, 1, 4, 3], [3, 0, 4, 4]], [4, 4], [[3, 1, 3, 2], [3, 0, 2, 2]], [0.0, 0.0], [[3, 1, 3], [3, 0, 0]]),
    # row 0 is the batch's longest: no padding, no extra token; the blank-only row 1 is all padding -> [0] against nothing
    ([[3, 4, 1, 1], [4, 4, 4, 4]], [4, 4], [[3, 1, 2], [2, 2, 2]], [0.0, INF], [[3, 1], [0, 0]]),
])
def test_ctc_metric_composition_by_hand(classes, lens, targets, want, decoded):
    logits = R.one_hot_logits(classes, C)
    assert R.dense_decode(logits, lens)[0] == decoded
    assert R.ctc_edit_distance(logits, lens, targets, EOS) == want
