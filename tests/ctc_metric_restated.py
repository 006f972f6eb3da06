"""The yardstick of the CTC head's EVAL metric `ctc_edit_distance` (model_helper.py:347-367 of the reference), composed of
functions this project already trusts and never of the kernels: oracle.las_oracle.ctc_greedy_decode (tf.nn.ctc_greedy_decoder),
tf.sparse.to_dense's zero padding to the batch's longest decode, and utils.metrics_utils.edit_distance.  Shared by
tests/test_edit_distance_host.py, which pins it with hand-computed batches, and the GPU tests."""
import numpy as np

from oracle import las_oracle as O
from phones_las_amd.utils import metrics_utils as mu


def dense_decode(logits, logit_len):
    """(dense [B, D] int list rows, zero padded to the batch's longest decode D; the decoded lengths)."""
    seqs = O.ctc_greedy_decode(np.asarray(logits), np.asarray(logit_len))
    D = max([len(s) for s in seqs] + [0])
    return [list(s) + [0] * (D - len(s)) for s in seqs], [len(s) for s in seqs]


def ctc_edit_distance(logits, logit_len, targets, eos_id, mapping=None):
    dense, _ = dense_decode(logits, logit_len)
    return mu.edit_distance(dense, [list(map(int, t)) for t in targets], eos_id, mapping)


def one_hot_logits(classes, C):
    """fp32 logits [B, T, C] whose per-frame argmax is classes[b][t]."""
    cls = np.asarray(classes)
    x = np.zeros(cls.shape + (C,), np.float32)
    np.put_along_axis(x, cls[..., None], 1.0, -1)
    return x
