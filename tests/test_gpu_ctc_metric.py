"""las_ctc_greedy_batch against oracle.las_oracle.ctc_greedy_decode, the CTC head's EVAL metric `ctc_edit_distance` against its
composed yardstick (tests/ctc_metric_restated.py) on the model's own logits, and LAS_HOST_METRICS: the device and the host
scoring of evaluate / train_edit_distance return the same Python floats (==, inf included)."""
import numpy as np
import pytest
import torch

from oracle import las_oracle as O
from phones_las_amd import hip
from phones_las_amd import model_helper as mh
from tests import ctc_metric_restated as R
from tests.helpers import make_batch, make_hparams, to_device

pytestmark = pytest.mark.gpu


def test_ctc_greedy_batch_against_the_oracle():
    rng = np.random.default_rng(3)
    B, T, C, LD = 6, 70, 9, 16
    lens = [0, 1, 63, 64, 65, 70]
    x = np.full((B, T, LD), 1e9, np.float32)                    # columns >= C: would win every argmax if they were read
    x[..., :C] = rng.integers(0, 3, (B, T, C)).astype(np.float32)    # three levels: exact ties (first index wins) and repeats
    x[:, :, C - 1] += rng.integers(0, 2, (B, T)) * 2.0               # ... and a fair share of blanks
    x[2, :, :C] = 0.0
    x[2, :, C - 1] = 1.0                                             # a blank-only row (63 frames of it)
    for b, n in enumerate(lens):                                     # frames >= len: a changing non-blank class, never to be emitted
        x[b, n:, :C] = 0.0
        for t in range(n, T):
            x[b, t, t % (C - 1)] = 5.0
    want = O.ctc_greedy_decode(x[..., :C], lens)
    assert want[2] == [] and want[0] == [] and max(len(s) for s in want) > 10
    decoded, dec_len = hip.ctc_greedy_batch(torch.as_tensor(x).cuda(), torch.tensor(lens, dtype=torch.int32).cuda(), C)
    decoded, dec_len = decoded.cpu().tolist(), dec_len.cpu().tolist()
    assert dec_len == [len(s) for s in want]
    assert decoded == [s + [0] * (T - len(s)) for s in want]          # compacted to the front, zeros behind


def _model(ctc, mapping=None, seed=21):
    _, params = make_hparams(ctc=ctc)
    if mapping is not None:
        params.del_hparam('mapping')
        params.add_hparam('mapping', mapping)
    model = mh.LasModel(params, seed=seed)
    if model.ctc is not None:                     # a head whose argmax changes from frame to frame
        g = torch.Generator().manual_seed(seed)
        k = model.vars.params['ctc_logits/kernel']
        k.copy_(torch.randn(k.shape, generator=g) * 2.0)
        model.refresh_images()
    return model, params


MAPPING = [0, 1, 2, 3, 3, 5, 5, -1, 8, 9, 10]      # V = 11; 4 -> 3 and 6 -> 5 merge neighbours, 7 -> -1


def _batch(seed=0):
    feats, labels = to_device(make_batch(B=4, T=32, U=7, tgt_len=[7, 5, 3, 6], seed=seed))
    labels['targets_outputs'][2, :] = O.EOS_ID       # an empty target: inf against a non-empty hypothesis
    return feats, labels


@pytest.mark.parametrize('mapping', [None, MAPPING])
def test_evaluate_reports_the_ctc_heads_edit_distance(mapping):
    model, params = _model(0.3, mapping)
    feats, labels = _batch()
    loss, ed, pred = model.evaluate(feats, labels)
    mem, mem_len = pred['_memory']
    logits = model.ctc.logits_only(mem.contiguous())[..., :model.ctc.C].float().cpu().numpy()
    tout = labels['targets_outputs'].cpu().tolist()
    want = R.ctc_edit_distance(logits, mem_len.cpu().tolist(), tout, params.decoder.eos_id, mapping)
    assert pred['ctc_edit_distance'] == want
    dense, lens = R.dense_decode(logits, mem_len.cpu().tolist())
    assert pred['ctc_decoded'].cpu().tolist() == dense and pred['ctc_decoded_length'].cpu().tolist() == lens
    assert max(lens) > min(lens)                                      # rows of different lengths: the padding rule is at work
    spec = mh.las_model_fn(feats, labels, mh.EVAL, None, params, model=model)
    assert spec.eval_metric_ops['ctc_edit_distance'] == float(np.mean(want))
    assert spec.eval_metric_ops['edit_distance'] == float(np.mean(ed))


def test_a_model_without_the_head_has_no_such_key():
    model, params = _model(-1.0)
    feats, labels = _batch()
    _, _, pred = model.evaluate(feats, labels)
    assert 'ctc_edit_distance' not in pred and 'ctc_decoded' not in pred
    assert 'ctc_edit_distance' not in mh.las_model_fn(feats, labels, mh.EVAL, None, params, model=model).eval_metric_ops


@pytest.mark.parametrize('mapping', [None, MAPPING])
def test_host_and_device_metrics_are_the_same_floats(mapping, monkeypatch):
    model, params = _model(0.3, mapping)
    feats, labels = _batch(seed=1)
    model.train_step(feats, labels)
    got = {}
    for host in ('1', '0'):
        monkeypatch.setenv('LAS_HOST_METRICS', host)
        train_ed = model.train_edit_distance(labels)
        _, ed, pred = model.evaluate(feats, labels)
        got[host] = (train_ed, ed, pred['ctc_edit_distance'])
        assert all(type(v) is float for v in ed + pred['ctc_edit_distance']) and type(train_ed) is float
    assert got['1'] == got['0']
    assert got['0'][1][2] in (float('inf'), 0.0) and len(got['0'][1]) == 4
