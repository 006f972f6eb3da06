"""The device route of the beam search (one las_beam_advance per step, windows, las_beam_gather_tree) against the host loop
(LAS_BEAM_HOST=1: the token-by-token loop, which the oracle tests of tests/test_gpu_model.py pin): ids, lengths and log-probs
equal bit for bit for every decoder kind, window and prefix; and a vocabulary the host loop's las_beam_step refuses."""
import numpy as np
import pytest
import torch

from tests.helpers import make_hparams, make_batch, to_device

pytestmark = pytest.mark.gpu
DT = torch.float64
K = 3


def _toy_binf(nf, V, seed=5):
    """A 0/1 feature-by-phone matrix with the structure of utils.load_binf2phone (tests/test_gpu_model.py builds the same)."""
    rng = np.random.default_rng(seed)
    m = (rng.random((nf, V)) < 0.4).astype(np.float32)
    m[:, 0] = 1.0
    m[:, 1:3] = 0.0
    m[nf - 2:, :] = 0.0
    m[nf - 2, 1] = 1.0
    m[nf - 1, 2] = 1.0
    return m


def _model(dropout=0.0, eos_bias=None, seed=7, **kw):
    from oracle import las_oracle as O
    from phones_las_amd import model_helper as mh
    ohp, params = make_hparams(**kw)
    if dropout:                  # the embedded token travels in the operand row (inference keeps everything)
        params.decoder.set_hparam('dropout', dropout)
    op = O.init_params(ohp, bias_scale=0.1)
    V = ohp.decoder.target_vocab_size
    g = torch.Generator().manual_seed(seed)
    op['speller/projection_layer/bias'] = torch.randn(V, generator=g, dtype=DT) * 1.5
    if eos_bias is not None:
        op['speller/projection_layer/bias'][O.EOS_ID] = eos_bias
    model = mh.LasModel(params, binf2phone=kw.get('binf'))
    model.load_variables({k: v for k, v in op.items()})
    model.params.decoder.set_hparam('beam_width', K)
    return O, model


def _feats(V=11):
    batch = make_batch(V=V, src_len=[12, 7, 10], tgt_len=[6, 4, 5])
    return to_device(batch)[0]


def _predict(model, feats, monkeypatch, host=False, window=None):
    monkeypatch.setenv('LAS_BEAM_HOST', '1' if host else '0')
    if window is None:
        monkeypatch.delenv('LAS_BEAM_WINDOW', raising=False)
    else:
        monkeypatch.setenv('LAS_BEAM_WINDOW', str(window))
    pred = model.predict(feats)
    torch.cuda.synchronize()
    return pred, model._beam_speller()


def _same(a, b, tag):
    assert a['sample_ids'].dtype == b['sample_ids'].dtype and a['sample_ids'].shape == b['sample_ids'].shape, tag
    assert torch.equal(a['sample_ids'], b['sample_ids']), (tag, a['sample_ids'][0].T.tolist(), b['sample_ids'][0].T.tolist())
    assert torch.equal(a['beam_lengths'], b['beam_lengths']), tag
    assert torch.equal(a['beam_log_probs'].view(torch.int32), b['beam_log_probs'].view(torch.int32)), tag


def _routes_agree(model, feats, monkeypatch, L=0):
    """Host route once, device route at windows 1, 2 and the default 32; returns the host prediction and its steps."""
    ref, sp = _predict(model, feats, monkeypatch, host=True)
    assert sp.last_decode_route == 'steps' and sp.last_decode_syncs == 0
    for w in (1, 2, None):
        got, sp = _predict(model, feats, monkeypatch, window=w)
        assert sp.last_decode_route == 'beam_device'
        wv = w or 32
        enq = sp.last_decode_launches + L                     # the steps enqueued: every search step launches one advance
        assert sp.last_decode_syncs == -(-enq // wv), (w, enq, sp.last_decode_syncs)
        _same(got, ref, 'window %s' % w)
    return ref


KINDS = {
    'one_cell_luong': dict(att='luong', dec_layers=1),
    'two_cells_bahdanau_al_bottom': dict(att='bahdanau', dec_layers=2, bottom_only=True, als=16),
    'two_cells_luong_monotonic': dict(att='luong_monotonic', dec_layers=2, bottom_only=True, als=16),
    'two_cells_stacked_luong': dict(att='luong', dec_layers=2, bottom_only=False, pass_hidden=False),
    'embedding': dict(att='luong', dec_layers=1, emb=8),
    'embedding_in_the_operand_row': dict(att='luong', dec_layers=2, bottom_only=True, emb=8, dropout=0.2),
    'binf_projection': dict(att='luong', dec_layers=1, binf=_toy_binf(8, 11)),
}


@pytest.mark.parametrize('kind', list(KINDS))
def test_device_route_equals_host_route(kind, monkeypatch):
    O, model = _model(**KINDS[kind])
    feats = _feats()
    ref = _routes_agree(model, feats, monkeypatch)
    assert ref['sample_ids'].shape[2] == K and ref['sample_ids'].shape[1] >= 1
    partial = torch.tensor([[O.SOS_ID, 5, 7], [O.SOS_ID, 3, 3], [O.SOS_ID, 9, 4]], dtype=torch.int32).cuda()
    _routes_agree(model, dict(feats, partial_targets=partial), monkeypatch, L=3)


def test_search_that_ends_inside_a_window(monkeypatch):
    """A favoured </s>: every utterance finishes after a few steps, windows of 2 and 32 enqueue steps past the end, and the
    frozen launches leave the state of the end."""
    O, model = _model(att='luong', dec_layers=1, eos_bias=6.0)
    ref = _routes_agree(model, _feats(), monkeypatch)
    got, sp = _predict(model, _feats(), monkeypatch, window=32)
    steps = ref['sample_ids'].shape[1]
    assert steps < sp.last_decode_launches                      # steps were enqueued past the end ...
    assert int(ref['beam_lengths'].max()) == steps              # ... and the end is the last beam's </s>


def test_search_pushed_to_capacity(monkeypatch):
    """</s> at -30: nobody finishes, the search stops at the capacity of the buffers."""
    O, model = _model(att='bahdanau', dec_layers=2, bottom_only=True, als=16, eos_bias=-30.0)
    ref = _routes_agree(model, _feats(), monkeypatch)
    got, sp = _predict(model, _feats(), monkeypatch, window=4)
    assert ref['sample_ids'].shape[1] == sp.last_decode_launches
    assert (ref['beam_lengths'] == ref['sample_ids'].shape[1]).all() and (ref['sample_ids'] != O.EOS_ID).all()


def test_large_vocabulary_only_the_device_route_runs(monkeypatch):
    """K = 8 over V = 2 100: the host loop's las_beam_step refuses the 16 800 candidates; the device route decodes.  (What is
    selected at that size is tests/test_gpu_beam_advance.py's matter; here: the shape of the result and window independence.)"""
    from phones_las_amd import hip
    V = 2100
    O, model = _model(att='luong', dec_layers=1, V=V)
    model.params.decoder.set_hparam('beam_width', 8)
    feats = _feats(V=V)
    with pytest.raises(hip.LasError, match='LDS'):
        _predict(model, feats, monkeypatch, host=True)
    a, sp = _predict(model, feats, monkeypatch, window=1)
    b, sp = _predict(model, feats, monkeypatch, window=32)
    assert sp.last_decode_route == 'beam_device'
    _same(a, b, 'windows 1 and 32')
    ids, lens, lps = b['sample_ids'].cpu(), b['beam_lengths'].cpu(), b['beam_log_probs'].cpu()
    B, steps, K8 = ids.shape
    assert (B, K8) == (3, 8) and tuple(lens.shape) == (3, 8) and int(lens.max()) <= steps
    for bb in range(B):
        for k in range(K8):
            assert (ids[bb, int(lens[bb, k]):, k] == O.EOS_ID).all()
    assert (lps[:, :-1] >= lps[:, 1:]).all() and torch.isfinite(lps).all()
