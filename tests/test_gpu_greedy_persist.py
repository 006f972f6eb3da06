"""Greedy decoding in one launch per window (las_dec_persist with `greedy`; Speller / GeneralSpeller.forward_greedy behind
LasModel.predict and evaluate) on the GPU: route and launch count, exact invariants of a decode, the replay of its tokens
through the tested teacher-forced path, windows that carry state exactly, the step-by-step path end to end, evaluate, and
the shapes that must stay on the step-by-step path.

Shapes: listener L = 2, H = 64 (M = 128), F = 13, T = 24 with ragged source lengths whose longest is 22 frames (T' = 12,
max_it = 11: no multiple of 4); B = 11 (two groups of utterances, the second with three: rows bs >= B exist); decoder_units
128 and 256 (the lean kernel's one-tile and two-tile instantiations), Luong and Bahdanau, V = 11 (the lean projection's
V <= 64 path) and V = 100 (the general path; Vp = 104 is no multiple of 64); two cells at 128 units in both wirings, with
one-hot tokens, an embedding as a row table, and an embedding as a dense token feed (the operand-row columns the launch
rewrites).  Every model is trained on the device for 150 steps on one batch (random weights decode one dull token); the
'noeos' variant of a model has its </s> projection bias at -1e4, so that no utterance ever finishes: final_len = steps =
max_it for every row, and the last window ends exactly at the capacity."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import make_hparams, make_batch, to_device

pytestmark = pytest.mark.gpu

B, T = 11, 24
SRC_LEN = [22, 9, 17, 22, 12, 21, 5, 20, 16, 3, 19]
TGT_LEN = [6, 4, 5, 6, 3, 6, 2, 5, 4, 1, 6]
MAX_IT = 11

CASES = {
    'luong128_v11': dict(att='luong', Hd=128, V=11),
    'luong256_v100': dict(att='luong', Hd=256, V=100),
    'bahdanau128_v100': dict(att='bahdanau', Hd=128, V=100),
    'bahdanau256_v11': dict(att='bahdanau', Hd=256, V=11),
    'stack2_onehot': dict(att='luong', Hd=128, V=11, dec_layers=2, bottom_only=False),
    'multicell2_onehot': dict(att='bahdanau', Hd=128, V=11, dec_layers=2, bottom_only=True),
    'stack2_emb16': dict(att='bahdanau', Hd=128, V=11, dec_layers=2, bottom_only=False, emb=16),
    'multicell2_emb16_dense': dict(att='luong', Hd=128, V=100, dec_layers=2, bottom_only=True, emb=16, dense=True),
}
ONE_CELL = [c for c in CASES if 'dec_layers' not in CASES[c]]
ALL = list(CASES)

_TRAINED = {}


def _build(kw, dropout=0.0):
    from phones_las_amd import model_helper as mh
    kw = {k: v for k, v in kw.items() if k != 'dense'}
    ohp, params = make_hparams(F=13, L=2, H=64, pass_hidden=False, lr=1e-2, **kw)
    if dropout:
        params.decoder.set_hparam('dropout', dropout)
    return ohp, params, mh.LasModel(params, seed=5)


def trained(case):
    """(model, batch, feats, labels) of a case, trained once per session: 150 optimiser steps on one batch.  A 'dense' case
    decodes with a twin built with input dropout in its hyper-parameters (PREDICT applies none): the embedded token then
    travels in the operand row instead of a row table."""
    if case not in _TRAINED:
        kw = CASES[case]
        ohp, params, model = _build(kw)
        batch = make_batch(B=B, T=T, V=kw['V'], src_len=SRC_LEN, tgt_len=TGT_LEN)
        feats, labels = to_device(batch)
        first = last = None
        for _ in range(150):
            last = float(model.train_step(feats, labels))
            first = last if first is None else first
        assert last < 0.5 * first, (first, last)
        model.check_device_status()
        teacher = model
        if kw.get('dense'):
            _, _, twin = _build(kw, dropout=0.2)
            twin.load_variables({n: t.detach().clone() for n, t in model.vars.params.items()})
            assert twin.speller.tokx and twin.speller.T0 == 16
            model = twin
        _TRAINED[case] = (model, batch, feats, labels, teacher)
    return _TRAINED[case]


class variant:
    """'noeos': the </s> projection bias at -1e4 for the duration of the block."""

    def __init__(self, model, name):
        self.model, self.name = model, name

    def __enter__(self):
        if self.name == 'noeos':
            self.saved = {n: t.detach().clone() for n, t in self.model.vars.params.items()}
            new = dict(self.saved)
            b = new['speller/projection_layer/bias'].clone()
            b[self.model.params.decoder.eos_id] = -1e4
            new['speller/projection_layer/bias'] = b
            self.model.load_variables(new)
        return self.model

    def __exit__(self, *a):
        if self.name == 'noeos':
            self.model.load_variables(self.saved)


def decode(model, feats):
    pred = model.predict(feats)
    torch.cuda.synchronize()
    return (pred['logits'].clone(), pred['sample_ids'].clone(), pred['final_sequence_length'].clone(), pred['alignment'].clone())


def expected_final_len(ids, eos, steps):
    out = []
    for row in ids.tolist():
        out.append(row.index(eos) + 1 if eos in row else steps)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# 1. route and launch count
@pytest.mark.parametrize('case', ALL)
def test_route_and_launch_count(case, monkeypatch):
    """A supported model decodes on the one-launch route, in at most ceil(max_it / window) launches (the default window of 32
    covers max_it = 11 in one; LAS_DEC_GREEDY_WINDOW=4 needs at most three); LAS_DEC_PERSIST_GREEDY=0 and LAS_DEC_PERSIST=0
    reach the step-by-step path."""
    model, batch, feats, labels, _ = trained(case)
    monkeypatch.delenv('LAS_DEC_PERSIST_GREEDY', raising=False)
    monkeypatch.delenv('LAS_DEC_GREEDY_WINDOW', raising=False)
    decode(model, feats)
    sp = model.speller
    assert sp.last_decode_route == 'persist'
    assert 1 <= sp.last_decode_launches <= math.ceil(MAX_IT / 32)
    monkeypatch.setenv('LAS_DEC_GREEDY_WINDOW', '4')
    with variant(model, 'noeos'):
        decode(model, feats)
        assert sp.last_decode_route == 'persist' and sp.last_decode_launches == math.ceil(MAX_IT / 4)
    decode(model, feats)
    assert 1 <= sp.last_decode_launches <= math.ceil(MAX_IT / 4)
    for hook in ('LAS_DEC_PERSIST_GREEDY', 'LAS_DEC_PERSIST'):
        monkeypatch.setenv(hook, '0')
        decode(model, feats)
        assert sp.last_decode_route == 'steps' and sp.last_decode_launches == 0
        monkeypatch.delenv(hook)
    model.check_device_status()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. exact invariants of one decode
@pytest.mark.parametrize('var', ['trained', 'noeos'])
@pytest.mark.parametrize('case', ALL)
def test_exact_invariants_of_one_decode(case, var):
    """No tolerance: every sample id is NumPy's first-index argmax of the returned logits row; final_len is the first t + 1
    with </s>, else steps; steps = max(final_len) when every utterance finished, else max_it; the shapes follow; a second
    decode is torch.equal in every output."""
    model, batch, feats, labels, _ = trained(case)
    V, eos = CASES[case]['V'], model.params.decoder.eos_id
    with variant(model, var):
        lg, ids, fl, al = decode(model, feats)
        again = decode(model, feats)
    assert model.speller.last_decode_route == 'persist'
    steps = ids.shape[1]
    assert lg.shape == (B, steps, V) and ids.shape == (B, steps) and fl.shape == (B,) and al.shape[:2] == (B, steps)
    assert 1 <= steps <= MAX_IT
    assert np.array_equal(ids.cpu().numpy(), lg.cpu().numpy().argmax(-1))
    want = expected_final_len(ids.cpu(), eos, steps)
    assert fl.tolist() == want
    finished = [eos in r for r in ids.tolist()]
    assert steps == (max(want) if all(finished) else MAX_IT)
    if var == 'noeos':
        assert steps == MAX_IT and fl.tolist() == [MAX_IT] * B
    else:
        assert len(set(fl.tolist())) >= 3                        # utterances end at different steps
    assert torch.isfinite(lg).all() and torch.isfinite(al).all()
    assert float((al.sum(-1) - 1).abs().max()) < 1e-3
    for a, b in zip((lg, ids, fl, al), again):
        assert torch.equal(a, b)
    model.check_device_status()


@pytest.mark.parametrize('case', ['luong128_v11', 'bahdanau128_v100', 'stack2_onehot'])
def test_planted_tie_takes_the_lower_index(case):
    """Two projection columns zeroed and their biases set to the same large value: the two logits are the same number at every
    step, above all others; tf.argmax takes the lower index.  (A lane of the reduction holds v, v + 64, ...: 3 and 7 meet
    across lanes, 5 and 69 inside one lane.)"""
    model, batch, feats, labels, _ = trained(case)
    V = CASES[case]['V']
    pairs = [(3, 7)] + ([(5, 69)] if V > 69 else [])
    saved = {n: t.detach().clone() for n, t in model.vars.params.items()}
    try:
        for lo, hi in pairs:
            new = {n: t.clone() for n, t in saved.items()}
            new['speller/projection_layer/kernel'][:, [lo, hi]] = 0.0
            new['speller/projection_layer/bias'][[lo, hi]] = 40.0
            model.load_variables(new)
            lg, ids, fl, al = decode(model, feats)
            assert model.speller.last_decode_route == 'persist'
            assert torch.equal(lg[..., lo], lg[..., hi]) and float(lg[..., lo].min()) == 40.0
            assert float(lg.max()) == 40.0
            assert (ids == lo).all() and ids.shape[1] == MAX_IT and fl.tolist() == [MAX_IT] * B
    finally:
        model.load_variables(saved)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. replay through the teacher-forced path
def _teacher_forced(model, feats, tin, U):
    """The existing teacher-forced forward of the speller on the PREDICT-mode memory: logits, alignments, contexts, h."""
    from phones_las_amd.las import ops
    from phones_las_amd.las.model import Speller
    x, src_len = feats['encoder_inputs'], feats['source_sequence_length']
    if model._images_stale:
        model.refresh_images()
    (mem, mem_len), state = model.listener.forward(x, src_len, ops.PREDICT)
    sp = model.speller
    logits = sp.forward_train(mem, mem_len, state, tin, U)
    torch.cuda.synchronize()
    sv = sp.saved
    Tm = mem.shape[1]
    if isinstance(sp, Speller):
        out = (logits.clone(), sv['align'][:, :U, :Tm].clone(), sv['ctx_all'].clone(), sv['h_all'].clone())
    else:
        out = (logits.clone(), sv['align'][:, :U, :Tm].clone(), sv['ctx'].clone(), sv['h'][0].clone())
    sp.saved = None
    return out


@pytest.mark.parametrize('case', ALL)
def test_replay_through_the_teacher_forced_path(case):
    """[<s>, ids[:, :-1]] of the one-launch decode through forward_train (the one-launch training kernels, tested against
    float64).  A wrong fed token, a lost state row or a stale operand row shows as a gross error.
    Alignments, contexts and h ARE bit-equal between the two (same cell and attention code, same inputs): asserted with
    torch.equal.  The logits are not -- the decode adds the four parts' partial products and the bias, forward_train takes one
    GEMM over the whole row (measured: 2e-6 to 6e-6 at |logits| of 11 to 22) -- and are held to 2e-2 of their max-abs.
    The 'dense' case replays on the model it was trained as, the embedding folded into a row table, so the cell's token
    product rounds differently: alignments within 2e-2, contexts and h (bf16) within 1.6e-2 (measured 1.2e-4 / 3.9e-3, one
    bf16 ulp / 3.9e-3; logits 2.5e-3 of 22.6)."""
    model, batch, feats, labels, teacher = trained(case)
    V, sos = CASES[case]['V'], model.params.decoder.sos_id
    lg, ids, fl, al = decode(model, feats)
    assert model.speller.last_decode_route == 'persist'
    dec = model.speller.last_decode_buffers
    steps = ids.shape[1]
    tin = torch.cat([torch.full((B, 1), sos, dtype=torch.int32, device='cuda'), ids[:, :-1].to(torch.int32)], 1).contiguous()
    rl, ral, rctx, rh = _teacher_forced(teacher, feats, tin, steps)
    scale = float(rl[..., :V].abs().max())
    e_lg = float((lg - rl[..., :V]).abs().max())
    e_al = float((al - ral).abs().max())
    e_ctx = float((dec['ctx'].float() - rctx.float()).abs().max())
    e_h = float((dec['h'].float() - rh.float()).abs().max())
    print('replay %s: logits %.3g of %.3g, align %.3g, ctx %.3g (equal %s), h %.3g (equal %s)'
          % (case, e_lg, scale, e_al, e_ctx, torch.equal(dec['ctx'], rctx), e_h, torch.equal(dec['h'], rh)))
    assert e_lg < 2e-2 * scale
    if CASES[case].get('dense'):
        assert e_al < 2e-2 and e_ctx < 1.6e-2 and e_h < 1.6e-2
    else:
        assert torch.equal(al, ral) and torch.equal(dec['ctx'], rctx) and torch.equal(dec['h'], rh)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. windows carry state exactly
@pytest.mark.parametrize('var', ['trained', 'noeos'])
@pytest.mark.parametrize('case', ALL)
def test_windows_carry_state_exactly(case, var, monkeypatch):
    """LAS_DEC_GREEDY_WINDOW = 1, 4 and 16 >= max_it = 11 (no multiple of 4): all four outputs torch.equal.  The operand row and
    token handed over at a window's last step, the state rows, finished / final_len across launches, and -- 'noeos' -- windows
    that end exactly at max_it (the last step of the capacity writes no next row)."""
    model, batch, feats, labels, _ = trained(case)
    outs, launches = [], []
    with variant(model, var):
        for w in (1, 4, 16):
            monkeypatch.setenv('LAS_DEC_GREEDY_WINDOW', str(w))
            outs.append(decode(model, feats))
            assert model.speller.last_decode_route == 'persist'
            launches.append(model.speller.last_decode_launches)
    steps = outs[0][1].shape[1]
    assert launches[2] == 1 and launches[0] == steps and launches[1] == math.ceil(steps / 4)
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.shape == b.shape and torch.equal(a, b)
    model.check_device_status()


# ------------------------------------------------------------------------------------------------------------------------------
# 5. against the step-by-step path end to end
@pytest.mark.parametrize('case', ALL)
def test_against_the_step_by_step_path(case, monkeypatch):
    """The same weights with LAS_DEC_PERSIST_GREEDY=0.  Per utterance the comparison runs until the first step where the STEP
    path's top-1 minus top-2 logit is below m = 4 delta (a flip there legitimately changes every later input); before it: ids
    exactly, logits within 2e-2 of max-abs, alignments within 2e-2; final_len exactly for utterances compared to their end.
    delta is the largest logit difference between the two EXISTING teacher-forced routes on these weights (forward_train with
    LAS_DEC_PERSIST=0 against the default), a reference-only number measured here on every run: 2 delta is what a flip needs,
    doubled because training to these weights is only reproducible per build.  At least half of all steps and two whole
    utterances must be compared.
    Measured: delta = 0 for the Luong cases and the one-hot / dense two-cell cases (the two teacher-forced routes are bit-equal
    there, so m = 0 and every step is compared), 2.4e-6 (m = 9.5e-6) for stack2_emb16, 9.4e-4 (m = 3.8e-3) for bahdanau256_v11,
    2.2e-3 (m = 8.7e-3) for bahdanau128_v100.  Share compared: 100 % of the steps and 11 of 11 utterances in six cases, 95 %
    (61 of 64) and 10 of 11 for bahdanau256_v11, 88 % (42 of 48) and 10 of 11 for bahdanau128_v100; the step path met the cap
    with the first seed tried (model seed 5, batch seed 0)."""
    model, batch, feats, labels, teacher = trained(case)
    V = CASES[case]['V']
    U = max(TGT_LEN)
    monkeypatch.delenv('LAS_DEC_PERSIST', raising=False)
    a = _teacher_forced(teacher, feats, labels['targets_inputs'], U)[0]
    monkeypatch.setenv('LAS_DEC_PERSIST', '0')
    b = _teacher_forced(teacher, feats, labels['targets_inputs'], U)[0]
    monkeypatch.delenv('LAS_DEC_PERSIST')
    delta = float((a[..., :V] - b[..., :V]).abs().max())
    m = 4 * delta
    lg, ids, fl, al = decode(model, feats)
    assert model.speller.last_decode_route == 'persist'
    monkeypatch.setenv('LAS_DEC_PERSIST_GREEDY', '0')
    slg, sids, sfl, sal = decode(model, feats)
    assert model.speller.last_decode_route == 'steps'
    top2 = slg.topk(2, -1).values
    margin = (top2[..., 0] - top2[..., 1]).cpu()
    scale = float(slg.abs().max())
    compared = total = whole = 0
    for u in range(B):
        n = int(sfl[u])
        total += n
        ok = True
        for t in range(n):
            if float(margin[u, t]) < m:
                ok = False
                break
            assert t < ids.shape[1] and int(ids[u, t]) == int(sids[u, t]), (u, t, ids[u].tolist(), sids[u].tolist())
            assert float((lg[u, t] - slg[u, t]).abs().max()) < 2e-2 * scale, (u, t)
            assert float((al[u, t] - sal[u, t]).abs().max()) < 2e-2, (u, t)
            compared += 1
        if ok:
            whole += 1
            assert int(fl[u]) == n, (u, int(fl[u]), n)
    print('steps %s: delta %.3g, m %.3g, compared %d of %d steps, %d of %d utterances whole' % (case, delta, m, compared, total, whole, B))
    assert compared >= 0.5 * total and whole >= 2, (compared, total, whole, delta)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. evaluate end to end
@pytest.mark.parametrize('case', ['luong128_v11', 'bahdanau256_v11', 'bahdanau128_v100', 'multicell2_onehot', 'stack2_emb16'])
def test_evaluate_on_the_one_launch_route(case):
    """Loss (pad-to-the-longer rule) and edit distance of model.evaluate equal the oracle's formulas applied to the route's OWN
    logits and ids: 2e-3 relative for the loss, exact for the distances."""
    from oracle import las_oracle as O
    model, batch, feats, labels, _ = trained(case)
    loss, ed, pred = model.evaluate(feats, labels)
    torch.cuda.synchronize()
    assert model.speller.last_decode_route == 'persist'
    lg = pred['logits'].double().cpu()
    ids, fl = pred['sample_ids'].cpu().long(), pred['final_sequence_length'].cpu().long()
    own = O.compute_loss_eval(lg, batch['targets_outputs'], fl, batch['target_sequence_length'])
    assert abs(float(loss) - float(own)) < 2e-3 * abs(float(own)), (float(loss), float(own))
    assert np.allclose(ed, O.edit_distance(ids.tolist(), batch['targets_outputs'].tolist()))


# ------------------------------------------------------------------------------------------------------------------------------
# 7. fallbacks unchanged
def _toy_binf(nf, V, seed=5):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(nf, V, generator=g) < 0.5).float()
    m[nf - 1] = 0.0
    m[nf - 1, 2] = 1.0                # the last feature marks </s>
    return m


FALLBACKS = {
    'units64': dict(att='luong', Hd=64),
    'units512': dict(att='luong', Hd=512),
    'attention_layer': dict(att='luong', Hd=128, als=32),
    'luong_monotonic': dict(att='luong_monotonic', Hd=128),
    'sigmoid_outputs': dict(att='luong', Hd=128, sigmoid=True),
    'beam2': dict(att='luong', Hd=128, beam=2),
}


@pytest.mark.parametrize('name', list(FALLBACKS))
def test_fallbacks_stay_on_the_step_path(name, monkeypatch):
    """64- and 512-unit decoders, an attention layer, a monotonic attention, the sigmoid-output decoder and beam search: route
    'steps', and every output torch.equal with and without LAS_DEC_PERSIST_GREEDY=0."""
    from phones_las_amd import model_helper as mh
    kw = dict(FALLBACKS[name])
    beam = kw.pop('beam', 0)
    binf = None
    if kw.pop('sigmoid', False):
        binf = _toy_binf(8, 11)
        kw.update(binf=binf, sigmoid=True)
    ohp, params = make_hparams(F=13, L=2, H=64, V=11, pass_hidden=False, **kw)
    if beam:
        params.decoder.set_hparam('beam_width', beam)
    model = mh.LasModel(params, seed=3, binf2phone=binf)
    feats, _ = to_device(make_batch(B=5, T=24, src_len=[22, 9, 17, 22, 12], tgt_len=[6, 4, 5, 6, 3]))
    outs = []
    for flag in (None, '0'):
        if flag is None:
            monkeypatch.delenv('LAS_DEC_PERSIST_GREEDY', raising=False)
        else:
            monkeypatch.setenv('LAS_DEC_PERSIST_GREEDY', flag)
        pred = model.predict(feats)
        torch.cuda.synchronize()
        sp = model._beam_speller() if beam else model.speller
        assert sp.last_decode_route == 'steps' and sp.last_decode_launches == 0
        outs.append({k: v.clone() for k, v in pred.items() if torch.is_tensor(v)})
    assert outs[0].keys() == outs[1].keys() and 'sample_ids' in outs[0]
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


# ------------------------------------------------------------------------------------------------------------------------------
def test_one_cell_beyond_the_lean_lds_layout(monkeypatch):
    """T' = 720 frames (stacked, non-pyramidal listener) at 128 units: the lean kernel's LDS layout (keys and transposed values
    of a quarter of the frames, 171 KB) does not fit, and the one-cell decode takes the greedy instantiation of the general
    kernel.  decoding_length_factor 0.02 keeps the decode at max_it = 14 steps; the weights are untrained (a dull decode: the
    step-by-step path is not compared, its margins are below the rounding noise), so: the exact invariants, windows of 4
    against one launch, and the replay through forward_train at the tolerances of the dense case above."""
    from phones_las_amd import model_helper as mh
    src = [720, 331, 640, 720, 87, 512, 700, 19, 256, 600, 444]
    ohp, params = make_hparams(F=13, L=2, H=64, Hd=128, V=11, att='luong', pass_hidden=False, pyramidal=False)
    params.decoder.set_hparam('decoding_length_factor', 0.02)
    model = mh.LasModel(params, seed=9)
    feats, labels = to_device(make_batch(B=B, T=720, src_len=src, tgt_len=TGT_LEN))
    outs = []
    for w in (4, 16):
        monkeypatch.setenv('LAS_DEC_GREEDY_WINDOW', str(w))
        outs.append(decode(model, feats))
        assert model.speller.last_decode_route == 'persist'
    lg, ids, fl, al = outs[0]
    steps, eos, sos = ids.shape[1], model.params.decoder.eos_id, model.params.decoder.sos_id
    assert al.shape == (B, steps, 720) and 1 <= steps <= 14
    assert np.array_equal(ids.cpu().numpy(), lg.cpu().numpy().argmax(-1))
    want = expected_final_len(ids.cpu(), eos, steps)
    assert fl.tolist() == want and steps == (max(want) if all(eos in r for r in ids.tolist()) else 14)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    dec = model.speller.last_decode_buffers
    tin = torch.cat([torch.full((B, 1), sos, dtype=torch.int32, device='cuda'), ids[:, :-1].to(torch.int32)], 1).contiguous()
    rl, ral, rctx, rh = _teacher_forced(model, feats, tin, steps)
    assert float((lg - rl[..., :11]).abs().max()) < 2e-2 * float(rl[..., :11].abs().max())
    assert float((al - ral).abs().max()) < 2e-2
    assert float((dec['ctx'].float() - rctx.float()).abs().max()) < 1.6e-2
    assert float((dec['h'].float() - rh.float()).abs().max()) < 1.6e-2
    model.check_device_status()


def test_planted_status_word_in_the_greedy_workspace_is_reported():
    """The sticky-status route of a greedy launch: a status word planted in the decode's workspace survives further decodes (the
    launches clear everything behind the header only) and LasModel.check_device_status raises once, then is clear."""
    from phones_las_amd import hip
    model, batch, feats, labels, _ = trained('luong128_v11')
    decode(model, feats)
    assert model.speller.last_decode_route == 'persist'
    ws = model.speller._persist_cache['fwd']
    assert model.speller._persist_ws is ws
    model.check_device_status()
    ws[:4].view(torch.int32).fill_(8)
    decode(model, feats)
    assert int(ws[:4].view(torch.int32).item()) == 8
    with pytest.raises(hip.LasError):
        model.check_device_status()
    model.check_device_status()
