"""tests/decoder_step_restated.py against independent references, without a GPU: the forward against the oracle's lstm_step,
Attention.__call__ (all five attention types) and monotonic_attention ('parallel', 'hard') in float64 with the bf16 roundings
switched off; the backward against torch.autograd in float64 on the same forward, every attention x {softmax, parallel}, with
mem_len of 0 / 1 / Tm and an engaged 1e-10 clip.  Then the conditions the kernel tests (tests/test_gpu_decoder_step.py) rely on,
for the committed cases, with no exclusions."""
import numpy as np
import pytest
import torch

import tests.decoder_step_restated as R
from oracle import las_oracle as O
from tests.rng_restated import bf2f

T64 = torch.float64


def _t(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=T64)


def _close(got, ref, tol=1e-11):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()


# ---- forward against the oracle ---------------------------------------------------------------------------------------------
def test_cell_against_oracle_lstm_step():
    r = np.random.default_rng(1)
    B, Hd, E = 4, 24, 5
    kernel, bias = r.standard_normal((E + Hd, 4 * Hd)) * 0.3, r.standard_normal(4 * Hd) * 0.2
    h_prev, c_prev = r.standard_normal((B, Hd)) * 0.5, r.standard_normal((B, Hd))
    ids = np.array([0, E - 1, 2, 2])
    onehot = np.eye(E)[ids]
    c_ref, h_ref = O.lstm_step(_t(onehot), _t(c_prev), _t(h_prev), _t(kernel), _t(bias))
    gates, c, h = R.cell_fwd(h_prev @ kernel[E:], bias, c_prev, kernel[:E], ids)
    _close(c, c_ref.numpy())
    _close(h, h_ref.numpy())
    # a dropped / scaled one-hot entry is the one-hot vector times the scale
    scale = np.array([0.0, 1.25, 1.25, 0.0])
    c_ref, h_ref = O.lstm_step(_t(onehot * scale[:, None]), _t(c_prev), _t(h_prev), _t(kernel), _t(bias))
    gates, c, h = R.cell_fwd(h_prev @ kernel[E:], bias, c_prev, kernel[:E], ids, scale)
    _close(c, c_ref.numpy())
    _close(h, h_ref.numpy())
    Hd4 = gates[:, 2 * Hd:3 * Hd]
    assert ((Hd4 > 0) & (Hd4 < 1)).all()


def _oracle_attention(att, train, memory, lens, wq, v, bias):
    Hd = memory.shape[2]
    hp = O.HP(decoder=O.DecoderHP(num_units=Hd, attention_type=R.ATT_NAMES[att]))
    params = {'speller/memory_layer/kernel': torch.eye(Hd, dtype=T64), 'speller/query_layer/kernel': _t(wq),
              'speller/attention_v': _t(v), 'speller/attention_score_bias': _t([bias])}
    return O.Attention(hp, params, _t(memory), torch.tensor(lens), O.make_q('f64'), train=train)


@pytest.mark.parametrize('att', range(5), ids=R.ATT_NAMES)
@pytest.mark.parametrize('train', [True, False], ids=['train', 'infer'])
def test_attention_against_oracle(att, train):
    """Scores, normaliser and alignments of every attention type; bahdanau_monotonic at inference is the 'hard' mode."""
    r = np.random.default_rng(10 + att)
    B, Hd, Tm = 4, 16, 23
    lens = [Tm, 1, 9, Tm + 4]
    memory = r.standard_normal((B, Tm, Hd))
    wq, v, bias = r.standard_normal((Hd, Hd)) * 0.4, r.standard_normal(Hd), -0.6
    query = r.standard_normal((B, Hd)) * 0.7
    prev = r.random((B, Tm))
    prev /= prev.sum(-1, keepdims=True)
    A = _oracle_attention(att, train, memory, lens, wq, v, bias)
    want = A(_t(query), _t(prev)).numpy()
    on = np.arange(Tm)[None, :] < np.minimum(lens, Tm)[:, None]
    keys = memory * on[:, :, None]
    if att == R.CUSTOM:
        keys = np.maximum(keys, 0.0)
    pq = R.processed_query(att, query, wq) if R.uses_wq(att) else None
    sc = R.scores(att, query, pq, keys, v)
    mono = att in (R.LUONG_MONO, R.BAHDANAU_MONO)
    norm = R.SOFTMAX if not mono else (R.HARD if att == R.BAHDANAU_MONO and not train else R.PARALLEL)
    p, align = R.normalise(norm, sc + (bias if mono else 0.0), lens, prev)
    _close(align, want)
    if norm == R.SOFTMAX:
        _close(align.sum(-1), np.ones(B))


@pytest.mark.parametrize('mode', ['parallel', 'hard'])
@pytest.mark.parametrize('given_prev', [False, True], ids=['dirac', 'prev'])
def test_monotonic_attention_against_oracle(mode, given_prev):
    """Including p of exactly 0 and 1 (the clips at float32 tiny and 1e-10 engaged) and the dirac of a NULL prev_align."""
    r = np.random.default_rng(3)
    B, Tm = 3, 40
    sv = r.standard_normal((B, Tm)) * 3
    sv[0, 5], sv[1, 7] = 800.0, -800.0                     # sigmoid gives exactly 1.0 and 0.0 in float64
    prev = r.random((B, Tm)) ** 3
    prev /= prev.sum(-1, keepdims=True)
    p_ref = torch.sigmoid(_t(sv)) if mode == 'parallel' else (_t(sv) > 0).to(T64)
    pr = _t(prev) if given_prev else _t(R.dirac(B, Tm))
    want = O.monotonic_attention(p_ref, pr, mode).numpy()
    p, align = R.normalise(R.PARALLEL if mode == 'parallel' else R.HARD, sv, [Tm] * B, prev if given_prev else None)
    _close(p, p_ref.numpy())
    _close(align, want)
    assert (p == 1.0).any() and (p == 0.0).any()


def test_empty_memory_gives_zero_alignments_and_noise_index():
    sv = np.random.default_rng(4).standard_normal((2, 9))
    for norm in (R.SOFTMAX, R.PARALLEL, R.HARD):
        _, a = R.normalise(norm, sv, [0, 9])
        assert (a[0] == 0).all() and a[1].sum() > 0
    from tests.rng_restated import normal
    got = R.noisy_scores(np.zeros((2, 9)), 0.25, 1.0, 0x77, 3, 5)
    assert got[1, 4] == 0.25 + normal(0x77, 3, np.uint64((5 * 2 + 1) * 9 + 4))


# ---- backward against torch.autograd ----------------------------------------------------------------------------------------
def _torch_step(att, norm, x, lens):
    """One fused step in float64 torch from leaf tensors x; the monotonic normaliser is the oracle's."""
    z = x['z'] + x['bias']
    i, j, f, o = z.chunk(4, dim=1)
    gates = torch.cat([torch.sigmoid(i), torch.tanh(j), torch.sigmoid(f + 1.0), torch.sigmoid(o)], 1)
    c = torch.sigmoid(f + 1.0) * x['c_prev'] + torch.sigmoid(i) * torch.tanh(j)
    h = torch.sigmoid(o) * torch.tanh(c)
    B, Tm = x['keys'].shape[:2]
    on = torch.arange(Tm)[None, :] < torch.tensor(np.minimum(lens, Tm))[:, None]
    pq_pre = pq = None
    if R.uses_wq(att):
        pq_pre = h @ x['wq']
        pq_pre.retain_grad()
        pq = torch.relu(pq_pre) if att == R.CUSTOM else pq_pre
    if R.additive(att):
        score = torch.einsum('h,bth->bt', x['att_v'], torch.tanh(x['keys'] + pq[:, None, :]))
    else:
        score = torch.einsum('bh,bth->bt', pq if att == R.CUSTOM else h, x['keys'])
    score.retain_grad()
    p = None
    if norm == R.SOFTMAX:
        m = torch.where(on, score, torch.full_like(score, -1e300)).max(-1, keepdim=True).values.detach()
        e = torch.where(on, torch.exp(torch.where(on, score - m, torch.zeros_like(score))), torch.zeros_like(score))
        align = e / e.sum(-1, keepdim=True).clamp_min(1e-300)
    else:
        p = torch.sigmoid(score + x['score_bias']) * on.to(T64)
        align = O.monotonic_attention(p, x['prev_align'], 'parallel')
    ctx = torch.einsum('bt,btm->bm', align, x['values'])
    return dict(gates=gates, c=c, h=h, pq_pre=pq_pre, pq=pq, score=score, p=p, align=align, ctx=ctx)


@pytest.mark.parametrize('att', range(5), ids=R.ATT_NAMES)
@pytest.mark.parametrize('norm,clip', [(R.SOFTMAX, False), (R.PARALLEL, False), (R.PARALLEL, True)],
                         ids=['softmax', 'parallel', 'parallel_clip_1e-10_engaged'])
def test_backward_against_autograd(att, norm, clip):
    r = np.random.default_rng(100 + 10 * att + norm)
    B, Hd, M, Tm = 5, 16, 12, 60 if clip else 21
    lens = [0, 1, Tm, Tm + 3, Tm // 2]
    case = dict(att=att, norm=norm, mode=R.FUSED, B=B, Hd=Hd, M=M, Tm=Tm, keep=1.0, seed=0, stream=0, step=0, feed_width=M)
    on = np.arange(Tm)[None, :] < np.minimum(lens, Tm)[:, None]
    keys = r.standard_normal((B, Tm, Hd)) * 0.5
    if att == R.CUSTOM:
        keys = np.maximum(keys, 0.0)
    prev = r.random((B, Tm)) ** 3
    prev /= prev.sum(-1, keepdims=True)
    lead = dict(z=r.standard_normal((B, 4 * Hd)), bias=r.standard_normal(4 * Hd) * 0.2, c_prev=r.standard_normal((B, Hd)),
                keys=bf2f(R._bf(keys)), values=bf2f(R._bf(r.standard_normal((B, Tm, M)) * on[:, :, None])),
                wq=bf2f(R._bf(r.standard_normal((Hd, Hd)) * 0.4)), att_v=r.standard_normal(Hd),
                score_bias=np.array([2.5 if clip else -0.4]), prev_align=prev)        # clip: p near 0.9, c under 1e-10 after ten frames
    x = {k: _t(v).requires_grad_(True) for k, v in lead.items()}
    f = _torch_step(att, norm, x, lens)
    if clip:
        cex = R.monotonic_chain(f['p'].detach().numpy(), prev)[0]
        assert (cex < 1e-10).any()
    dctx_a, dctx_b = r.standard_normal((B, M)), r.standard_normal((B, M))
    dh_rec, dh_b, dc_in, carry = (r.standard_normal(s) for s in ((B, Hd), (B, Hd), (B, Hd), (B, Tm)))
    loss = (f['ctx'] * _t(dctx_a + dctx_b)).sum() + (f['h'] * _t(dh_rec + dh_b)).sum() + (f['c'] * _t(dc_in)).sum()
    if norm == R.PARALLEL:
        loss = loss + (f['align'] * _t(carry)).sum()
    loss.backward()
    inp = dict(dctx_a=dctx_a, dctx_b=dctx_b, dh_rec=dh_rec, dh_b=dh_b, dh_c=None, dc=dc_in, gates=f['gates'].detach().numpy(),
               c_new=f['c'].detach().numpy(), c_prev=lead['c_prev'], align=f['align'].detach().numpy(), mem_len=np.array(lens),
               keys=R._bf(lead['keys']), values=R._bf(lead['values']), carry=carry, prev_align=prev)
    if R.uses_wq(att):
        inp['pq'] = f['pq'].detach().numpy()
        inp['wq_t'] = R._bf(lead['wq'].T)
    if R.additive(att):
        inp['att_v'] = lead['att_v']
    if norm == R.PARALLEL:
        inp['p'] = f['p'].detach().numpy()
    got = R.bwd_reference(case, inp)
    _close(got['dz'], x['z'].grad.numpy(), 1e-9)
    _close(got['dc'], x['c_prev'].grad.numpy(), 1e-9)
    _close(got['ds'], np.where(on, f['score'].grad.numpy(), 0.0), 1e-9)
    _close(got['dctx'], dctx_a + dctx_b)
    if R.uses_wq(att):
        _close(got['dpq'], f['pq_pre'].grad.numpy(), 1e-9)
    if R.additive(att):
        _close(got['dkeys'], x['keys'].grad.numpy(), 1e-9)
        _close(got['dv'], x['att_v'].grad.numpy(), 1e-9)
    if norm == R.PARALLEL:
        _close(got['carry'], x['prev_align'].grad.numpy(), 1e-9)
        _close(np.array([got['dbias']]), x['score_bias'].grad.numpy(), 1e-9)


def test_backward_modes_and_masks():
    """CELL_ONLY takes its dh from the extra sources alone; ATTENTION_ONLY stops at d(query) = what FUSED feeds its cell; the feed
    mask on dctx_b is step t+1's draw with the division in fp32."""
    case = next(c for c in R.BWD_CASES if c['name'] == 'dctx_b_dropped')
    inp = R.bwd_inputs(case)
    full = R.bwd_reference(case, inp)
    kept = full['kept']
    want = inp['dctx_a'].astype(np.float64) + np.where(kept, (inp['dctx_b'] / np.float32(0.8)).astype(np.float64), 0.0)
    assert (full['dctx'] == want).all()
    att_only = R.bwd_reference(dict(case, mode=R.ATTENTION_ONLY), inp)
    _close(att_only['dq'] + inp['dh_rec'], full['dh'])
    cell = R.bwd_reference(dict(case, mode=R.CELL_ONLY), inp)
    _close(cell['dh'], inp['dh_rec'])


# ---- the conditions the kernel tests rely on --------------------------------------------------------------------------------
def test_case_names_are_unique():
    for table in (R.FWD_CASES, R.SPLIT_CASES, R.BWD_CASES):
        names = [c['name'] for c in table]
        assert len(set(names)) == len(names)


def test_hard_cases_keep_their_margin():
    hard = [c for c in R.FWD_CASES if c['norm'] == R.HARD and not c['refuse']]
    assert len(hard) >= 4
    for case in hard:
        inp = R.fwd_inputs(case)
        ref = R.fwd_reference(case, inp)
        on = np.arange(case['Tm'])[None, :] < np.minimum(case['lens'], case['Tm'])[:, None]
        assert np.abs(ref['sv'][on]).min() >= R.HARD_MARGIN, case['name']
        assert (ref['p'][on] == 1).any() and (ref['p'][on] == 0).any(), case['name']


def test_monotonic_backward_cases_stay_off_the_clip_edge():
    """No exclusive cumprod c of a monotonic backward case lies in [1e-11, 1e-9] (the gradient gate of clip(c, 1e-10, 1) must fall
    the same way in fp32 and in float64); cases with p exactly 0.0f and 1.0f are present, and so is an engaged clip."""
    mono = [c for c in R.BWD_CASES if c['norm'] == R.PARALLEL and not c['refuse']]
    assert len(mono) >= 6
    zero = one = engaged = 0
    for case in mono:
        inp = R.bwd_inputs(case)
        Tm = case['Tm']
        on = np.arange(Tm)[None, :] < np.minimum(case['lens'], Tm)[:, None]
        p = np.where(on, inp['p'].astype(np.float64), 0.0)
        c = R.monotonic_chain(p, R.dirac(case['B'], Tm))[0]
        assert not ((c >= 1e-11) & (c <= 1e-9)).any(), case['name']
        x = 1.0 - p
        assert not ((x > 0) & (x < 1e-6)).any(), case['name']                 # 1 - p is exactly 0 or well inside its clip
        zero += int((inp['p'][on] == 0).any())
        one += int((inp['p'][on] == 1).any())
        engaged += int((c < 1e-10).any())
    assert zero and one and engaged


def test_dropout_cases_draw_both_outcomes():
    drop = [c for c in R.FWD_CASES if c['keep'] < 1.0]
    assert len(drop) >= 5
    for case in drop:
        if case['tok']:
            inp = R.fwd_inputs(case)
            sc = R.tok_scale(case['B'], inp['tok_ids'], case['keep'], case['seed'], case['stream'], case['step'], case['feed_width'])
            assert (sc == 0).any() and (sc > 1).any(), case['name']
        if case['feed_plain'] != 1:
            _, kept = R.feed_copy(np.zeros((case['B'], case['M']), dtype=np.uint16), case['keep'], case['feed_plain'], case['seed'],
                                  case['stream'], case['feed_stream0'], case['step'], case['feed_width'], case['tok'])
            assert kept.any() and (~kept).any(), case['name']
    for case in (c for c in R.BWD_CASES if c['keep'] < 1.0):
        kept = R.feed_grad_mask(case['B'], case['M'], case['keep'], case['seed'], case['stream'], case['step'], case['feed_width'])
        assert kept.any() and (~kept).any(), case['name']


def test_custom_backward_cases_have_zero_pq_entries():
    for case in (c for c in R.BWD_CASES if c['att'] == R.CUSTOM and not c['refuse']):
        pq = R.bwd_inputs(case)['pq']
        assert (pq == 0).any() and (pq > 0).any(), case['name']


def test_cases_cover_what_the_kernel_tests_promise():
    f = [c for c in R.FWD_CASES if not c['refuse']]
    assert {64, 128, 256, 512, 1024, 72, 24} <= {c['Hd'] for c in f}
    assert {1, 63, 64, 65, 255, 256, 257, 600} <= {c['Tm'] for c in f}
    assert {8, 24, 128, 512, 1024, 2056} <= {c['M'] for c in f}
    assert set(range(5)) == {c['att'] for c in f} and set(range(3)) == {c['norm'] for c in f} == {c['mode'] for c in f}
    assert {0, 1, 2} == {c['feed_plain'] for c in f if c['keep'] < 1.0}
    b = [c for c in R.BWD_CASES if not c['refuse']]
    assert {64, 128, 256, 512, 1024} <= {c['Hd'] for c in b}
    assert {128, 512, 640, 1024, 1152} <= {c['M'] for c in b}
    assert {1, 100, 129, 255, 256, 257, 300} <= {c['Tm'] for c in b}
    assert set(range(5)) == {c['att'] for c in b} and set(range(3)) == {c['mode'] for c in b}
    # the LDS limits of the forward entry point at Hd = 64: floats 2 Hd + Tm + 16 + 2048 (+ 2 Tm monotonic) within 64 KiB
    assert (2 * 64 + 14192 + 16 + 2048) * 4 == 64 * 1024 and (2 * 64 + 3 * 4730 + 16 + 2048) * 4 <= 64 * 1024 < (2 * 64 + 3 * 4731 + 16 + 2048) * 4
