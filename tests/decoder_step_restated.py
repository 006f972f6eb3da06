"""One decoder step -- las_decoder_step_fwd and las_decoder_step_bwd of csrc/decoder.hip -- restated in NumPy float64 from the
contract in include/las_hip.h and SURVEY.md Appendix A.5-A.7 / F: the LSTM cell (token row gather, tok_scale, bias, forget bias 1,
gate order i, j, f, o), the processed query, the five score forms, the length-masked softmax, tf.contrib.seq2seq's
monotonic_attention 'parallel' and 'hard' (safe_cumprod in log space, the clips at float32 tiny and 1e-10), the context and the
copy that feeds the next step under the three feed_plain schemes; backward the d(context) sum, d(alignments), the softmax and
monotonic backward with TF's clip_by_value gradient gates, the Luong and additive query paths and the cell.  Nothing follows the
kernels' code: no fast exponentials, no lane layouts, no chunking.  Values are rounded to bf16 exactly where the kernel's operands
are bf16 (h_t; CustomAttention's processed query; the stored context, dz, ds, dpq, d(context) copy); round=False switches those
roundings off for the comparison with the oracle and with torch.autograd (tests/test_decoder_step_host.py).

Staging.  Where the kernel rounds an intermediate to bf16 and then consumes it, the later stage's reference starts from the
kernel's own bf16 output (fwd_reference(..., h_bits=, pq_bits=)): a half-ulp flip in h is charged to h alone.

The second half holds the inputs and the case tables of tests/test_gpu_decoder_step.py, each case named for the path or edge it
exists for.  Uses f2bf, bf2f, uniform and normal of tests/rng_restated.py; imports nothing from the project."""
import zlib

import numpy as np

from tests.rng_restated import bf2f, f2bf, normal, uniform

F64, F32 = np.float64, np.float32
TINY = float(np.finfo(np.float32).tiny)
LUONG, BAHDANAU, CUSTOM, LUONG_MONO, BAHDANAU_MONO = range(5)
SOFTMAX, PARALLEL, HARD = range(3)
FUSED, CELL_ONLY, ATTENTION_ONLY = range(3)
ATT_NAMES = ('luong', 'bahdanau', 'custom', 'luong_monotonic', 'bahdanau_monotonic')
HARD_MARGIN = 1e-2            # |score + bias| of every valid frame of a HARD case (asserted on the host)


def additive(att):
    return att in (BAHDANAU, BAHDANAU_MONO)


def uses_wq(att):
    return additive(att) or att == CUSTOM


def rbf(x):
    """Round to bf16 and back (float64 in, float64 out)."""
    return bf2f(f2bf(np.asarray(x, dtype=F64).astype(F32))).astype(F64)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _lens(mem_len, Tm):
    return np.minimum(np.asarray(mem_len, dtype=np.int64), Tm)


# ---- forward ----------------------------------------------------------------------------------------------------------------
def tok_scale(B, tok_ids, keep, seed, stream, step, feed_width):
    """The DropoutWrapper outcome of the one-hot feed's single non-zero entry: draw (step*B + b)*feed_width + id."""
    if not keep < 1.0:
        return np.ones(B, dtype=F64)
    idx = (np.uint64(step) * np.uint64(B) + np.arange(B, dtype=np.uint64)) * np.uint64(feed_width) + np.asarray(tok_ids, dtype=np.uint64)
    return np.where(uniform(seed, stream, idx) < F32(keep), F32(1.0) / F32(keep), F32(0.0)).astype(F64)


def cell_fwd(z, bias, c_prev, tok_rows=None, tok_ids=None, scale=None):
    """z [B, 4Hd] (+ scale_b * tok_rows[id_b]) + bias -> (gates [B, 4Hd] = i, j, f, o activated, c [B, Hd], h [B, Hd] unrounded)."""
    z = np.asarray(z, dtype=F64) + np.asarray(bias, dtype=F64)[None, :]
    B, Hd = z.shape[0], z.shape[1] // 4
    if tok_rows is not None:
        rows = np.asarray(tok_rows, dtype=F64)[np.asarray(tok_ids, dtype=np.int64)]
        z = z + (np.ones(B) if scale is None else scale)[:, None] * rows
    i, j, f, o = (z[:, g * Hd:(g + 1) * Hd] for g in range(4))
    gi, gj, gf, go = _sigmoid(i), np.tanh(j), _sigmoid(f + 1.0), _sigmoid(o)
    c = gf * np.asarray(c_prev, dtype=F64) + gi * gj
    return np.concatenate([gi, gj, gf, go], 1), c, go * np.tanh(c)


def processed_query(att, h, wq):
    """h Wq (Wq [in, out]); CustomAttention: relu.  Unrounded."""
    pq = np.asarray(h, dtype=F64) @ np.asarray(wq, dtype=F64)
    return np.maximum(pq, 0.0) if att == CUSTOM else pq


def scores(att, h, pq, keys, v):
    """[B, Tm]: h . keys (Luong), pq . keys (Custom), v . tanh(keys + pq) (Bahdanau); score_bias is the normaliser's."""
    keys = np.asarray(keys, dtype=F64)
    if additive(att):
        return np.einsum('h,bth->bt', np.asarray(v, dtype=F64), np.tanh(keys + pq[:, None, :]))
    return np.einsum('bh,bth->bt', pq if att == CUSTOM else h, keys)


def dirac(B, Tm):
    a = np.zeros((B, Tm), dtype=F64)
    a[:, 0] = 1.0
    return a


def monotonic_chain(p, prev):
    """'parallel': (c, cc, S, a) with c = exclusive cumprod(1 - p) in log space, cc = clip(c, 1e-10, 1), S = cumsum(prev / cc)."""
    lx = np.log(np.clip(1.0 - p, TINY, 1.0))
    c = np.exp(np.cumsum(lx, -1) - lx)
    cc = np.clip(c, 1e-10, 1.0)
    S = np.cumsum(prev / cc, -1)
    return c, cc, S, p * c * S


def noisy_scores(score, bias, noise_scale, noise_seed, noise_stream, step):
    B, Tm = score.shape
    sv = score + bias
    if noise_scale > 0:
        idx = ((np.uint64(step) * np.uint64(B) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(Tm)
               + np.arange(Tm, dtype=np.uint64)[None, :])
        sv = sv + float(F32(noise_scale)) * normal(noise_seed, noise_stream, idx)
    return sv


def normalise(norm, sv, mem_len, prev=None):
    """sv [B, Tm]: the scores with bias and noise.  -> (p_choose or None, alignments); frames from min(mem_len, Tm) on: p = 0,
    alignment 0; an empty memory gives all-zero softmax alignments."""
    B, Tm = sv.shape
    on = np.arange(Tm)[None, :] < _lens(mem_len, Tm)[:, None]
    if norm == SOFTMAX:
        with np.errstate(invalid='ignore', over='ignore'):
            m = np.where(on, sv, -np.inf).max(-1, keepdims=True)
            e = np.where(on, np.exp(np.where(on, sv - m, 0.0)), 0.0)
        tot = e.sum(-1, keepdims=True)
        return None, np.where(tot > 0, e / np.where(tot > 0, tot, 1.0), 0.0)
    prev = dirac(B, Tm) if prev is None else np.asarray(prev, dtype=F64)
    if norm == PARALLEL:
        p = np.where(on, _sigmoid(np.where(on, sv, 0.0)), 0.0)
        return p, monotonic_chain(p, prev)[3]
    p = np.where(on & (np.where(on, sv, 0.0) > 0), 1.0, 0.0)
    q = p * np.cumsum(prev, -1)
    excl = np.cumprod(np.concatenate([np.ones((B, 1)), 1.0 - q], -1), -1)[:, :-1]
    return p, q * excl


def context(align, values):
    return np.einsum('bt,btm->bm', align, np.asarray(values, dtype=F64))


def feed_copy(ctx_bits, keep, feed_plain, seed, stream, feed_stream0, step, feed_width, has_tok):
    """ctx_out2 from the bits of ctx_out [B, M], exactly (fp32 arithmetic on a bf16 value, one bf16 rounding): -> (bits, kept)."""
    ctx_bits = np.asarray(ctx_bits, dtype=np.uint16)
    B, M = ctx_bits.shape
    if not keep < 1.0 or feed_plain == 1:
        return ctx_bits.copy(), np.ones((B, M), dtype=bool)
    b, col = np.arange(B, dtype=np.uint64)[:, None], np.arange(M, dtype=np.uint64)[None, :]
    if feed_plain == 2:
        W2 = M if has_tok else max(feed_width, M)
        u = uniform(seed, (feed_stream0 + step + 1) & 0xFFFFFFFF, b * np.uint64(W2) + np.uint64(W2 - M) + col)
        val = bf2f(ctx_bits) * (F32(1.0) / F32(keep))
    else:
        u = uniform(seed, stream, (np.uint64(step + 1) * np.uint64(B) + b) * np.uint64(feed_width) + np.uint64(feed_width - M) + col)
        val = bf2f(ctx_bits) / F32(keep)
    kept = u < F32(keep)
    return np.where(kept, f2bf(val.astype(F32)), np.uint16(0)).astype(np.uint16), kept


def fwd_reference(case, inp, h_bits=None, pq_bits=None, round=True):
    """Every output of one forward step as float64 (the values BEFORE their storage rounding, except where `round` rounds an
    operand).  h_bits / pq_bits: the kernel's own bf16 h_t / Custom processed query to start the later stages from."""
    att, norm, mode, B, Tm = case['att'], case['norm'], case['mode'], case['B'], case['Tm']
    out = {}
    if mode == ATTENTION_ONLY:
        h = bf2f(inp['query']).astype(F64)
    else:
        sc = tok_scale(B, inp['tok_ids'], case['keep'], case['seed'], case['stream'], case['step'], case['feed_width']) if case['tok'] else None
        out['tok_scale'] = sc
        out['gates'], out['c'], out['h'] = cell_fwd(inp['z'], inp['bias'], inp['c_prev'],
                                                    bf2f(inp['tok_rows']) if case['tok'] else None, inp['tok_ids'], sc)
        h = bf2f(h_bits).astype(F64) if h_bits is not None else (rbf(out['h']) if round else out['h'])
    if mode == CELL_ONLY:
        return out
    pq = None
    if uses_wq(att):
        pq = out['pq'] = processed_query(att, h, bf2f(inp['wq']))
        if att == CUSTOM:
            pq = bf2f(pq_bits).astype(F64) if pq_bits is not None else (rbf(pq) if round else pq)
    out['score'] = scores(att, h, pq, bf2f(inp['keys']), inp.get('att_v'))
    sv = out['score']
    if norm != SOFTMAX:
        sv = out['sv'] = noisy_scores(sv, float(inp['score_bias'][0]), case['noise'], case['noise_seed'], case['noise_stream'], case['step'])
    out['p'], out['align'] = normalise(norm, sv, inp['mem_len'], inp.get('prev_align'))
    out['ctx'] = context(out['align'], bf2f(inp['values']))
    return out


# ---- backward ---------------------------------------------------------------------------------------------------------------
def feed_grad_mask(B, M, keep, seed, stream, step, feed_width):
    """Step t+1's attention-feed mask on dctx_b: [B, M] factors 1/keep or 0 (fp32 division: v / keep)."""
    if not keep < 1.0:
        return np.ones((B, M), dtype=bool)
    b, col = np.arange(B, dtype=np.uint64)[:, None], np.arange(M, dtype=np.uint64)[None, :]
    return uniform(seed, stream, (np.uint64(step + 1) * np.uint64(B) + b) * np.uint64(feed_width) + np.uint64(feed_width - M) + col) < F32(keep)


def monotonic_bwd(da, p, prev):
    """Backward of a = p c S through TF's graph: clip_by_value passes a gradient only where its input lies inside the clip
    (bounds included).  -> (d p, d prev)."""
    c, cc, S, _ = monotonic_chain(p, prev)
    dS = da * p * c
    du = np.cumsum(dS[:, ::-1], -1)[:, ::-1]                    # sum_{i >= t} dS[i]
    dprev = du / cc
    dc = da * p * S - np.where((c >= 1e-10) & (c <= 1.0), du * prev / (cc * cc), 0.0)
    dcs = dc * c
    dlx = np.cumsum(dcs[:, ::-1], -1)[:, ::-1] - dcs            # sum_{j > t} dcs[j]
    x = 1.0 - p
    dp = da * c * S - np.where((x >= TINY) & (x <= 1.0), dlx / np.clip(x, TINY, 1.0), 0.0)
    return dp, dprev


def cell_bwd(dh, dc, gates, c_new, c_prev):
    """-> (dz [B, 4Hd] unrounded, dc_{t-1})."""
    gates = np.asarray(gates, dtype=F64)
    Hd = gates.shape[1] // 4
    gi, gj, gf, go = (gates[:, g * Hd:(g + 1) * Hd] for g in range(4))
    tc = np.tanh(np.asarray(c_new, dtype=F64))
    dct = np.asarray(dc, dtype=F64) + dh * go * (1.0 - tc * tc)
    dz = np.concatenate([dct * gj * gi * (1.0 - gi), dct * gi * (1.0 - gj * gj),
                         dct * np.asarray(c_prev, dtype=F64) * gf * (1.0 - gf), dh * tc * go * (1.0 - go)], 1)
    return dz, dct * gf


def bwd_reference(case, inp):
    """Every output of one backward step as float64, before its storage rounding; the accumulators as the AMOUNT added."""
    att, norm, mode, B, Hd, M, Tm = (case[k] for k in ('att', 'norm', 'mode', 'B', 'Hd', 'M', 'Tm'))
    out = {}
    dh = np.zeros((B, Hd), dtype=F64)
    if mode != CELL_ONLY:
        on = np.arange(Tm)[None, :] < _lens(inp['mem_len'], Tm)[:, None]
        dctx = np.zeros((B, M), dtype=F64) if inp.get('dctx_a') is None else np.asarray(inp['dctx_a'], dtype=F64).copy()
        if inp.get('dctx_b') is not None:
            kept = feed_grad_mask(B, M, case['keep'], case['seed'], case['stream'], case['step'], case['feed_width'])
            fb = np.asarray(inp['dctx_b'])
            if case['keep'] < 1.0:                                  # the kernel's own fp32 quotient of an fp32 input
                fb = (fb.astype(F32) / F32(case['keep'])).astype(F32)
            dctx = dctx + np.where(kept, fb.astype(F64), 0.0)
            out['kept'] = kept
        out['dctx'] = dctx
        dalign = np.where(on, np.einsum('bm,btm->bt', dctx, bf2f(inp['values']).astype(F64)), 0.0)
        out['dalign'] = dalign
        if norm == SOFTMAX:
            a = np.where(on, np.asarray(inp['align'], dtype=F64), 0.0)
            ds = a * (dalign - (a * dalign).sum(-1, keepdims=True))
        else:
            p = np.where(on, np.asarray(inp['p'], dtype=F64), 0.0)
            prev = dirac(B, Tm) if inp.get('prev_align') is None else np.asarray(inp['prev_align'], dtype=F64)
            dp, out['carry'] = monotonic_bwd(dalign + np.asarray(inp['carry'], dtype=F64), p, prev)
            ds = np.where(on, dp * p * (1.0 - p), 0.0)
            out['dbias'] = ds.sum()
        out['ds'] = ds
        keys = bf2f(inp['keys']).astype(F64)
        if additive(att):
            th = np.tanh(keys + np.asarray(inp['pq'], dtype=F64)[:, None, :])
            out['dv'] = np.einsum('bt,bth->h', ds, th)
            out['dkeys'] = ds[:, :, None] * np.asarray(inp['att_v'], dtype=F64)[None, None, :] * (1.0 - th * th)
            dq = out['dkeys'].sum(1)
        else:
            dq = np.einsum('bt,bth->bh', ds, keys)
        if att == CUSTOM:
            dq = np.where(np.asarray(inp['pq']) > 0, dq, 0.0)
        if uses_wq(att):
            out['dpq'] = dq
            dq = dq @ bf2f(inp['wq_t']).astype(F64)             # dh[u] = sum_a dpq[a] Wq[u][a]; wq_t is [out, in]
        dh = dq
        if mode == ATTENTION_ONLY:
            out['dq'] = dh
            return out
    for k in ('dh_rec', 'dh_b', 'dh_c'):
        if inp.get(k) is not None:
            dh = dh + np.asarray(inp[k], dtype=F64)
    out['dh'] = dh
    out['dz'], out['dc'] = cell_bwd(dh, inp['dc'], inp['gates'], inp['c_new'], inp['c_prev'])
    return out


# ---- inputs and case tables -------------------------------------------------------------------------------------------------
E_TOK = 5                     # rows of the token-feed kernel


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _bf(x):
    return f2bf(np.asarray(x, dtype=F32))


def ragged(B, Tm):
    """Tm, half, a third, above Tm (clamped), 0: the first B of them."""
    return [Tm, (Tm + 1) // 2, max(1, Tm // 3), Tm + 5, 0][:B]


def _memory(r, case, key_query=None):
    """keys [B, Tm, Hd] bf16 with scores of order 1 (finite garbage beyond mem_len: masking is the normaliser's job), values
    [B, Tm, M] bf16, zero beyond mem_len as the contract says."""
    B, Hd, M, Tm = case['B'], case['Hd'], case['M'], case['Tm']
    lens = _lens(case['lens'], Tm)
    on = np.arange(Tm)[None, :] < lens[:, None]
    keys = r.standard_normal((B, Tm, Hd)) * (case.get('key_scale', 3.0) / np.sqrt(Hd))
    if case['att'] == CUSTOM:
        keys = np.maximum(keys, 0.0)
    keys = np.where(on[:, :, None], keys, 7.0)
    values = np.where(on[:, :, None], r.standard_normal((B, Tm, M)), 0.0)
    return _bf(keys), _bf(values)


FWD_DEFAULTS = dict(B=3, Hd=64, M=128, Tm=65, att=LUONG, norm=SOFTMAX, mode=FUSED, parts=1, lens=None, tok=True, keep=1.0,
                    feed_plain=0, feed_width=None, step=0, prev=False, bias=0.0, noise=0.0, optional=True,
                    seed=0x1234, stream=7, feed_stream0=100, noise_seed=0x77, noise_stream=3, refuse=False)


def _fc(name, **kw):
    c = dict(FWD_DEFAULTS, name=name, **kw)
    if c['lens'] is None:
        c['lens'] = ragged(c['B'], c['Tm'])
    if c['feed_width'] is None:
        c['feed_width'] = E_TOK + c['M']
    assert len(c['lens']) == c['B']
    return c


def fwd_inputs(case):
    """Everything a forward launch reads: fp32 arrays, bf16 as uint16 bits.  HARD cases: a valid frame whose score lies within 5x
    the margin of the threshold gets a new key row until none does (the margin is asserted in tests/test_decoder_step_host.py)."""
    r = _rng(case['name'])
    B, Hd, M, Tm, att = case['B'], case['Hd'], case['M'], case['Tm'], case['att']
    inp = dict(z=r.standard_normal((B, 4 * Hd)).astype(F32), bias=(0.2 * r.standard_normal(4 * Hd)).astype(F32),
               c_prev=(0.7 * r.standard_normal((B, Hd))).astype(F32), tok_rows=_bf(0.5 * r.standard_normal((E_TOK, 4 * Hd))),
               tok_ids=np.array([0, E_TOK - 1, 2, 1, 3][:B], dtype=np.int32), mem_len=np.array(case['lens'], dtype=np.int32),
               query=_bf(0.5 * r.standard_normal((B, Hd))), score_bias=np.array([case['bias']], dtype=F32))
    inp['keys'], inp['values'] = _memory(r, case)
    if uses_wq(att):
        inp['wq'] = _bf(r.standard_normal((Hd, Hd)) * (1.5 / np.sqrt(Hd)))
    if additive(att):
        inp['att_v'] = (r.standard_normal(Hd) * (3.0 / np.sqrt(Hd))).astype(F32)
    if case['prev']:
        pa = r.random((B, Tm)) ** 4 * (np.arange(Tm)[None, :] < np.maximum(_lens(case['lens'], Tm), 1)[:, None])
        inp['prev_align'] = (pa / pa.sum(-1, keepdims=True)).astype(F32)
    if case['norm'] == HARD and not case['refuse']:
        on = np.arange(Tm)[None, :] < _lens(case['lens'], Tm)[:, None]
        for _ in range(200):
            sv = fwd_reference(case, inp)['sv']
            bad = on & (np.abs(sv) < 5 * HARD_MARGIN)
            if not bad.any():
                break
            fresh = r.standard_normal((B, Tm, Hd)) * (3.0 / np.sqrt(Hd))
            inp['keys'] = np.where(bad[:, :, None], _bf(fresh), inp['keys'])
    return inp


_A = dict(att=BAHDANAU)
_C = dict(att=CUSTOM)
FWD_CASES = [
    # ---- widths: the score phase's pieces per lane, the rolled loop, the cell loop's laps
    _fc('Hd64_nk2'), _fc('Hd128_nk4', Hd=128), _fc('Hd256_nk8', Hd=256, **_A),
    _fc('Hd512_rolled', Hd=512, B=2), _fc('Hd512_rolled_additive', Hd=512, B=2, **_A), _fc('Hd1024_rolled_custom', Hd=1024, B=2, **_C),
    _fc('Hd128_additive', Hd=128, **_A), _fc('Hd64_custom', **_C),
    # ---- accepted widths that are no multiple of 32 (the last Hd % 32 units must enter the scores)
    _fc('Hd72_luong', Hd=72), _fc('Hd72_bahdanau', Hd=72, **_A), _fc('Hd72_custom', Hd=72, **_C),
    _fc('Hd24_luong', Hd=24), _fc('Hd24_bahdanau', Hd=24, **_A), _fc('Hd24_custom', Hd=24, **_C),
    # ---- memory lengths: one frame, the 64-frame pass, the 256-frame group of four passes, context passes with a tail
    _fc('Tm1', Tm=1, B=2, lens=[1, 0]), _fc('Tm63', Tm=63), _fc('Tm64', Tm=64), _fc('Tm255', Tm=255), _fc('Tm256', Tm=256, **_A),
    _fc('Tm257', Tm=257), _fc('Tm600_context_tail', Tm=600, **_C),
    _fc('mem_len_0_1_Tm_above', B=5, Tm=70, lens=[0, 1, 70, 99, 33]),
    _fc('mem_len_0_1_Tm_above_additive', B=5, Tm=70, lens=[0, 1, 70, 99, 33], **_A),
    # ---- memory depths and the context phase's lane layout
    _fc('M8', M=8), _fc('M24_parts4_empty_part', M=24, parts=4), _fc('M8_parts4_above_M_over_8', M=8, parts=4),
    _fc('M512_parts4', M=512, parts=4), _fc('M1024', M=1024, B=2), _fc('M2056_second_chunk', M=2056, B=2, Tm=40),
    _fc('M2056_parts4', M=2056, B=2, Tm=40, parts=4),
    # ---- normalisers: registers (Tm <= 256) and LDS, NULL and given prev_align, score bias, noise
    _fc('parallel_reg_dirac', att=LUONG_MONO, norm=PARALLEL, Tm=100, bias=-2.7),
    _fc('parallel_reg_prev', att=BAHDANAU_MONO, norm=PARALLEL, Tm=256, prev=True, bias=-3.1, B=5, lens=[256, 0, 1, 300, 77]),
    _fc('parallel_lds_dirac', att=BAHDANAU_MONO, norm=PARALLEL, Tm=257, bias=-3.5),
    _fc('parallel_lds_prev', att=LUONG_MONO, norm=PARALLEL, Tm=300, prev=True, bias=-3.3, B=5, lens=[300, 0, 1, 400, 129]),
    _fc('parallel_noise1_step3', att=BAHDANAU_MONO, norm=PARALLEL, Tm=90, prev=True, noise=1.0, step=3, bias=-2.2),
    _fc('parallel_lds_noise1', att=LUONG_MONO, norm=PARALLEL, Tm=270, noise=1.0, step=2, bias=-3.6),
    _fc('hard_reg_dirac', att=BAHDANAU_MONO, norm=HARD, Tm=100, bias=-0.6),
    _fc('hard_reg_prev', att=LUONG_MONO, norm=HARD, Tm=256, prev=True, bias=0.5, B=5, lens=[256, 0, 1, 300, 77]),
    _fc('hard_lds_dirac', att=LUONG_MONO, norm=HARD, Tm=257, bias=-0.4),
    _fc('hard_lds_prev', att=BAHDANAU_MONO, norm=HARD, Tm=300, prev=True, bias=0.6),
    _fc('softmax_prev_ignored', att=LUONG, Tm=80, prev=True), _fc('softmax_prev_ignored_Tm300', att=BAHDANAU, Tm=300, prev=True),
    # ---- modes
    _fc('cell_only', mode=CELL_ONLY, Hd=128), _fc('attention_only_query_copy', mode=ATTENTION_ONLY, Hd=128, **_A),
    _fc('attention_only_no_optional', mode=ATTENTION_ONLY, optional=False), _fc('no_optional_outputs', optional=False, **_A),
    _fc('no_token_rows', tok=False),
    # ---- input dropout: the three feed_plain schemes, a feed wider than M, a later step, a dense token vector in front
    _fc('drop_plain0', B=5, keep=0.8, lens=[65] * 5), _fc('drop_plain1', B=5, keep=0.8, feed_plain=1, lens=[65] * 5),
    _fc('drop_plain2', B=5, keep=0.8, feed_plain=2, lens=[65] * 5, step=1),
    _fc('drop_plain0_wide_feed_step2', B=5, keep=0.8, feed_width=300, step=2, lens=[65] * 5, M=24, parts=4),
    _fc('drop_plain2_no_tok_window', B=5, keep=0.8, feed_plain=2, tok=False, feed_width=200, lens=[65] * 5, step=4),
    # ---- the longest memories the LDS check admits at Hd = 64, and one frame more
    _fc('Tm14192_softmax_limit', Tm=14192, M=8, B=2, lens=[14192, 9000]),
    _fc('Tm14193_softmax_refused', Tm=14193, M=8, B=2, lens=[14193, 9000], refuse=True),
    _fc('Tm4730_monotonic_limit', Tm=4730, M=8, B=2, lens=[4730, 3000], att=LUONG_MONO, norm=PARALLEL, bias=-6.0, key_scale=1.0),
    _fc('Tm4731_monotonic_refused', Tm=4731, M=8, B=2, lens=[4731, 3000], att=LUONG_MONO, norm=PARALLEL, refuse=True),
]
# a fused launch against CELL_ONLY followed by ATTENTION_ONLY on its h_out
SPLIT_CASES = [_fc('split_luong', Hd=128), _fc('split_bahdanau_parallel', att=BAHDANAU_MONO, norm=PARALLEL, Tm=120, bias=-2.3, Hd=256),
               _fc('split_custom_Hd512', Hd=512, B=2, **_C)]

BWD_DEFAULTS = dict(B=3, Hd=64, M=128, Tm=100, att=LUONG, norm=SOFTMAX, mode=FUSED, lens=None, keep=1.0, feed_width=None, step=0,
                    prev=False, carry=False, dctx_a=True, dctx_b=True, dh=('dh_rec',), optional=True, acc0=False, p01=False,
                    seed=0x4321, stream=9, refuse=False)


def _bc(name, **kw):
    c = dict(BWD_DEFAULTS, name=name, **kw)
    if c['lens'] is None:
        c['lens'] = ragged(c['B'], c['Tm'])
    if c['feed_width'] is None:
        c['feed_width'] = E_TOK + c['M']
    assert len(c['lens']) == c['B']
    return c


def bwd_inputs(case):
    """Everything a backward launch reads.  The saved tensors are free inputs of the kernel: gates inside their ranges, alignments
    a distribution over the valid frames, p_choose small enough that the exclusive cumprod c stays above 1e-9 (p01: one frame
    with p = 1.0f exactly, behind which c drops to float32 tiny at once -- the 1e-10 clip engaged, nothing near its edge -- and
    some with p = 0.0f)."""
    r = _rng(case['name'])
    B, Hd, M, Tm, att = case['B'], case['Hd'], case['M'], case['Tm'], case['att']
    lens = _lens(case['lens'], Tm)
    on = np.arange(Tm)[None, :] < lens[:, None]
    g = r.standard_normal((B, 4 * Hd))
    gates = np.concatenate([_sigmoid(g[:, :Hd]), np.tanh(g[:, Hd:2 * Hd]), _sigmoid(g[:, 2 * Hd:3 * Hd] + 1), _sigmoid(g[:, 3 * Hd:])], 1)
    al = r.random((B, Tm)) ** 3 * on
    inp = dict(gates=gates.astype(F32), c_new=(0.8 * r.standard_normal((B, Hd))).astype(F32),
               c_prev=(0.8 * r.standard_normal((B, Hd))).astype(F32), dc=(0.3 * r.standard_normal((B, Hd))).astype(F32),
               align=(al / np.maximum(al.sum(-1, keepdims=True), 1e-30)).astype(F32), mem_len=np.array(case['lens'], dtype=np.int32),
               dctx_a=(r.standard_normal((B, M)) / np.sqrt(M)).astype(F32) if case['dctx_a'] else None,
               dctx_b=(r.standard_normal((B, M)) / np.sqrt(M)).astype(F32) if case['dctx_b'] else None)
    inp['keys'], inp['values'] = _memory(r, case)
    for k in ('dh_rec', 'dh_b', 'dh_c'):
        inp[k] = (0.2 * r.standard_normal((B, Hd))).astype(F32) if k in case['dh'] else None
    if uses_wq(att):
        inp['wq_t'] = _bf(r.standard_normal((Hd, Hd)) * (1.5 / np.sqrt(Hd)))
        pq = 0.6 * r.standard_normal((B, Hd))
        inp['pq'] = (bf2f(_bf(np.maximum(pq, 0.0))) if att == CUSTOM else pq).astype(F32)     # Custom: entries exactly 0
    if additive(att):
        inp['att_v'] = (r.standard_normal(Hd) * (3.0 / np.sqrt(Hd))).astype(F32)
    if case['norm'] != SOFTMAX:
        p = r.random((B, Tm)) ** 2 * min(0.5, 12.0 / Tm)
        p[:, 0] = 0.3
        if case['p01']:
            p[:, min(Tm - 1, 2 * Tm // 3)] = 1.0
            p[:, 1:Tm:7] = 0.0
        inp['p'] = p.astype(F32)
        inp['carry'] = ((0.3 * r.standard_normal((B, Tm))) if case['carry'] else np.zeros((B, Tm))).astype(F32)
        if case['prev']:
            pa = r.random((B, Tm)) ** 4 * (np.arange(Tm)[None, :] < np.maximum(lens, 1)[:, None])
            if case['p01']:
                pa[:, 2 * Tm // 3:] = 0.0          # attention cannot be behind a frame that was chosen with certainty
            inp['prev_align'] = (pa / pa.sum(-1, keepdims=True)).astype(F32)
    return inp


_P = dict(norm=PARALLEL)
BWD_CASES = [
    # ---- widths: P = 256 / (Hd / 8) frame phases from 32 down to 2
    _bc('Hd64_P32'), _bc('Hd128_P16', Hd=128, **_A), _bc('Hd256_P8', Hd=256, **_C), _bc('Hd512_P4', Hd=512, B=2, **_A),
    _bc('Hd1024_P2', Hd=1024, B=2, **_A), _bc('Hd1024_P2_custom', Hd=1024, B=2, **_C), _bc('Hd512_luong', Hd=512, B=2),
    # ---- memory depths: the three d(alignments) paths (M / 128 <= 4, <= 8, above) and their boundaries
    _bc('M512_path1_edge', M=512), _bc('M640_path2', M=640), _bc('M1024_path2_edge', M=1024, B=2), _bc('M1152_path3', M=1152, B=2),
    # ---- memory lengths
    _bc('Tm1', Tm=1, B=2, lens=[1, 0]), _bc('Tm129', Tm=129, **_A), _bc('Tm255', Tm=255), _bc('Tm256', Tm=256), _bc('Tm257', Tm=257, **_A),
    _bc('Tm300', Tm=300, **_C), _bc('mem_len_0_1_above', B=5, Tm=100, lens=[0, 1, 100, 140, 37]),
    _bc('mem_len_0_1_above_additive', B=5, Tm=100, lens=[0, 1, 100, 140, 37], **_A),
    # ---- monotonic chain in registers (Tm <= 256) and in LDS, with the clip gates
    _bc('parallel_reg', att=LUONG_MONO, Tm=100, **_P), _bc('parallel_reg_prev_carry', att=BAHDANAU_MONO, Tm=256, prev=True, carry=True, **_P),
    _bc('parallel_lds', att=BAHDANAU_MONO, Tm=257, **_P), _bc('parallel_lds_prev_carry', att=LUONG_MONO, Tm=300, prev=True, carry=True, **_P),
    _bc('parallel_reg_p01_clip', att=LUONG_MONO, Tm=129, prev=True, carry=True, p01=True, **_P),
    _bc('parallel_lds_p01_clip', att=BAHDANAU_MONO, Tm=300, prev=True, carry=True, p01=True, **_P),
    _bc('parallel_mem_len_0_1_above', att=LUONG_MONO, B=5, Tm=100, lens=[0, 1, 100, 140, 37], carry=True, **_P),
    _bc('parallel_lds_mem_len_0_1_above', att=BAHDANAU_MONO, B=5, Tm=260, lens=[0, 1, 260, 300, 37], carry=True, prev=True, **_P),
    # ---- accumulators that hold values before the launch
    _bc('acc_nonzero_additive', acc0=True, Tm=129, Hd=128, **_A), _bc('acc_nonzero_parallel', att=BAHDANAU_MONO, acc0=True, carry=True, **_P),
    # ---- gradient sources
    _bc('dctx_a_null', dctx_a=False), _bc('dctx_b_null', dctx_b=False, **_A), _bc('dctx_b_dropped', keep=0.8, step=2, B=5, lens=[100] * 5),
    _bc('dctx_b_dropped_wide_feed', keep=0.8, step=1, feed_width=300, **_C),
    _bc('dh_none', dh=()), _bc('dh_b_only', dh=('dh_b',)), _bc('dh_c_only', dh=('dh_c',)), _bc('dh_all', dh=('dh_rec', 'dh_b', 'dh_c'), **_A),
    _bc('no_optional_outputs', optional=False, **_A), _bc('no_optional_outputs_custom', optional=False, **_C),
    # ---- modes
    _bc('cell_only', mode=CELL_ONLY, Hd=128, dh=('dh_rec', 'dh_b')), _bc('attention_only', mode=ATTENTION_ONLY, Hd=128, **_A),
    _bc('attention_only_parallel', mode=ATTENTION_ONLY, att=LUONG_MONO, carry=True, **_P),
    # ---- refusals
    _bc('refuse_Hd96', Hd=96, refuse=True), _bc('refuse_M64', M=64, refuse=True), _bc('refuse_hard', att=LUONG_MONO, norm=HARD, refuse=True),
    _bc('refuse_lds_budget', Tm=12100, B=2, lens=[12100, 5], refuse=True),
]
