"""las_decoder_step_fwd and las_decoder_step_bwd -- the general path of the speller and the yardstick of the one-launch decoder
kernels -- through the C-ABI against the float64 restatement of tests/decoder_step_restated.py (which
tests/test_decoder_step_host.py checks against the oracle and torch.autograd).  The cases and the path or edge each exists for are
listed there (FWD_CASES, SPLIT_CASES, BWD_CASES).

Every output buffer starts as a sentinel and has rows wider than the data; what lies outside an output's window must still hold
the sentinel afterwards, and a refused launch leaves everything as it was.

Comparison, element by element: |kernel - ref| <= REL |ref| + EPS * scale, scale = the largest |ref| of that output in the case.
bf16 outputs: REL = 2^-8.  fp32 outputs: REL = 2^-23 F, F the roundings that act on the output's VALUE along its longest chain
(listed above TOL); what enters as an absolute error instead -- the rounding of a sum's terms against the sum's size, the fast-math
exp / tanh / sigmoid -- is what EPS measures.  Each EPS is four times the largest figure (|kernel - ref| - REL |ref|) / scale measured
over all cases of that output on an MI355X, 0 where it is never positive; every test prints FIGURE <output> <case> <value> for
every output before it asserts.  Exact equality where nothing is rounded: HARD p_out, dropped elements, zeros beyond mem_len,
copies (h_out2, the query copy, ctx_out2 against ctx_out -- through the feed mask in fp32 arithmetic --, align_bf16 against
align_out).  Staging: the reference of a stage that consumes a bf16 value the kernel itself produced (h_t, Custom's processed
query) starts from the kernel's bits; that value is checked against float64 by itself.  The whole file runs in a few seconds."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.decoder_step_restated as R
from tests.rng_restated import bf2f, f2bf

pytestmark = pytest.mark.gpu

BF16_REL = 2.0 ** -8
FP32_REL = 2.0 ** -23
SENT_BF16 = 0xC040            # -3.0: what the output buffers hold before a launch
SENT_F32 = -3.0
# The largest score error behind a p_choose of the PARALLEL cases, |p - ref| / (p (1 - p)): measured 1.47e-6 (case
# parallel_noise1_step3).  The HARD cases' margin, |score + bias| >= 1e-2 at every valid frame, is 6800 times that.
SCORE_ERR = 1.47e-6


def _dot(n):
    """Roundings of an n-term dot product along one accumulation chain (a product and a sum each) and its tree of partials."""
    return 2 * n + 8


# output -> (REL as a function of the case, EPS).  EPS: 4 x the largest figure measured on an MI355X (the figure and its case beside
# it; LABNOTES.md), 0 where the figure was never positive.  F of the fp32 outputs:
#   gates 4    z + bias, + scale * row, the activation's reciprocal and its result
#   c 10       two gates of 4 each in a product, the sum of the two products
#   pq, dq     a dot product's chain: 2 Hd + 8 (see _dot)
#   p 6        score + bias, + noise, the sigmoid's exp, sum, reciprocal
#   align 8    softmax: exp, 1 / sum, product, the sum's tree;  12  monotonic: log, exp, the clip quotient, two products, the scans
#   dc 12      dc + dh go (1 - tc^2), times gf; tanh and its square
#   carry 12   da p c, the reverse scan's tree, the quotient by clip(c)
#   dkeys 8    ds v (1 - th^2) and the sum onto what the buffer held
#   dv, dbias  a sum over the frames: 2 Tm + 8
TOL = {
    # ---- forward
    'gates': (lambda c: 4 * FP32_REL, 4.7e-7),                   # measured 1.16e-7, case M512_parts4
    'c': (lambda c: 10 * FP32_REL, 2.8e-7),                      # measured 6.81e-8, case hard_lds_dirac
    'h': (lambda c: BF16_REL, 0.0),                              # measured -3.6e-8: never positive
    # (Custom's processed query is a bf16 value in an fp32 buffer)
    'pq': (lambda c: BF16_REL if c['att'] == R.CUSTOM else _dot(c['Hd']) * FP32_REL, 1.1e-9),   # measured 2.64e-10, case hard_lds_prev
    'p': (lambda c: 6 * FP32_REL, 5.3e-7),                       # measured 1.30e-7, case parallel_lds_noise1
    'align': (lambda c: (8 if c['norm'] == R.SOFTMAX else 12) * FP32_REL, 3.4e-7),   # measured 8.41e-8, case Tm4730_monotonic_limit
    'ctx': (lambda c: BF16_REL, 2.7e-8),                         # measured 6.69e-9, case mem_len_0_1_Tm_above_additive
    # ---- backward
    'dctx_save': (lambda c: BF16_REL, 0.0),                      # measured -6.1e-8: never positive
    'ds': (lambda c: BF16_REL, 3.2e-7),                          # measured 7.91e-8, case parallel_reg_prev_carry
    'dz': (lambda c: BF16_REL, 1.8e-10),                         # measured 4.46e-11, case Tm300
    'dpq': (lambda c: BF16_REL, 6.6e-7),                         # measured 1.64e-7, case Hd1024_P2
    'dc': (lambda c: 12 * FP32_REL, 2.2e-7),                     # measured 5.44e-8, case mem_len_0_1_above_additive
    'dq': (lambda c: _dot(c['Hd']) * FP32_REL, 1.5e-6),          # measured 3.59e-7, case attention_only
    'carry': (lambda c: 12 * FP32_REL, 7.1e-7),                  # measured 1.77e-7, case parallel_mem_len_0_1_above
    'dkeys': (lambda c: 8 * FP32_REL, 5.0e-7),                   # measured 1.24e-7, case parallel_lds_mem_len_0_1_above
    'dv': (lambda c: _dot(c['Tm']) * FP32_REL, 4.7e-6),          # measured 1.15e-6, case Hd1024_P2 (one atomic per workgroup)
    'dbias': (lambda c: _dot(c['Tm']) * FP32_REL, 0.0),          # measured -2.4e-5: never positive
}


def _hip():
    from phones_las_amd import hip
    return hip, hip.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16_dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


def _padded(a, ld, fill):
    """[rows, w] -> [rows, ld] with `fill` behind the data."""
    out = np.full((a.shape[0], ld), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


class _Outs:
    """Sentinel-filled output buffers [rows, ld]; window(name) is [:, :width], outside_intact(name) says whether the rest (or, for
    a buffer the launch must not write at all, everything) still holds the sentinel."""

    def __init__(self):
        self.t, self.w = {}, {}

    def f32(self, name, rows, width, ld):
        self.t[name], self.w[name] = torch.full((rows, ld), SENT_F32, dtype=torch.float32, device='cuda'), width
        return self.t[name].data_ptr()

    def bf16(self, name, rows, width, ld):
        self.t[name], self.w[name] = _bf16_dev(np.full((rows, ld), SENT_BF16, dtype=np.uint16)), width
        return self.t[name].data_ptr()

    def fetch(self):
        self.a = {k: (v.cpu().numpy() if v.dtype == torch.float32 else _bits(v)) for k, v in self.t.items()}

    def window(self, name):
        return self.a[name][:, :self.w[name]]

    def outside_intact(self, name, whole=False):
        a = self.a[name] if whole else self.a[name][:, self.w[name]:]
        return bool((a == (SENT_F32 if a.dtype == np.float32 else SENT_BF16)).all())


class _Check:
    """Collects the figures of a case: every output is printed, the assertion comes at the end."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def close(self, name, got, ref, label=None):
        rel, eps = TOL[name]
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        scale = float(np.abs(ref).max()) if ref.size else 0.0
        fig = float((np.abs(got - ref) - rel(self.case) * np.abs(ref)).max() / (scale if scale > 0 else 1.0)) if ref.size else 0.0
        print('FIGURE %s %s %.4e' % (label or name, self.case['name'], fig))
        if not fig <= eps:
            self.bad.append('%s: figure %.4e > EPS %.4e' % (label or name, fig, eps))

    def true(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, '%s: %s' % (self.case['name'], '; '.join(self.bad))


# ---- forward ----------------------------------------------------------------------------------------------------------------
def _launch_fwd(case, inp, mode=None, query_bits=None):
    """-> (status, outs, keep-alive list).  Strides are wider than the data; tok_stride 3."""
    hip, lib = _hip()
    B, Hd, M, Tm = case['B'], case['Hd'], case['M'], case['Tm']
    mode = case['mode'] if mode is None else mode
    opt = case['optional']
    s, o, live = hip.DecStep(), _Outs(), []

    def dev(a, bf=False):
        live.append(_bf16_dev(a) if bf else _dev(a))
        return live[-1].data_ptr()

    s.B, s.Hd, s.M, s.Tm, s.attention, s.mode = B, Hd, M, Tm, case['att'], mode
    s.z, s.bias = dev(inp['z']), dev(inp['bias'])
    if case['tok']:
        ids = np.full(B * 3, -77, dtype=np.int32)
        ids[::3] = inp['tok_ids']
        s.tok_rows, s.tok_ids, s.tok_stride = dev(inp['tok_rows'], True), dev(ids), 3
    s.c_prev, s.ldcp = dev(_padded(inp['c_prev'], Hd + 8, np.float32(9.0))), Hd + 8
    if mode != R.ATTENTION_ONLY:
        s.gates_out, s.ldg = o.f32('gates', B, 4 * Hd, 4 * Hd + 8), 4 * Hd + 8
        s.c_out, s.ldco = o.f32('c', B, Hd, Hd + 16), Hd + 16
        s.h_out, s.ldh = o.bf16('h', B, Hd, Hd + 8), Hd + 8
    if opt:
        s.h_out2, s.ldh2 = o.bf16('h2', B, Hd, Hd + 24), Hd + 24
    s.keys, s.values, s.mem_len = dev(inp['keys'], True), dev(inp['values'], True), dev(inp['mem_len'])
    if 'wq' in inp:
        s.wq = dev(inp['wq'], True)
    if 'att_v' in inp:
        s.att_v = dev(inp['att_v'])
    if mode != R.CELL_ONLY:
        s.align_out, s.lda = o.f32('align', B, Tm, Tm + 3), Tm + 3
        s.ctx_out, s.ldc = o.bf16('ctx', B, M, M + 8), M + 8
        if opt:
            s.align_bf16 = o.bf16('align_bf16', B, Tm, Tm + 3)
            s.ctx_out2, s.ldc2 = o.bf16('ctx2', B, M, M + 16), M + 16
            if R.uses_wq(case['att']):
                s.pq_out, s.ldpq = o.f32('pq', B, Hd, Hd + 8), Hd + 8
            if case['norm'] != R.SOFTMAX:
                s.p_out, s.ldp = o.f32('p', B, Tm, Tm + 7), Tm + 7
    s.drop_keep, s.drop_seed, s.drop_stream = case['keep'], case['seed'], case['stream']
    s.step, s.feed_width, s.feed_plain, s.feed_stream0 = case['step'], case['feed_width'], case['feed_plain'], case['feed_stream0']
    if mode == R.ATTENTION_ONLY:
        q = inp['query'] if query_bits is None else query_bits
        s.query, s.ldq = dev(_padded(q, Hd + 8, np.uint16(0x7F80)), True), Hd + 8
    s.norm = case['norm']
    s.score_bias = dev(inp['score_bias'])
    if 'prev_align' in inp:
        s.prev_align, s.ldpa = dev(_padded(inp['prev_align'], Tm + 5, np.float32(5.0))), Tm + 5
    s.noise_scale, s.noise_seed, s.noise_stream = case['noise'], case['noise_seed'], case['noise_stream']
    rc = lib.las_decoder_step_fwd(C.byref(s), case['parts'], hip.stream())
    torch.cuda.synchronize()
    o.fetch()
    return rc, o


def _check_refused(case, rc, o, ck, needle):
    hip, lib = _hip()
    msg = lib.las_last_error().decode()
    print('REFUSAL %s status %d: %s' % (case['name'], rc, msg))
    ck.true(rc < 0, 'status %d is not an error' % rc)
    ck.true(needle in msg, 'the message %r does not name %s' % (msg, needle))
    for name in o.t:
        ck.true(o.outside_intact(name, whole=True), '%s was written by a refused launch' % name)


def _check_cell(case, inp, o, ck, ref):
    for name in ('gates', 'c'):
        ck.close(name, o.window(name), ref[name])
        ck.true(o.outside_intact(name), '%s written outside its window' % name)
    ck.close('h', bf2f(o.window('h')), ref['h'])
    ck.true(o.outside_intact('h'), 'h written outside its window')


def _check_attention(case, inp, o, ck, ref):
    """ref: fwd_reference from the kernel's own h_t (and Custom pq) bits."""
    B, M, Tm, att, norm = case['B'], case['M'], case['Tm'], case['att'], case['norm']
    lens = np.minimum(inp['mem_len'], Tm)
    off = np.arange(Tm)[None, :] >= lens[:, None]
    if 'pq' in o.t:
        ck.close('pq', o.window('pq'), R.rbf(ref['pq']) if att == R.CUSTOM else ref['pq'])
        ck.true(o.outside_intact('pq'), 'pq written outside its window')
    if 'p' in o.t:
        p = o.window('p')
        if norm == R.HARD:
            ck.true((p == ref['p']).all(), 'HARD p_out differs in %d places' % int((p != ref['p']).sum()))
        else:
            ck.close('p', p, ref['p'])
            # the score error behind it: d p = p (1 - p) d score (what the HARD margin has to exceed; see SCORE_ERR)
            pr = ref['p'][~off]
            print('FIGURE score_err %s %.4e' % (case['name'], float((np.abs(p[~off] - pr) / (pr * (1.0 - pr))).max()) if pr.size else 0.0))
        ck.true((p[off] == 0).all(), 'p_out not zero beyond mem_len')
        ck.true(o.outside_intact('p'), 'p written outside its window')
    al = o.window('align')
    ck.close('align', al, ref['align'])
    ck.true((al[off] == 0).all(), 'alignments not zero beyond mem_len')
    ck.true((al[lens == 0] == 0).all(), 'an empty memory must give all-zero alignments')
    ck.true(o.outside_intact('align'), 'align written outside its window')
    ctx = o.window('ctx')
    ck.close('ctx', bf2f(ctx), ref['ctx'])
    ck.true((ctx[lens == 0] == 0).all(), 'an empty memory must give a zero context')
    ck.true(o.outside_intact('ctx'), 'ctx written outside its window')
    if 'align_bf16' in o.t:
        ck.true((o.window('align_bf16') == f2bf(al)).all(), 'align_bf16 is not the rounding of align_out')
        ck.true(o.outside_intact('align_bf16'), 'align_bf16 written outside its window')
    if 'ctx2' in o.t:
        want, kept = R.feed_copy(ctx, case['keep'], case['feed_plain'], case['seed'], case['stream'], case['feed_stream0'], case['step'],
                                 case['feed_width'], case['tok'])
        ck.true((o.window('ctx2') == want).all(), 'ctx_out2 is not ctx_out through the feed mask (%d differ, %d dropped)'
                % (int((o.window('ctx2') != want).sum()), int((~kept).sum())))
        ck.true(o.outside_intact('ctx2'), 'ctx2 written outside its window')


@pytest.mark.parametrize('case', R.FWD_CASES, ids=lambda c: c['name'])
def test_decoder_step_fwd_vs_float64(case):
    inp = R.fwd_inputs(case)
    ck = _Check(case)
    rc, o = _launch_fwd(case, inp)
    if case['refuse']:
        _check_refused(case, rc, o, ck, str(case['Tm']))
        return ck.done()
    hip, _ = _hip()
    hip.check(rc)
    mode = case['mode']
    if mode == R.ATTENTION_ONLY:
        for name in ('gates', 'c', 'h'):
            assert name not in o.t
        if 'h2' in o.t:
            ck.true((o.window('h2') == inp['query']).all(), 'h_out2 is not the query')
        ref = R.fwd_reference(case, inp, pq_bits=f2bf(o.window('pq')) if case['att'] == R.CUSTOM and 'pq' in o.t else None)
    else:
        cell = R.fwd_reference(dict(case, mode=R.CELL_ONLY), inp)
        _check_cell(case, inp, o, ck, cell)
        if 'h2' in o.t:
            ck.true((o.window('h2') == o.window('h')).all(), 'h_out2 is not h_out')
        if mode == R.CELL_ONLY:
            return ck.done()
        ref = R.fwd_reference(case, inp, h_bits=o.window('h'),
                              pq_bits=f2bf(o.window('pq')) if case['att'] == R.CUSTOM and 'pq' in o.t else None)
    if 'h2' in o.t:
        ck.true(o.outside_intact('h2'), 'h2 written outside its window')
    _check_attention(case, inp, o, ck, ref)
    ck.done()


@pytest.mark.parametrize('case', R.SPLIT_CASES, ids=lambda c: c['name'])
def test_decoder_step_fused_equals_cell_then_attention(case):
    """LAS_DEC_FUSED against LAS_DEC_CELL_ONLY followed by LAS_DEC_ATTENTION_ONLY on its h_out: the same body, bit for bit."""
    hip, _ = _hip()
    inp = R.fwd_inputs(case)
    rc, fused = _launch_fwd(case, inp)
    hip.check(rc)
    rc, cell = _launch_fwd(case, inp, mode=R.CELL_ONLY)
    hip.check(rc)
    rc, attn = _launch_fwd(case, inp, mode=R.ATTENTION_ONLY, query_bits=cell.window('h'))
    hip.check(rc)
    for name in ('gates', 'c', 'h'):
        assert (fused.a[name] == cell.a[name]).all(), name
    assert (attn.window('h2') == cell.window('h')).all()
    for name in attn.t:
        if name != 'h2':
            assert (fused.a[name] == attn.a[name]).all(), name


# ---- backward ---------------------------------------------------------------------------------------------------------------
ACC0 = 0.625                  # what dbias_acc, dv_acc and dkeys_acc hold before an acc0 case's launch (times a pattern)


def _launch_bwd(case, inp):
    hip, lib = _hip()
    B, Hd, M, Tm, att, mode = case['B'], case['Hd'], case['M'], case['Tm'], case['att'], case['mode']
    opt = case['optional']
    s, o, live = hip.DecStepBwd(), _Outs(), []

    def dev(a, bf=False):
        live.append(_bf16_dev(a) if bf else _dev(a))
        return live[-1].data_ptr()

    def rows(a, ld, bf=False):
        return dev(_padded(a, ld, np.uint16(0x7F80) if bf else np.float32(11.0)), bf)

    s.B, s.Hd, s.M, s.Tm, s.attention, s.mode, s.norm = B, Hd, M, Tm, att, mode, case['norm']
    if inp['dctx_a'] is not None:
        s.dctx_a, s.ldda = rows(inp['dctx_a'], M + 8), M + 8
    if inp['dctx_b'] is not None:
        s.dctx_b, s.lddb = rows(inp['dctx_b'], M + 16), M + 16
    for k, f, ld in (('dh_rec', 'ldr', Hd + 8), ('dh_b', 'ldhb', Hd + 16), ('dh_c', 'ldhc', Hd + 24)):
        if inp[k] is not None:
            setattr(s, k, rows(inp[k], ld))
            setattr(s, f, ld)
    state = {}
    state['dc'] = _dev(inp['dc'])
    s.dc = state['dc'].data_ptr()
    s.gates, s.ldg = rows(inp['gates'], 4 * Hd + 8), 4 * Hd + 8
    s.c_new, s.ldcn = rows(inp['c_new'], Hd + 8), Hd + 8
    s.c_prev, s.ldcp = rows(inp['c_prev'], Hd + 16), Hd + 16
    s.align, s.lda = rows(inp['align'], Tm + 3), Tm + 3
    s.keys, s.values, s.mem_len = dev(inp['keys'], True), dev(inp['values'], True), dev(inp['mem_len'])
    if 'pq' in inp:
        s.pq, s.ldpq = rows(inp['pq'], Hd + 8), Hd + 8
        s.wq_t = dev(inp['wq_t'], True)
    if 'att_v' in inp:
        s.att_v = dev(inp['att_v'])
    s.dz, s.ldz = o.bf16('dz', B, 4 * Hd, 4 * Hd + 8), 4 * Hd + 8
    s.ds_out, s.ldso = o.bf16('ds', B, Tm, Tm + 5), Tm + 5
    if opt:
        s.dctx_save, s.ldds = o.bf16('dctx_save', B, M, M + 24), M + 24
        if R.uses_wq(att):
            s.dpq_out, s.lddpq = o.bf16('dpq', B, Hd, Hd + 8), Hd + 8
    if mode == R.ATTENTION_ONLY:
        s.dq_out, s.lddq = o.f32('dq', B, Hd, Hd + 8), Hd + 8
    r = np.random.default_rng(5)
    if R.additive(att):
        state['dkeys0'] = (ACC0 * r.standard_normal((B, Tm, Hd)) if case['acc0'] else np.zeros((B, Tm, Hd))).astype(np.float32)
        state['dv0'] = (ACC0 * r.standard_normal(Hd) if case['acc0'] else np.zeros(Hd)).astype(np.float32)
        state['dkeys'], state['dv'] = _dev(state['dkeys0']), _dev(state['dv0'])
        s.dkeys_acc, s.dv_acc = state['dkeys'].data_ptr(), state['dv'].data_ptr()
    s.drop_keep, s.drop_seed, s.drop_stream, s.step, s.feed_width = case['keep'], case['seed'], case['stream'], case['step'], case['feed_width']
    if case['norm'] != R.SOFTMAX:
        s.p, s.ldp = rows(inp['p'], Tm + 7), Tm + 7
        if 'prev_align' in inp:
            s.prev_align, s.ldpa = rows(inp['prev_align'], Tm + 5), Tm + 5
        state['carry'] = _dev(_padded(inp['carry'], Tm + 9, np.float32(SENT_F32)))
        s.dalign_carry, s.ldcarry = state['carry'].data_ptr(), Tm + 9
        state['dbias0'] = np.float32(ACC0 if case['acc0'] else 0.0)
        state['dbias'] = torch.full((1,), float(state['dbias0']), dtype=torch.float32, device='cuda')
        s.dbias_acc = state['dbias'].data_ptr()
    rc = lib.las_decoder_step_bwd(C.byref(s), hip.stream())
    torch.cuda.synchronize()
    o.fetch()
    return rc, o, {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in state.items()}


@pytest.mark.parametrize('case', R.BWD_CASES, ids=lambda c: c['name'])
def test_decoder_step_bwd_vs_float64(case):
    hip, _ = _hip()
    inp = R.bwd_inputs(case)
    ck = _Check(case)
    B, Hd, M, Tm, att, mode = case['B'], case['Hd'], case['M'], case['Tm'], case['att'], case['mode']
    rc, o, st = _launch_bwd(case, inp)
    if case['refuse']:
        _check_refused(case, rc, o, ck, 'las_decoder_step_bwd')
        ck.true((st['dc'] == inp['dc']).all(), 'dc was written by a refused launch')
        return ck.done()
    hip.check(rc)
    ref = R.bwd_reference(case, inp)
    lens = np.minimum(inp['mem_len'], Tm)
    off = np.arange(Tm)[None, :] >= lens[:, None]
    if mode != R.CELL_ONLY:
        if 'dctx_save' in o.t:
            ck.close('dctx_save', bf2f(o.window('dctx_save')), ref['dctx'])
            if 'kept' in ref and inp['dctx_a'] is None:
                ck.true((o.window('dctx_save')[~ref['kept']] == 0).all(), 'a dropped feed element has a gradient')
            ck.true(o.outside_intact('dctx_save'), 'dctx_save written outside its window')
        ds = o.window('ds')
        ck.close('ds', bf2f(ds), ref['ds'])
        ck.true((ds[off] == 0).all(), 'ds_out not zero beyond mem_len')
        ck.true(o.outside_intact('ds'), 'ds written outside its window')
        if 'dpq' in o.t:
            ck.close('dpq', bf2f(o.window('dpq')), ref['dpq'])
            if att == R.CUSTOM:
                ck.true((o.window('dpq')[inp['pq'] == 0] == 0).all(), 'relu gate: a gradient where the saved pq is 0')
            ck.true(o.outside_intact('dpq'), 'dpq written outside its window')
        if R.additive(att):
            ck.close('dkeys', st['dkeys'], st['dkeys0'].astype(np.float64) + ref['dkeys'])
            ck.true((st['dkeys'][off] == st['dkeys0'][off]).all(), 'dkeys_acc touched beyond mem_len')
            ck.close('dv', st['dv'], st['dv0'].astype(np.float64) + ref['dv'])
        if case['norm'] != R.SOFTMAX:
            ck.close('carry', st['carry'][:, :Tm], ref['carry'])
            ck.true((st['carry'][:, Tm:] == SENT_F32).all(), 'dalign_carry written outside its window')
            ck.close('dbias', st['dbias'], np.array([float(st['dbias0']) + ref['dbias']]))
    else:
        ck.true(o.outside_intact('ds', whole=True), 'CELL_ONLY wrote ds_out')
    if mode == R.ATTENTION_ONLY:
        ck.close('dq', o.window('dq'), ref['dq'])
        ck.true(o.outside_intact('dq'), 'dq written outside its window')
        ck.true(o.outside_intact('dz', whole=True), 'ATTENTION_ONLY wrote dz')
        ck.true((st['dc'] == inp['dc']).all(), 'ATTENTION_ONLY wrote dc')
    else:
        ck.close('dz', bf2f(o.window('dz')), ref['dz'])
        ck.true(o.outside_intact('dz'), 'dz written outside its window')
        ck.close('dc', st['dc'], ref['dc'])
    ck.done()
