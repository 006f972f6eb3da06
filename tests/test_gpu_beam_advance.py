"""las_beam_advance through the C-ABI: bit-equal to las_beam_step wherever that runs (the arithmetic is the same and the
selection is exact comparison, so there is no margin and no skipped utterance), against the float64 restatement beyond
las_beam_step's LDS limit, and the rest of the launch -- records, fed token, embedded feed, row gathers, ledger, freeze,
refusals -- against tests/beam_advance_restated.py.  Every buffer the launch may write starts at a sentinel.  The whole file runs
in a few seconds."""
import ctypes as C

import numpy as np
import pytest
import torch

import tests.beam_advance_restated as A
import tests.loss_heads_restated as R
import tests.test_gpu_loss_heads as T

pytestmark = pytest.mark.gpu

SENT = -7                     # int32 buffers before a launch
SENT_BYTE = 0xA5              # gather targets, gaps and neighbours before a launch


def _lib():
    from phones_las_amd import hip
    return hip, hip.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Launch:
    """The buffers of one search over B utterances: state, records [B K, U], fed tokens, ledger."""

    def __init__(self, log_probs, finished, lengths, K, V, eos, U=4, ledger=None):
        self.hip, self.lib = _lib()
        B = log_probs.shape[0]
        self.B, self.K, self.V, self.eos, self.U = B, K, V, eos, U
        self.lp, self.fin, self.ln = _dev(log_probs), _dev(finished), _dev(lengths)
        i32 = dict(dtype=torch.int32, device='cuda')
        self.word = torch.full((B * K, U), SENT, **i32)
        self.parent = torch.full((B * K, U), SENT, **i32)
        self.fed = torch.full((B * K, U + 1), SENT, **i32)
        led = ledger or A.new_ledger(B)
        self.ledger = _dev(np.concatenate([led['utt_done'], [led['remaining'], led['steps_done']]]).astype(np.int32))

    def args(self, logits_dev, ldl, t, fed=True, jobs=(), emb=None, x_next=None, ldx=0):
        hip = self.hip
        a = hip.BeamAdv()
        a.B, a.K, a.V, a.eos, a.t = self.B, self.K, self.V, self.eos, t
        a.logits, a.ldl = hip.addr(logits_dev), ldl
        a.log_probs, a.finished, a.lengths = hip.addr(self.lp), hip.addr(self.fin), hip.addr(self.ln)
        a.word_ids, a.parent_ids, a.ld_rec = hip.addr(self.word), hip.addr(self.parent), self.U
        if fed:
            a.next_token, a.ld_tok = hip.addr(self.fed), self.U + 1
        if x_next is not None:
            a.emb, a.ld_emb, a.emb_cols = hip.addr(emb), emb.stride(0), emb.shape[1]
            a.x_next, a.ldx = hip.addr(x_next), ldx
        a.utt_done, a.remaining, a.steps_done = hip.addr(self.ledger), hip.addr(self.ledger, self.B), hip.addr(self.ledger, self.B + 1)
        a.set_jobs(list(jobs))
        return a

    def run(self, logits, t=0, **kw):
        d_logits = _dev(logits)
        a = self.args(d_logits, logits.shape[-1], t, **kw)
        self.hip.check(self.lib.las_beam_advance(C.byref(a), self.hip.stream()))
        torch.cuda.synchronize()
        return self.outputs(t)

    def outputs(self, t):
        B, K = self.B, self.K
        return [self.word[:, t].reshape(B, K).cpu().numpy(), self.parent[:, t].reshape(B, K).cpu().numpy(), self.lp.cpu().numpy(),
                self.fin.cpu().numpy(), self.ln.cpu().numpy()]

    def led(self):
        v = self.ledger.cpu().numpy()
        return dict(utt_done=v[:self.B].tolist(), remaining=int(v[self.B]), steps_done=int(v[self.B + 1]))


def _advance(logits, log_probs, finished, lengths, K, V, eos):
    return Launch(log_probs, finished, lengths, K, V, eos).run(logits)


def _bit_equal(got, ref, tag):
    for g, r, name in zip(got, ref, ('word', 'parent', 'log_probs', 'finished', 'lengths')):
        if name == 'log_probs':
            g, r = g.view(np.uint32), r.view(np.uint32)
        assert np.array_equal(g, r), (tag, name, g, r)


# ---- 1. bit-equal to las_beam_step --------------------------------------------------------------------------------------------
def _finished_state():
    """The state of test_gpu_loss_heads.test_beam_step_finished_beams."""
    K, V, eos, ldl = 4, 70, 2, 72
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((2, K, ldl)) * 2).astype(np.float32)
    logits[..., V:] = np.nan
    logits[0, 1, eos] = 30.0
    log_probs = np.array([[-0.5, -1.25, -40.0, -50.0], [-3.0, -1.0, -4.0, -2.0]], dtype=np.float32)
    finished = np.array([[1, 0, 0, 1], [1, 1, 1, 1]], dtype=np.int32)
    lengths = np.array([[5, 6, 7, 8], [9, 3, 4, 6]], dtype=np.int32)
    return logits, log_probs, finished, lengths, K, V, eos


def _step_cases():
    cases = []
    for case in R.BEAM_RANDOM_CASES:
        name, B, K, V, ldl, eos, seed = case
        cases.append((name, lambda case=case: R.beam_random_inputs(case) + case[2:4] + (case[5],)))
    for K, V, ldl in [(4, 40, 40), (5, 100, 104), (8, 5, 8)]:
        cases.append(('first_step_K%d_V%d' % (K, V), lambda K=K, V=V, ldl=ldl: R.beam_first_step_inputs(8, K, V, ldl, 100 + K) + (K, V, 1)))
    cases.append(('ties', R.beam_tie_inputs))
    cases.append(('finished', _finished_state))
    return cases


@pytest.mark.parametrize('name,make', _step_cases(), ids=[c[0] for c in _step_cases()])
def test_bit_equal_to_beam_step(name, make):
    logits, log_probs, finished, lengths, K, V, eos = make()
    ref = T._run_beam(logits, log_probs, finished, lengths, K, V, eos)
    got = _advance(logits, log_probs, finished, lengths, K, V, eos)
    _bit_equal(got, ref, name)


# ---- 2. beyond the old LDS limit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', A.BEYOND_CASES, ids=lambda c: c[0])
def test_beyond_the_lds_limit_vs_float64(case):
    """K V words above las_beam_step's candidate buffer (asserted: it refuses).  Utterances count where both gaps of the
    restatement exceed R.BEAM_MARGIN; the seeds keep every one of them above it.  Log-probs within _beam_equal's bound
    (2^-23 F max(1, |ref|) + EPS_BEAM_LP, F = ceil(V / 64) + 9), and the largest error at most a tenth of the margin: the
    precondition of the margin rule, checked here and not assumed.
    The largest error is printed as a FIGURE line; not measured on an MI355X yet; no figures are claimed."""
    name, B, K, V, ldl, eos, seed = case
    hip, lib = _lib()
    assert R.beam_lds_bytes(K, V) > 64 * 1024
    logits, log_probs, finished, lengths = A.beyond_inputs(case)
    assert finished[-1].all() and 0.1 < finished[:-1].mean() < 0.45 and (ldl == V or np.isnan(logits[..., V:]).all())
    with pytest.raises(hip.LasError, match='LDS'):
        T._run_beam(logits, log_probs, finished, lengths, K, V, eos)
    under, pairs = A.beyond_skipped()
    print('beam utterances under the margin (skipped): %d of %d over the cases' % (under, pairs))
    assert under <= R.BEAM_SKIP_CAP * pairs
    ref = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
    rows = [b for b in range(B) if min(ref[5][b], ref[6][b]) > R.BEAM_MARGIN]
    got = _advance(logits, log_probs, finished, lengths, K, V, eos)
    fig, err = T._beam_equal(got, ref, rows, V, name)
    print('FIGURE beam_advance_log_probs %s largest error %.4e' % (name, err))
    assert fig <= T.EPS_BEAM_LP
    assert err <= R.BEAM_MARGIN / 10


# ---- 3. edge shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,V,ldl', [(1, 70, 72), (5, 100, 104), (8, 5, 8), (3, 64, 64), (3, 65, 72), (6, 129, 136)],
                         ids=['K1', 'K5_on_four_waves', 'V5_lt_K8', 'V64', 'V65', 'V129'])
def test_edge_shapes(K, V, ldl):
    """Against las_beam_step bit for bit, and against float64 where its gaps exceed the margin."""
    case = ('edge', 6, K, V, ldl, min(2, V - 1), 300 + 7 * K + V)
    logits, log_probs, finished, lengths = R.beam_random_inputs(case)
    eos = case[5]
    got = _advance(logits, log_probs, finished, lengths, K, V, eos)
    _bit_equal(got, T._run_beam(logits, log_probs, finished, lengths, K, V, eos), 'edge')
    ref = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
    rows = [b for b in range(6) if min(ref[5][b], ref[6][b]) > R.BEAM_MARGIN]
    assert len(rows) >= 4
    fig, err = T._beam_equal(got, ref, rows, V, 'edge_K%d_V%d' % (K, V))
    assert fig <= T.EPS_BEAM_LP and err <= R.BEAM_MARGIN / 10


def test_all_parents_at_minus_infinity_but_beam_0():
    """The first step of a search at K = 8 over V = 129: the finite winners descend from beam 0, in the float64 order."""
    K, V, ldl, eos = 8, 129, 136, 1
    logits, log_probs, finished, lengths = R.beam_first_step_inputs(4, K, V, ldl, 23)
    ref = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
    assert (np.minimum(ref[5], ref[6]) > R.BEAM_MARGIN).all()
    got = _advance(logits, log_probs, finished, lengths, K, V, eos)
    T._beam_equal(got, ref, range(4), V, 'first_step')
    assert (got[1] == 0).all() and (got[4] == 1).all()
    _bit_equal(got, T._run_beam(logits, log_probs, finished, lengths, K, V, eos), 'first_step')


# ---- 4. gather ----------------------------------------------------------------------------------------------------------------
def _rows(rng, nrows, width, stride, dtype, offset=0):
    """A buffer of nrows rows of `width` elements at `stride`, `offset` elements into an allocation: random payload, the gaps at
    the sentinel.  Returns (device buffer as bytes, the [nrows, width] device view, host copy of the payload)."""
    itemsize = np.dtype(dtype).itemsize
    buf = np.full((offset + nrows * stride) * itemsize, SENT_BYTE, dtype=np.uint8)
    view = buf.view(dtype)[offset:].reshape(nrows, stride)
    payload = rng.integers(0, 256, size=(nrows, width * itemsize), dtype=np.uint8).view(dtype)
    view[:, :width] = payload
    d = torch.from_numpy(buf).cuda()
    tdt = {np.uint16: torch.int16, np.float32: torch.float32, np.uint8: torch.uint8}[dtype]
    dview = d.view(tdt)[offset:].view(nrows, stride)[:, :width]
    return d, dview, buf.copy(), (offset, stride, width, itemsize)


def _expect(buf, geom, first, parents):
    """The host image after the gather of rows [first, first + K) by `parents` [1, K] (other rows untouched)."""
    offset, stride, width, itemsize = geom
    out = buf.copy()
    K = parents.shape[1]
    rows = out[offset * itemsize:].reshape(-1, stride * itemsize)
    old = buf[offset * itemsize:].reshape(-1, stride * itemsize)
    for j in range(K):
        rows[first + j, :width * itemsize] = old[first + parents[0, j], :width * itemsize]
    return out


def _middle_launch(make, specs):
    """B = 1 on the middle utterance of buffers that hold three: the outer utterances' rows must keep their bytes."""
    logits, log_probs, finished, lengths, K, V, eos = make()
    rng = np.random.default_rng(K)
    bufs = [_rows(rng, 3 * K, w, s, dt, off) for (w, s, dt, off) in specs]
    L = Launch(log_probs, finished, lengths, K, V, eos)
    got = L.run(logits, jobs=[dv[K:2 * K] for _, dv, _, _ in bufs])
    return got, bufs, K


SPECS3 = [(72, 80, np.uint16, 0), (100, 104, np.float32, 0), (808, 808, np.float32, 0)]


@pytest.mark.parametrize('make,want', [(A.parents_0021_inputs, [0, 0, 2, 1]), (A.parents_all_7_inputs, [7] * 8)], ids=['K4_0021', 'K8_all_7'])
def test_gather_three_jobs(make, want):
    """bf16 rows of 72 columns (144 bytes: no multiple of 16) at stride 80, fp32 rows of 100 at 104, fp32 rows of 808 at 808, in one
    launch: every row is its parent's old row bit for bit; gaps and the neighbours' rows keep their bytes."""
    got, bufs, K = _middle_launch(make, SPECS3)
    assert got[1].tolist() == [want]
    for d, _, host, geom in bufs:
        assert np.array_equal(d.cpu().numpy(), _expect(host, geom, K, got[1]))


def test_gather_no_jobs_and_sixteen_jobs():
    """0 jobs: a launch as in the last step.  16 jobs over B = 2 with different parents per utterance: odd element offsets (2-byte
    and 1-byte copies), rows wider than one staging tile (10 000 and 9 001 bytes at K = 4), rows of one element."""
    hip, lib = _lib()
    l0, p0, f0, n0, K, V, eos = A.parents_0021_inputs()
    logits = np.concatenate([l0, l0[:, ::-1]])                       # utterance 1: the beams' rows in reverse order
    log_probs = np.concatenate([p0, p0[:, ::-1]])
    finished, lengths = np.concatenate([f0, f0]), np.concatenate([n0, n0])
    ref = R.beam_step(logits, log_probs, finished, lengths, K, eos)
    assert ref[1].tolist() == [[0, 0, 2, 1], [3, 3, 1, 2]] and min(ref[5].min(), ref[6].min()) > R.BEAM_MARGIN
    got = Launch(log_probs, finished, lengths, K, V, eos).run(logits)
    assert np.array_equal(got[1], ref[1])
    rng = np.random.default_rng(16)
    specs = [(72, 80, np.uint16, 1), (72, 80, np.uint16, 0), (71, 75, np.uint16, 0), (33, 37, np.uint8, 3), (100, 104, np.float32, 0),
             (2500, 2504, np.float32, 0), (9001, 9001, np.uint8, 0), (3, 8, np.float32, 0), (1, 1, np.float32, 0), (1, 3, np.uint8, 0),
             (808, 808, np.float32, 0), (5000, 5001, np.uint16, 1), (64, 64, np.float32, 0), (65, 80, np.float32, 0),
             (256, 256, np.uint16, 0), (257, 300, np.uint16, 0)]
    assert len(specs) == hip.BEAM_MAX_JOBS
    bufs = [_rows(rng, 2 * K, w, s, dt, off) for (w, s, dt, off) in specs]
    got = Launch(log_probs, finished, lengths, K, V, eos).run(logits, jobs=[dv for _, dv, _, _ in bufs])
    assert np.array_equal(got[1], ref[1])
    for d, _, host, geom in bufs:
        want = _expect(_expect(host, geom, 0, ref[1][:1]), geom, K, ref[1][1:])
        assert np.array_equal(d.cpu().numpy(), want), geom


# ---- 5. feed ------------------------------------------------------------------------------------------------------------------
def test_feed_next_token_and_embedded_row():
    """Column t + 1 of the fed tokens and the embedded row follow the NEW beam order; the embedded row lands on top of a gathered
    row (the operand row is a gather target too), its other columns gathered.  NULL next_token: nothing written."""
    logits, log_probs, finished, lengths, K, V, eos = A.parents_0021_inputs()
    rng = np.random.default_rng(3)
    E, W = 8, 24
    emb = torch.from_numpy(rng.integers(0, 2 ** 15, size=(V, E), dtype=np.int16)).cuda().view(torch.bfloat16)
    d, dview, host, geom = _rows(rng, K, W, W + 4, np.uint16)
    L = Launch(log_probs, finished, lengths, K, V, eos)
    got = L.run(logits, t=1, jobs=[dview], emb=emb, x_next=dview, ldx=W + 4)
    word, parent = got[0], got[1]
    assert word.tolist() == [[0, 1, 0, 4]] and parent.tolist() == [[0, 0, 2, 1]]
    fed = L.fed.cpu().numpy()
    assert fed[:, 2].tolist() == [0, 1, 0, 4] and (np.delete(fed, 2, axis=1) == SENT).all()
    want = _expect(host, geom, 0, parent).view(np.uint16).reshape(K, W + 4)
    want[:, :E] = emb.view(torch.int16).cpu().numpy().view(np.uint16)[word[0]]
    assert np.array_equal(d.cpu().numpy().view(np.uint16).reshape(K, W + 4), want)
    assert (L.word[:, [0, 2, 3]] == SENT).all() and (L.parent[:, [0, 2, 3]] == SENT).all()
    L2 = Launch(log_probs, finished, lengths, K, V, eos)
    L2.run(logits, t=1, fed=False)
    assert (L2.fed == SENT).all()


# ---- 6. bookkeeping and freeze ------------------------------------------------------------------------------------------------
def test_ledger_over_three_steps_and_freeze():
    steps, K, V, eos = A.three_step_logits()
    B = 2
    state = (np.array([[0.0, -np.inf]] * B, dtype=np.float32), np.zeros((B, K), dtype=np.int32), np.zeros((B, K), dtype=np.int32))
    L = Launch(*state, K, V, eos)
    ref_state = tuple(s.copy() for s in state)
    rec = (np.full((B * K, 4), SENT, dtype=np.int32), np.full((B * K, 4), SENT, dtype=np.int32))
    led = A.new_ledger(B)
    want_led = [([0, 0], 2, 0), ([1, 0], 1, 0), ([1, 1], 0, 3)]
    for t, logits in enumerate(steps):
        lp, gap_out, gap_in = A.advance(logits, ref_state, K, eos, t, rec, led)
        assert min(gap_out.min(), gap_in.min()) > R.BEAM_MARGIN
        got = L.run(logits, t=t)
        assert np.array_equal(got[0].reshape(-1), rec[0][:, t]) and np.array_equal(got[1].reshape(-1), rec[1][:, t])
        assert np.array_equal(got[3], ref_state[1]) and np.array_equal(got[4], ref_state[2])
        assert np.allclose(got[2], lp, rtol=0, atol=1e-5)
        now = L.led()
        assert (now['utt_done'], now['remaining'], now['steps_done']) == want_led[t]
        assert (led['utt_done'].tolist(), led['remaining'], led['steps_done']) == want_led[t]
    # a fourth launch: remaining == 0, the search ended at step 3 -- nothing is written
    F = Launch(np.full((B, K), -3.0, dtype=np.float32), np.full((B, K), SENT, dtype=np.int32), np.full((B, K), SENT, dtype=np.int32),
               K, V, eos, ledger=dict(utt_done=np.array([1, 1]), remaining=0, steps_done=3))
    rng = np.random.default_rng(1)
    d, dview, host, geom = _rows(rng, B * K, 40, 48, np.float32)
    emb = torch.zeros(V, 8, dtype=torch.bfloat16, device='cuda')
    F.run(steps[1], t=3, jobs=[dview], emb=emb, x_next=dview.view(torch.bfloat16), ldx=96)
    assert (F.lp == -3.0).all() and (F.fin == SENT).all() and (F.ln == SENT).all()
    assert (F.word == SENT).all() and (F.parent == SENT).all() and (F.fed == SENT).all()
    assert np.array_equal(d.cpu().numpy(), host)
    assert F.led() == dict(utt_done=[1, 1], remaining=0, steps_done=3)
    assert A.advance(steps[1], ref_state, K, eos, 3, rec, led) == (None, None, None)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('what,words', [('K', ['beam_width 33', 'cap of 32']), ('null', ['null argument']), ('jobs', ['17 gather jobs', '16'])])
def test_refusals(what, words):
    """An error code and the message; nothing is launched (state and records stay at their sentinels)."""
    hip, lib = _lib()
    K = 33 if what == 'K' else 4
    V = 10
    L = Launch(np.full((1, K), -3.0, dtype=np.float32), np.full((1, K), SENT, dtype=np.int32), np.full((1, K), SENT, dtype=np.int32),
               K, V, 1)
    logits = torch.zeros(K, V, device='cuda')
    a = L.args(logits, V, 0)
    if what == 'null':
        a.parent_ids = None
    if what == 'jobs':
        a.njobs = hip.BEAM_MAX_JOBS + 1
    rc = lib.las_beam_advance(C.byref(a), hip.stream())
    msg = lib.las_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith('las_beam_advance') and all(w in msg for w in words), msg
    assert (L.lp == -3.0).all() and (L.fin == SENT).all() and (L.word == SENT).all() and (L.parent == SENT).all()
    assert L.led()['remaining'] == 1
    with pytest.raises(hip.LasError):
        hip.check(rc)
