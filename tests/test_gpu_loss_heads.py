"""las_seq_ce_loss, las_seq_sigmoid_loss, las_log_probs_loss, las_ctc_loss and las_beam_step through the C-ABI against the float64
restatements of tests/loss_heads_restated.py (which tests/test_loss_heads_host.py checks against torch, brute force and the
oracle).  The cases and the launch form or edge each one exists for are listed there (CE_CASES, SIGMOID_CASES, LOG_PROBS_CASES,
CTC_CASES, BEAM_RANDOM_CASES); for CTC the forms are read off the parameters by ctc_form() and printed.

Tolerances.  Losses: the project's own (CE / sigmoid 1e-5 relative, CTC per utterance rtol = atol = 1e-4).  Gradients element by
element: |kernel - ref| <= 2^-8 |ref| + EPS * scale for the bf16 ones (one bf16 rounding of the exact value, plus the fp32
fast-math error ahead of it), 2^-23 F |ref| + EPS * scale for the fp32 ones, F the number of roundings.  `scale` is the factor the
kernel multiplies an O(1) quantity (softmax - onehot, sigmoid - z) by -- grad_scale over the divisor -- so that one EPS serves every
case of an entry point; for CTC it also grows with the utterance's loss (_check_ctc_gradient says why).  Each EPS is four times the
largest figure measured over all cases of its entry point on an MI355X (LABNOTES.md); the test prints the figure of every case
before it asserts.  The whole file runs in about 3 s."""
import functools

import numpy as np
import pytest
import torch

import tests.loss_heads_restated as R

pytestmark = pytest.mark.gpu

BF16_REL = 2.0 ** -8
FP32_REL = 2.0 ** -23
# Each EPS = 4 x the largest (|kernel - ref| - rel |ref|) / scale measured over the cases of the entry point on an MI355X, and 0
# where that figure is negative for every element (the rounding term alone covers the kernel: a round-to-nearest errs by half
# of 2^-8, which leaves the fast-math error of a relative 1e-6 ample room).
EPS_CE = 0.0                  # measured -9.2e-14 (units of grad_scale / sum of lengths): never positive
EPS_SIGMOID = 1.3e-8          # measured 3.08e-9 (units of grad_scale / (nf sum of lengths)), case rows1209_gridstride
EPS_CTC = 9.2                 # measured 2.28 (units of grad_scale 2^-23 max(1, nll_b)), case S255_blocks (nll near 900)
EPS_LOG_PROBS_DX = 0.0        # measured -3.7e-9 (units of k): never positive
EPS_LOG_PROBS_LOSS = 0.0      # measured -9.0e-7 (relative to the loss; the errors themselves: 5e-8 .. 3.9e-7): never positive
EPS_BEAM_LP = 0.0             # measured -8.3e-7: never positive
BEAM_LP_ERR = 2.9e-6          # 4 x the largest |kernel - ref| of a log-prob measured (7.2e-7): the margin 1e-4 is 35 times this
SENT_BF16 = 0xC040            # -3.0: what the output buffers hold before a launch
SENT_F32 = -3.0


def _lib():
    from phones_las_amd import hip
    return hip, hip.lib()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bf16_dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def _bf16_sentinel(n):
    return _bf16_dev(np.full(n, SENT_BF16, dtype=np.uint16))


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _figure(tag, name, got, ref, rel, scale):
    """The largest |got - ref| - rel |ref| over the elements, in units of scale: printed, returned."""
    fig = float((np.abs(got - ref) - rel * np.abs(ref)).max() / scale) if ref.size else 0.0
    print('FIGURE %s %s %.4e' % (tag, name, fig))
    return fig


def _sum_loss_tol(ref, loss0, blocks):
    """The project's 1e-5 relative; onto a loss_out that held loss0 every workgroup's atomic rounds a sum of that size once more."""
    return 1e-5 * abs(ref) + (blocks * 2.0 ** -24 * (abs(loss0) + abs(ref)) if loss0 else 0.0)


# ---- sequence cross-entropy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CE_CASES, ids=lambda c: c[0])
def test_seq_ce_loss_vs_float64(case):
    """seq_ce_kernel: a wave per row, `blocks` capped at 256 workgroups of four rows.  dlogits: an active row's [0, V) is written,
    a masked row's [0, V) is zeroed, [V, ldd) of every row is never written (the sentinel survives)."""
    hip, lib = _lib()
    name, B, U, V, ldl, ldd, grad = case
    logits, targets, lens = R.ce_inputs(case)
    ref_loss, ref_d = R.seq_ce(logits[..., :V], targets, lens)
    grad_scale = 0.5
    loss0 = 0.75 if name == 'V200_ldl_ne_ldd' else 0.0          # the kernel adds to loss_out: the sum, not an overwrite
    d_logits, d_targets, d_lens = _dev(logits), _dev(targets), _dev(lens)
    loss = torch.full((1,), loss0, dtype=torch.float32, device='cuda')
    dl = _bf16_sentinel(B * U * ldd) if grad else None
    hip.check(lib.las_seq_ce_loss(hip.p(d_logits), ldl, hip.p(d_targets), hip.p(d_lens), B, U, V, grad_scale, hip.p(loss),
                                  hip.p(dl), ldd, hip.stream()))
    torch.cuda.synchronize()
    got = float(loss) - loss0
    print('FIGURE ce_loss_rel %s %.4e' % (name, abs(got - ref_loss) / abs(ref_loss)))
    assert abs(got - ref_loss) <= _sum_loss_tol(ref_loss, loss0, min(256, (B * U + 3) // 4))
    if not grad:
        return
    bits = _bits(dl).reshape(B, U, ldd)
    on = np.arange(U)[None, :] < np.minimum(lens, U)[:, None]
    assert (bits[..., V:] == SENT_BF16).all()
    assert (bits[~on][:, :V] == 0).all()
    total = float(np.minimum(lens, U).sum())
    fig = _figure('ce_dlogits', name, R.bf_bits2f(bits[on][:, :V]).astype(np.float64), grad_scale * ref_d[on], BF16_REL,
                  grad_scale / total)
    assert fig <= EPS_CE


# ---- sequence sigmoid loss --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.SIGMOID_CASES, ids=lambda c: c[0])
def test_seq_sigmoid_loss_vs_float64(case):
    """seq_sigmoid_kernel: the launch form of the CE kernel; the same columns written, zeroed and left alone, with nf for V."""
    hip, lib = _lib()
    name, B, U, nf, ldl, ldt, ldd, grad = case
    logits, targets, lens = R.sigmoid_inputs(case)
    ref_loss, ref_d = R.seq_sigmoid(logits[..., :nf], targets[..., :nf], lens)
    grad_scale = 0.5
    loss0 = 0.75 if name == 'nf150_ldt_ne_nf' else 0.0
    d_logits, d_lens = _dev(logits), _dev(lens)
    d_targets = _dev(targets).to(torch.bfloat16)
    loss = torch.full((1,), loss0, dtype=torch.float32, device='cuda')
    dl = _bf16_sentinel(B * U * ldd) if grad else None
    hip.check(lib.las_seq_sigmoid_loss(hip.p(d_logits), ldl, hip.p(d_targets), ldt, hip.p(d_lens), B, U, nf, grad_scale,
                                       hip.p(loss), hip.p(dl), ldd, hip.stream()))
    torch.cuda.synchronize()
    got = float(loss) - loss0
    print('FIGURE sigmoid_loss_rel %s %.4e' % (name, abs(got - ref_loss) / abs(ref_loss)))
    assert abs(got - ref_loss) <= _sum_loss_tol(ref_loss, loss0, min(256, (B * U + 3) // 4))
    if not grad:
        return
    bits = _bits(dl).reshape(B, U, ldd)
    on = np.arange(U)[None, :] < np.minimum(lens, U)[:, None]
    assert (bits[..., nf:] == SENT_BF16).all()
    assert (bits[~on][:, :nf] == 0).all()
    total = float(np.minimum(lens, U).sum())
    fig = _figure('sigmoid_dlogits', name, R.bf_bits2f(bits[on][:, :nf]).astype(np.float64), grad_scale * ref_d[on], BF16_REL,
                  grad_scale / (nf * total))
    assert fig <= EPS_SIGMOID


# ---- log-probs loss ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.LOG_PROBS_CASES, ids=lambda c: c[0])
def test_log_probs_loss_vs_float64(case):
    """log_probs_loss_kernel: an element per thread, the grid capped at 1024 workgroups.  dx: columns [0, 2 nf) of every row are
    written, [2 nf, ldd) never.  The inputs are bf16 on both sides and stay 1e-2 away from the kink of |e^a + e^b - 1| (asserted
    on the host), so the sign is the same on both sides.
    dx: k (sign e^a + [a > 0]) with k = weight grad_scale / (rows nf): the roundings of k (two), of the sum and of the product: F = 4;
    the fast exponential's error is what EPS covers, in units of k.
    loss: every thread adds its n / (256 blocks) terms one after the other, a wave adds its 64 in a tree of depth 6, and the
    4 blocks waves' atomics land on a sum that grows from nothing to the whole: F = terms + 6 + 4 blocks / 4 roundings of at most
    the whole sum -- and never more than the 1e-5 the project asks of its other summed losses."""
    hip, lib = _lib()
    name, rows, nf, ldx, ldd, grad = case
    bits = R.log_probs_inputs(case)
    ref_loss, ref_dx = R.log_probs_loss(R.bf_bits2f(bits)[:, :2 * nf], nf)
    weight, grad_scale, loss0 = 0.7, 0.5, (0.25 if name == 'wide_strides' else 0.0)
    x = _bf16_dev(bits)
    loss = torch.full((1,), loss0, dtype=torch.float32, device='cuda')
    dx = torch.full((rows * ldd,), SENT_F32, dtype=torch.float32, device='cuda') if grad else None
    hip.check(lib.las_log_probs_loss(hip.p(x), ldx, rows, nf, weight, grad_scale, hip.p(loss), hip.p(dx), ldd, hip.stream()))
    torch.cuda.synchronize()
    n = rows * nf
    blocks = min(1024, (n + 255) // 256)
    F = -(-n // (256 * blocks)) + 6 + blocks
    rel = min(1e-5, FP32_REL * F)
    got, ref = float(loss) - loss0, weight * ref_loss
    fig = (abs(got - ref) - rel * abs(ref) - (4 * blocks * 2.0 ** -24 * (loss0 + ref) if loss0 else 0.0)) / abs(ref)
    print('FIGURE log_probs_loss %s %.4e (rel err %.4e, allowed %.4e)' % (name, fig, abs(got - ref) / abs(ref), rel))
    assert fig <= EPS_LOG_PROBS_LOSS
    if not grad:
        return
    out = dx.cpu().numpy().reshape(rows, ldd)
    assert (out[:, 2 * nf:] == SENT_F32).all()
    k = weight * grad_scale / n
    fig = _figure('log_probs_dx', name, out[:, :2 * nf].astype(np.float64), weight * grad_scale * ref_dx, 4 * FP32_REL, k)
    assert fig <= EPS_LOG_PROBS_DX


# ---- CTC --------------------------------------------------------------------------------------------------------------------
def _run_ctc(logits, ldl, labels, label_len, logit_len, C, blank, loss_scale, grad_scale, loss0=0.0, want_per=True, want_grad=True):
    hip, lib = _lib()
    B, T, _ = logits.shape
    U = labels.shape[1]
    ws = torch.empty(lib.las_ctc_workspace_bytes(B, T, ldl, U), dtype=torch.uint8, device='cuda')
    loss = torch.full((1,), loss0, dtype=torch.float32, device='cuda')
    per = torch.full((B,), SENT_F32, dtype=torch.float32, device='cuda') if want_per else None
    dl = _bf16_sentinel(B * T * ldl) if want_grad else None
    d = [_dev(logits), _dev(labels), _dev(label_len), _dev(logit_len)]                 # keep the device tensors alive
    hip.check(lib.las_ctc_loss(hip.p(d[0]), ldl, hip.p(d[1]), U, hip.p(d[2]), hip.p(d[3]), B, T, C, U, blank, loss_scale, grad_scale,
                               hip.p(ws), hip.p(loss), hip.p(per), hip.p(dl), hip.stream()))
    torch.cuda.synchronize()
    return (float(loss) - loss0, per.cpu().numpy() if want_per else None,
            _bits(dl).reshape(B, T, ldl) if want_grad else None)


def _check_ctc_gradient(name, bits, ref_d, ref_nll, logit_len, C, grad_scale, rows=None):
    """The whole of dlogits is written: frames from min(logit_len, T) on and the pad columns [C, ldl) are zero, everything else
    within one bf16 rounding + EPS_CTC * scale of the restatement.  scale = grad_scale 2^-23 max(1, nll_b): the occupancy term is
    exp(alpha + beta - log y - log p) with fp32 operands of the size of log p = -nll_b, each of which carries an absolute error
    of that size times 2^-24, so the error grows with the utterance's loss (a long utterance: nll near 900) and EPS_CTC counts
    roundings of such a value."""
    B, T, ldl = bits.shape
    rows = range(B) if rows is None else rows
    figs = []
    for b in rows:
        Tb = min(int(logit_len[b]), T)
        assert (bits[b, :, C:] == 0).all() and (bits[b, max(Tb, 0):] == 0).all(), b
        got = R.bf_bits2f(bits[b, :Tb, :C]).astype(np.float64)
        scale = grad_scale * FP32_REL * max(1.0, abs(float(ref_nll[b])))
        figs.append((np.abs(got - grad_scale * ref_d[b, :Tb]) - BF16_REL * np.abs(grad_scale * ref_d[b, :Tb])).max() / scale
                    if Tb > 0 else 0.0)
    fig = float(max(figs))
    print('FIGURE ctc_dlogits %s %.4e' % (name, fig))
    return fig


@pytest.mark.parametrize('case', R.CTC_CASES, ids=lambda c: c[0])
def test_ctc_loss_vs_float64(case):
    """ctc_kernel, one workgroup per utterance; the forms of each case (log-softmax by C, recursion by S = 2 L + 1, class lists by
    S + C <= 2 Sp, the staging area by the LDS left) are printed from its parameters.  loss_out is held against the kernel's own
    per-utterance losses (B fp32 adds of loss_scale nll_b), and those against float64."""
    name, B, T, C, ldl, U, blank, kind = case
    logits, labels, label_len, logit_len = R.ctc_inputs(case)
    print('FORMS %s %s' % (name, R.ctc_form(T, C, U, int(np.minimum(label_len, U).max()))))
    assert R.ctc_lds_plan(T, C, U)[0] <= R.CTC_LDS_BYTES                       # it fits: nothing here relies on a rejected launch
    ref, ref_d = R.ctc(logits[..., :C], labels, label_len, logit_len, blank)
    assert np.isfinite(ref).all()
    loss_scale, grad_scale, loss0 = 0.5, 0.25, (2.0 if name == 'C65' else 0.0)
    loss, per, bits = _run_ctc(logits, ldl, labels, label_len, logit_len, C, blank, loss_scale, grad_scale, loss0)
    print('FIGURE ctc_per_example_abs %s %.4e' % (name, np.abs(per - ref).max()))
    assert np.allclose(per.astype(np.float64), ref, rtol=1e-4, atol=1e-4)
    own = loss_scale * float(per.astype(np.float64).sum())
    assert abs(loss - own) <= (B + 1) * FP32_REL * (loss0 + loss_scale * float(np.abs(per).sum()))
    assert _check_ctc_gradient(name, bits, ref_d, ref, logit_len, C, grad_scale) <= EPS_CTC


def test_ctc_optional_outputs_may_be_null():
    """dlogits == NULL (EVAL) and per_example == NULL: loss_out alone, bit-equal to the full call's."""
    case = next(c for c in R.CTC_CASES if c[0] == 'C100_two_per_lane')
    name, B, T, C, ldl, U, blank, kind = case
    logits, labels, label_len, logit_len = R.ctc_inputs(case)
    ref, _ = R.ctc(logits[..., :C], labels, label_len, logit_len, blank)
    full, per, bits = _run_ctc(logits, ldl, labels, label_len, logit_len, C, blank, 0.5, 0.25)
    bare, _, _ = _run_ctc(logits, ldl, labels, label_len, logit_len, C, blank, 0.5, 0.25, want_per=False, want_grad=False)
    no_per, _, bits2 = _run_ctc(logits, ldl, labels, label_len, logit_len, C, blank, 0.5, 0.25, want_per=False)
    assert abs(bare - 0.5 * ref.sum()) <= 0.5 * (1e-4 * np.abs(ref).sum() + 1e-4 * B)
    assert abs(bare - full) <= (B + 1) * FP32_REL * abs(full) and abs(no_per - full) <= (B + 1) * FP32_REL * abs(full)     # (the atomics' order)
    assert np.array_equal(bits, bits2)


def test_ctc_infeasible_utterance_beside_feasible_ones():
    """label_len > logit_len for one utterance.  The restatement gives +inf; the kernel works with -1e30 in place of -inf, so its
    loss is at least 1e29 and its gradient free of NaN and inf (every state's alpha + beta stays at or below -1e30, so the
    occupancy term is dropped and softmax remains).  The other utterances (a workgroup each, nothing shared but the loss_out
    atomic) are bit-equal to the same batch without it, where loss_out is compared."""
    case = next(c for c in R.CTC_CASES if c[0] == 'C100_two_per_lane')
    name, B, T, C, ldl, U, blank, kind = case
    logits, labels, label_len, logit_len = R.ctc_inputs(case)
    bad = 2
    label_len[bad], logit_len[bad] = 18, 10
    ref, ref_d = R.ctc(logits[..., :C], labels, label_len, logit_len, blank)
    assert np.isposinf(ref[bad]) and np.isfinite(np.delete(ref, bad)).all()
    _, per, bits = _run_ctc(logits, ldl, labels, label_len, logit_len, C, blank, 0.5, 0.25)
    assert per[bad] >= 1e29 and np.isfinite(per[bad])
    assert np.isfinite(R.bf_bits2f(bits[bad])).all()
    keep = [b for b in range(B) if b != bad]
    loss2, per2, bits2 = _run_ctc(logits[keep], ldl, labels[keep], label_len[keep], logit_len[keep], C, blank, 0.5, 0.25)
    assert np.array_equal(per[keep].view(np.uint32), per2.view(np.uint32))
    assert np.array_equal(bits[keep], bits2)
    assert np.allclose(per2.astype(np.float64), ref[keep], rtol=1e-4, atol=1e-4)
    assert abs(loss2 - 0.5 * float(per2.astype(np.float64).sum())) <= B * FP32_REL * 0.5 * float(np.abs(per2).sum())
    assert _check_ctc_gradient('infeasible_neighbours', bits, ref_d, ref, logit_len, C, 0.25, rows=keep) <= EPS_CTC


def test_ctc_utterance_without_frames_contributes_nothing():
    """logit_len == 0 with labels: there is no path either, but the kernel leaves such an utterance out (loss 0, gradient 0)
    instead of charging 1e30 for it -- an encoder never returns zero frames; pinned here so that a change shows."""
    case = R.CTC_CASES[0]
    name, B, T, C, ldl, U, blank, kind = case
    logits, labels, label_len, logit_len = R.ctc_inputs(case)
    label_len[3] = 2
    assert logit_len[3] == 0
    ref, ref_d = R.ctc(logits[..., :C], labels, label_len, logit_len, blank)
    assert np.isposinf(ref[3])
    _, per, bits = _run_ctc(logits, ldl, labels, label_len, logit_len, C, blank, 0.5, 0.25)
    assert per[3] == 0.0 and (bits[3] == 0).all()
    keep = [b for b in range(B) if b != 3]
    assert np.allclose(per[keep].astype(np.float64), ref[keep], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize('C,U,words', [(21000, 6, ('C=21000', 'U=6', str(R.CTC_LDS_BYTES))), (30, 2729, ('2729',))],
                         ids=['classes_beyond_the_lds', 'labels_beyond_the_lds'])
def test_ctc_refuses_what_cannot_fit(C, U, words):
    """8 C + 8 bytes of class counters beyond the 160 KiB - 64 of a launch, or 12 (2 U + 4) bytes of columns beyond 64 KiB: an error
    code and a message that names the numbers, decided on the host -- nothing is launched, the outputs keep their sentinels."""
    hip, lib = _lib()
    B, T = 1, 4
    assert R.ctc_lds_plan(T, C, U)[0] > R.CTC_LDS_BYTES or 12 * (2 * U + 4) > 64 * 1024
    logits = torch.zeros(B * T * C, device='cuda')
    labels = torch.ones(B * U, dtype=torch.int32, device='cuda')
    lens = torch.ones(B, dtype=torch.int32, device='cuda')
    ws = torch.empty(lib.las_ctc_workspace_bytes(B, T, C, U), dtype=torch.uint8, device='cuda')
    loss = torch.full((1,), SENT_F32, device='cuda')
    per = torch.full((B,), SENT_F32, device='cuda')
    dl = _bf16_sentinel(B * T * C)
    rc = lib.las_ctc_loss(hip.p(logits), C, hip.p(labels), U, hip.p(lens), hip.p(lens), B, T, C, U, 0, 1.0, 1.0, hip.p(ws),
                          hip.p(loss), hip.p(per), hip.p(dl), hip.stream())
    msg = lib.las_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and msg.startswith('las_ctc_loss') and all(w in msg for w in words), msg
    assert float(loss) == SENT_F32 and float(per[0]) == SENT_F32 and (_bits(dl) == SENT_BF16).all()
    with pytest.raises(hip.LasError):
        hip.check(rc)


# ---- beam step --------------------------------------------------------------------------------------------------------------
def _run_beam(logits, log_probs, finished, lengths, K, V, eos):
    hip, lib = _lib()
    B, _, ldl = logits.shape
    d_logits = _dev(logits)
    lp, fin, ln = _dev(log_probs), _dev(finished), _dev(lengths)
    word = torch.full((B, K), -7, dtype=torch.int32, device='cuda')
    parent = torch.full((B, K), -7, dtype=torch.int32, device='cuda')
    hip.check(lib.las_beam_step(hip.p(d_logits), ldl, hip.p(lp), hip.p(fin), hip.p(ln), hip.p(word), hip.p(parent), B, K, V, eos,
                                hip.stream()))
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (word, parent, lp, fin, ln)]


def _beam_equal(got, ref, rows, V, tag):
    """Integer outputs exactly; log_probs within 2^-23 F max(1, |ref|) + EPS_BEAM_LP, F = ceil(V / 64) + 6 + 3: a lane's terms of the
    row sum, the tree over the lanes, and the roundings of the logarithm, of x - lse and of the sum with the previous log-prob."""
    word, parent, lp, fin, ln = got
    rw, rp, rlp, rfin, rln = ref[:5]
    for b in rows:
        assert np.array_equal(word[b], rw[b]) and np.array_equal(parent[b], rp[b]), (tag, b, word[b], rw[b], parent[b], rp[b])
        assert np.array_equal(fin[b], rfin[b]) and np.array_equal(ln[b], rln[b]), (tag, b)
    rows = list(rows)
    finite = np.isfinite(rlp[rows])
    assert np.array_equal(lp[rows][~finite].astype(np.float64), rlp[rows][~finite])
    F = -(-V // 64) + 6 + 3
    err = np.abs(lp[rows][finite].astype(np.float64) - rlp[rows][finite])
    fig = float((err - FP32_REL * F * np.maximum(1.0, np.abs(rlp[rows][finite]))).max()) if err.size else 0.0
    print('FIGURE beam_log_probs %s excess %.4e, largest error %.4e' % (tag, fig, err.max() if err.size else 0.0))
    return fig, float(err.max()) if err.size else 0.0


@functools.lru_cache(None)
def _beam_skipped_share():
    """(pairs under the margin, all pairs) over the random cases: the restatement's gaps alone decide."""
    under = pairs = 0
    for case in R.BEAM_RANDOM_CASES:
        name, B, K, V, ldl, eos, seed = case
        logits, log_probs, finished, lengths = R.beam_random_inputs(case)
        *_, gap_out, gap_in = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
        under += int((np.minimum(gap_out, gap_in) <= R.BEAM_MARGIN).sum())
        pairs += B
    return under, pairs


@pytest.mark.parametrize('case', R.BEAM_RANDOM_CASES, ids=lambda c: c[0])
def test_beam_step_random_states_vs_float64(case):
    """(a) a state in the middle of a search (a quarter of the beams finished), (g) the largest K V the LDS check admits, (h) NaN
    in the pad columns of the logits.  An utterance counts where both of the restatement's gaps exceed BEAM_MARGIN = 1e-4: float64
    and fp32 agree on the order there, the kernel's log-probs being within BEAM_LP_ERR (measured, at least ten times smaller)."""
    name, B, K, V, ldl, eos, seed = case
    assert 10 * BEAM_LP_ERR <= R.BEAM_MARGIN
    under, pairs = _beam_skipped_share()
    print('beam utterances under the margin (skipped): %d of %d over all cases' % (under, pairs))
    assert under <= R.BEAM_SKIP_CAP * pairs
    logits, log_probs, finished, lengths = R.beam_random_inputs(case)
    ref = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
    rows = [b for b in range(B) if min(ref[5][b], ref[6][b]) > R.BEAM_MARGIN]
    got = _run_beam(logits, log_probs, finished, lengths, K, V, eos)
    fig, err = _beam_equal(got, ref, rows, V, name)
    assert fig <= EPS_BEAM_LP and err <= BEAM_LP_ERR
    # (d) in the kernel's own outputs: a winner whose parent had finished is eos with the log-prob and the length unchanged
    word, parent, lp, fin, ln = got
    for b in rows:
        for j in range(K):
            k = parent[b, j]
            if finished[b, k]:
                assert word[b, j] == eos and fin[b, j] == 1 and ln[b, j] == lengths[b, k]
                assert lp[b, j].view(np.uint32) == log_probs[b, k].view(np.uint32)
            else:
                assert ln[b, j] == lengths[b, k] + 1 and fin[b, j] == int(word[b, j] == eos)


@pytest.mark.parametrize('K,V,ldl', [(4, 40, 40), (5, 100, 104), (8, 5, 8)], ids=['K4_V40', 'K5_V100', 'K8_V5_fewer_candidates_than_K'])
def test_beam_step_first_step(K, V, ldl):
    """(b) log_probs = [0, -inf, ...]: every finite candidate descends from beam 0.  (f) V = 5 < K = 8: after the five finite
    candidates the -inf ones follow in index order (beam 1, classes 0, 1, 2) -- ties at -inf are exact, nothing is skipped."""
    B, eos = 8, 1
    logits, log_probs, finished, lengths = R.beam_first_step_inputs(B, K, V, ldl, 100 + K)
    ref = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
    if K <= V:
        close = np.minimum(ref[5], ref[6])
    else:                                         # the finite ones are beam 0's whole row: their order needs distinct values only
        close = np.diff(np.sort(ref[2][:, :V], axis=1), axis=1).min(1)
    assert (close > R.BEAM_MARGIN).all()          # (the seeds are chosen so: no utterance of these cases is left out)
    rows = range(B)
    got = _run_beam(logits, log_probs, finished, lengths, K, V, eos)
    fig, err = _beam_equal(got, ref, rows, V, 'first_step_K%d_V%d' % (K, V))
    assert fig <= EPS_BEAM_LP and err <= BEAM_LP_ERR
    word, parent, lp, fin, ln = got
    n = min(K, V)
    assert (parent[:, :n] == 0).all() and (ln == 1).all()
    if K > V:
        assert (parent[:, V:] == 1).all() and (word[:, V:] == np.arange(K - V)[None]).all() and np.isneginf(lp[:, V:]).all()


def test_beam_step_exact_ties_go_to_the_lower_index():
    """(c) bit-identical logit rows with equal log-probs, duplicated values inside a row: equal inputs go through the same
    arithmetic, so the ties are exact in fp32 as in float64, and the lower flat index k V + v wins.  Never skipped."""
    logits, log_probs, finished, lengths, K, V, eos = R.beam_tie_inputs()
    ref = R.beam_step(logits, log_probs, finished, lengths, K, eos)
    got = _run_beam(logits, log_probs, finished, lengths, K, V, eos)
    fig, err = _beam_equal(got, ref, range(logits.shape[0]), V, 'ties')
    assert fig <= EPS_BEAM_LP and err <= BEAM_LP_ERR
    word, parent, lp = got[:3]
    assert list(zip(parent[2], word[2])) == [(0, 3), (0, 8), (1, 3), (1, 8)]
    assert list(zip(parent[3], word[3])) == [(1, 4), (1, 10), (3, 4), (3, 10)]
    assert len(set(lp[2].view(np.uint32))) == 1 and len(set(lp[3].view(np.uint32))) == 1      # ties in fp32 too


def test_beam_step_finished_beams():
    """(d) a finished beam offers eos alone, log-prob unchanged, length frozen; a live beam that takes eos finishes one longer.
    (e) every beam finished: the beams in the order of their log-probs, everything else as it was."""
    K, V, eos, ldl = 4, 70, 2, 72
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((2, K, ldl)) * 2).astype(np.float32)
    logits[..., V:] = np.nan
    logits[0, 1, eos] = 30.0                                         # the live beam 1 takes eos (step log-prob ~ 0)
    log_probs = np.array([[-0.5, -1.25, -40.0, -50.0], [-3.0, -1.0, -4.0, -2.0]], dtype=np.float32)
    finished = np.array([[1, 0, 0, 1], [1, 1, 1, 1]], dtype=np.int32)
    lengths = np.array([[5, 6, 7, 8], [9, 3, 4, 6]], dtype=np.int32)
    ref = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
    assert min(ref[5].min(), ref[6].min()) > R.BEAM_MARGIN
    got = _run_beam(logits, log_probs, finished, lengths, K, V, eos)
    fig, err = _beam_equal(got, ref, range(2), V, 'finished')
    assert fig <= EPS_BEAM_LP and err <= BEAM_LP_ERR
    word, parent, lp, fin, ln = got
    assert (parent[0, 0], word[0, 0], fin[0, 0], ln[0, 0]) == (0, eos, 1, 5) and lp[0, 0] == np.float32(-0.5)
    assert (parent[0, 1], word[0, 1], fin[0, 1], ln[0, 1]) == (1, eos, 1, 7)
    assert parent[1].tolist() == [1, 3, 0, 2] and (word[1] == eos).all() and (fin[1] == 1).all()
    assert ln[1].tolist() == [3, 6, 9, 4] and lp[1].tolist() == [-1.0, -2.0, -3.0, -4.0]


def test_beam_step_refuses_beyond_the_lds():
    """(g) one class beyond the largest case: an error code and the message, no launch (the outputs and the state stay as they were)."""
    hip, lib = _lib()
    K, V = R.BEAM_REFUSED
    assert R.beam_lds_bytes(K, V) > 64 * 1024 >= R.beam_lds_bytes(K, V - 1)
    logits = torch.zeros(K * V, device='cuda')
    lp = torch.full((K,), SENT_F32, device='cuda')
    ints = [torch.full((K,), -7, dtype=torch.int32, device='cuda') for _ in range(4)]
    rc = lib.las_beam_step(hip.p(logits), V, hip.p(lp), hip.p(ints[0]), hip.p(ints[1]), hip.p(ints[2]), hip.p(ints[3]), 1, K, V, 1,
                           hip.stream())
    msg = lib.las_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and 'las_beam_step' in msg and str(K * V) in msg and 'LDS' in msg, msg
    assert (lp == SENT_F32).all() and all((t == -7).all() for t in ints)
