"""tests/loss_heads_restated.py against independent implementations (torch in float64, brute force, the oracle's beam search), and the
conditions under which tests/test_gpu_loss_heads.py compares the kernels with it: the share of beam cases under the margin, the
exact ties, the distance from the kink of the log-probs loss, the LDS arithmetic of the CTC cases.  No GPU."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.loss_heads_restated as R

D = torch.float64


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# ---- CE / sigmoid / log-probs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CE_CASES[:5], ids=lambda c: c[0])
def test_seq_ce_vs_torch_cross_entropy(case):
    _, B, U, V, *_ = case
    logits, targets, lens = R.ce_inputs(case)
    loss, d = R.seq_ce(logits[..., :V], targets, lens)
    x = torch.from_numpy(logits[..., :V].astype(np.float64)).requires_grad_(True)
    ce = F.cross_entropy(x.reshape(B * U, V), torch.from_numpy(targets.astype(np.int64)).reshape(-1), reduction='none').view(B, U)
    n = torch.clamp(torch.from_numpy(lens.astype(np.int64)), max=U)
    w = (torch.arange(U)[None] < n[:, None]).to(D)
    ref = (ce * w).sum() / (n.sum() + 1e-12)
    ref.backward()
    assert _close(loss, ref.item()) and _close(d, x.grad.numpy())
    assert (d[np.arange(U)[None] >= np.minimum(lens, U)[:, None]] == 0).all()
    assert lens.min() == 0 and lens.max() > U and (lens == U).any()           # the edges the kernel test relies on


def test_seq_ce_all_lengths_zero_is_zero():
    loss, d = R.seq_ce(np.ones((2, 3, 4)), np.zeros((2, 3), dtype=int), [0, 0])
    assert loss == 0.0 and not d.any()


@pytest.mark.parametrize('case', R.SIGMOID_CASES[:5], ids=lambda c: c[0])
def test_seq_sigmoid_vs_torch_bce_with_logits(case):
    _, B, U, nf, *_ = case
    logits, targets, lens = R.sigmoid_inputs(case)
    loss, d = R.seq_sigmoid(logits[..., :nf], targets[..., :nf], lens)
    x = torch.from_numpy(logits[..., :nf].astype(np.float64)).requires_grad_(True)
    bce = F.binary_cross_entropy_with_logits(x, torch.from_numpy(targets[..., :nf].astype(np.float64)), reduction='none').mean(-1)
    n = torch.clamp(torch.from_numpy(lens.astype(np.int64)), max=U)
    w = (torch.arange(U)[None] < n[:, None]).to(D)
    ref = (bce * w).sum() / (n.sum() + 1e-12)
    ref.backward()
    assert _close(loss, ref.item()) and _close(d, x.grad.numpy())
    assert set(np.unique(targets[..., :nf])) == {0.0, 1.0}


@pytest.mark.parametrize('case', R.LOG_PROBS_CASES, ids=lambda c: c[0])
def test_log_probs_loss_vs_autograd_and_kink_distance(case):
    _, rows, nf, ldx, *_ = case
    x = R.bf_bits2f(R.log_probs_inputs(case))[:, :2 * nf]
    loss, dx = R.log_probs_loss(x, nf)
    t = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    a, b = t[:, :nf], t[:, nf:]
    ref = ((a.exp() + b.exp() - 1).abs() + torch.relu(a) + torch.relu(b)).mean()
    ref.backward()
    assert _close(loss, ref.item()) and _close(dx, t.grad.numpy())
    # the conditions of the kernel test: every element away from the kink, every sign case present, inputs exact in bf16
    assert R.log_probs_kink_distance(x, nf).min() > R.LOG_PROBS_KINK_MIN
    v = np.exp(x[:, :nf].astype(np.float64)) + np.exp(x[:, nf:].astype(np.float64)) - 1
    assert (v > 0).any() and (v < 0).any() and (x[:, :nf] > 0).any() and (x[:, nf:] > 0).any()
    assert np.array_equal(R.f2bf_bits(x), R.log_probs_inputs(case)[:, :2 * nf])


def test_bf16_helpers_round_to_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -2.5, 3.0e-5], dtype=np.float32)      # 1 + 2^-8: a tie, to even (down); 1 + 3 * 2^-8: up
    got = R.bf_bits2f(R.f2bf_bits(x))
    assert np.array_equal(got, torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert got[1] == 1.0 and got[2] == np.float32(1.015625)


# ---- CTC --------------------------------------------------------------------------------------------------------------------
def _torch_ctc(logits, labels, label_len, logit_len, blank):
    B, T, C = logits.shape
    U = labels.shape[1]
    x = torch.from_numpy(logits.astype(np.float64)).requires_grad_(True)
    ll = torch.clamp(torch.from_numpy(label_len.astype(np.int64)), max=U)
    tl = torch.clamp(torch.from_numpy(logit_len.astype(np.int64)), max=T)
    nll = F.ctc_loss(torch.log_softmax(x, -1).transpose(0, 1), torch.from_numpy(labels.astype(np.int64)), tl, ll, blank=blank,
                     reduction='none')
    finite = torch.isfinite(nll)
    nll[finite].sum().backward()
    return nll.detach().numpy(), x.grad.numpy()


CTC_HOST = [c for c in R.CTC_CASES if c[0] in ('C64', 'C65', 'C100_two_per_lane', 'C150_no_lists', 'same_label_long_list',
                                               'same_label_blank5', 'blank_last', 'S257_blocks', 'staging_cut')]


@pytest.mark.parametrize('case', CTC_HOST, ids=lambda c: c[0])
def test_ctc_vs_torch_ctc_loss(case):
    _, B, T, C, ldl, U, blank, kind = case
    logits, labels, label_len, logit_len = R.ctc_inputs(case)
    nll, d = R.ctc(logits[..., :C], labels, label_len, logit_len, blank)
    ref, dref = _torch_ctc(logits[..., :C], labels, label_len, logit_len, blank)
    assert np.isfinite(nll).all()
    assert _close(nll, ref, 1e-10) and _close(d, dref, 1e-10)


def test_ctc_edges_vs_torch_ctc_loss():
    """L = 0, clamped lengths, one frame with one label -- and the utterance without frames apart (torch does not take it)."""
    case = R.CTC_CASES[0]
    _, B, T, C, ldl, U, blank, kind = case
    logits, labels, label_len, logit_len = R.ctc_inputs(case)
    assert label_len[1] == 0 and label_len[2] > U and logit_len[2] > T and logit_len[3] == 0 and label_len[3] == 0
    nll, d = R.ctc(logits[..., :C], labels, label_len, logit_len, blank)
    keep = np.array([0, 1, 2, 4, 5])
    ref, dref = _torch_ctc(logits[keep][..., :C], labels[keep], label_len[keep], logit_len[keep], blank)
    assert _close(nll[keep], ref, 1e-10) and _close(d[keep], dref, 1e-10)
    assert nll[3] == 0.0 and not d[3].any()
    # no labels: every frame emits the blank
    lp = torch.log_softmax(torch.from_numpy(logits[1, :5, :C].astype(np.float64)), -1)
    assert abs(nll[1] + float(lp[:, blank].sum())) < 1e-12


def test_ctc_repeated_labels_and_infeasible_are_inf_on_both_sides():
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((3, 4, 6))
    labels = np.array([[2, 2, 3], [1, 2, 3], [4, 4, 4]])
    label_len, logit_len = np.array([3, 3, 3]), np.array([4, 4, 4])          # 2 2 3 needs 4 frames: the only path; 4 4 4 needs 5
    nll, d = R.ctc(logits, labels, label_len, logit_len, 0)
    ref, dref = _torch_ctc(logits, labels, label_len, logit_len, 0)
    assert np.isinf(ref[2]) and np.isinf(nll[2]) and nll[2] > 0 and np.isnan(d[2]).all()
    assert _close(nll[:2], ref[:2], 1e-10) and _close(d[:2], dref[:2], 1e-10)
    lp = torch.log_softmax(torch.from_numpy(logits[0]), -1)
    assert abs(nll[0] + float(lp[0, 2] + lp[1, 0] + lp[2, 2] + lp[3, 3])) < 1e-12
    # more labels than frames
    nll, _ = R.ctc(logits, labels, np.array([3, 3, 3]), np.array([2, 4, 4]), 0)
    assert np.isinf(nll[0]) and np.isfinite(nll[1])


def test_ctc_cases_name_their_forms():
    """The launch forms of the kernel test's cases, from the parameters alone (the kernel chooses by C, S = 2 L + 1, S + C <= 2 Sp
    and the LDS left for the staging area): each form of each axis occurs, and the budget cases fit as they say."""
    forms = {}
    for case in R.CTC_CASES:
        name, B, T, C, ldl, U, blank, kind = case
        _, labels, label_len, logit_len = R.ctc_inputs(case)
        forms[name] = R.ctc_form(T, C, U, int(np.minimum(label_len, U).max()))
        assert R.ctc_lds_plan(T, C, U)[0] <= R.CTC_LDS_BYTES, name
        assert 12 * (2 * U + 4) <= 64 * 1024, name                           # the label-length limit of las_ctc_loss
    for axis, values in (('softmax', ('one class per lane', 'two classes per lane', 'loop')), ('recursion', ('side by side', 'strided')),
                         ('lists', (True, False)), ('staging', ('whole', 'several blocks', 'cut by the budget', 'absent'))):
        assert {f[axis] for f in forms.values()} >= set(values), axis
    assert forms['S255_blocks']['recursion'] == 'side by side' and forms['S257_blocks']['recursion'] == 'strided'
    assert forms['C128']['softmax'] == 'two classes per lane' and forms['C129']['softmax'] == 'loop'
    assert forms['staging_cut']['staging'] == 'cut by the budget' and R.ctc_lds_plan(6, 30, 2498)[1:] == (4, 3)
    assert forms['staging_absent']['staging'] == 'absent' and forms['staging_absent']['lists']
    # the issue's example: the launch used to ask for more than the kernel's attribute; now the staging area gives way
    fixed, want, got = R.ctc_lds_plan(240, 9000, 50)
    assert fixed + want * 104 * 4 > R.CTC_LDS_BYTES >= fixed + got * 104 * 4 and 0 < got < want
    assert R.ctc_lds_plan(20, 21000, 6)[0] > R.CTC_LDS_BYTES                  # the refused call of the kernel test


# ---- beam step --------------------------------------------------------------------------------------------------------------
def _brute_force(logits, log_probs, finished, lengths, K, eos):
    """All K V candidates as Python tuples, sorted by (-score, flat index); scores from math, not from array code."""
    import math
    out = []
    for b in range(logits.shape[0]):
        cand = []
        for k, v in itertools.product(range(K), range(logits.shape[2])):
            row = [float(z) for z in logits[b, k]]
            lse = math.log(sum(math.exp(z - max(row)) for z in row)) + max(row)
            step = (0.0 if v == eos else R.F32_MIN) if finished[b, k] else row[v] - lse
            cand.append((-(float(log_probs[b, k]) + step), k * logits.shape[2] + v))
        cand.sort()
        out.append([(i % logits.shape[2], i // logits.shape[2], -s) for s, i in cand[:K]])
    return out


@pytest.mark.parametrize('K,V,eos', [(1, 2, 0), (2, 3, 1), (3, 4, 3), (4, 3, 2)])
def test_beam_step_vs_brute_force(K, V, eos):
    rng = np.random.default_rng(K * 10 + V)
    B = 6
    logits = rng.standard_normal((B, K, V)) * 3
    log_probs = -rng.random((B, K)) * 4
    log_probs[1, 1:] = -np.inf                                    # a first step
    finished = (rng.random((B, K)) < 0.3).astype(np.int64)
    finished[1] = 0
    finished[2] = 1                                               # everything finished
    lengths = rng.integers(0, 9, size=(B, K))
    word, parent, lp, fin, ln, gap_out, gap_in = R.beam_step(logits, log_probs, finished, lengths, K, eos)
    ref = _brute_force(logits, log_probs, finished, lengths, K, eos)
    for b in range(B):
        for j, (w, p, s) in enumerate(ref[b]):
            assert (word[b, j], parent[b, j]) == (w, p)
            assert lp[b, j] == s or abs(lp[b, j] - s) < 1e-12 * max(1.0, abs(s))
            assert fin[b, j] == int(bool(finished[b, p]) or w == eos)
            assert ln[b, j] == lengths[b, p] + (0 if finished[b, p] else 1)
    assert (word[2] == eos).all() and (ln[2] == np.take_along_axis(lengths[2:3], parent[2:3], 1)[0]).all()
    assert (gap_in[0] >= 0) and (gap_out >= 0).all()


def test_beam_step_ties_go_to_the_lower_flat_index():
    logits = np.zeros((1, 3, 4))
    word, parent, lp, *_ = R.beam_step(logits, np.zeros((1, 3)), np.zeros((1, 3), dtype=int), np.zeros((1, 3), dtype=int), 3, 0)
    assert word.tolist() == [[0, 1, 2]] and parent.tolist() == [[0, 0, 0]]


def test_beam_search_vs_oracle_speller_beam(monkeypatch):
    """The oracle's own step (oracle.las_oracle.speller_beam) fed with prepared logits, against the restatement stepped over the same
    logits: per-step scores, final lengths and the back-tracked beams.  Random logits: no ties, so torch.topk's order is defined."""
    from oracle import las_oracle as O
    B, K, V, T = 3, 4, 7, 6
    rng = np.random.default_rng(9)
    feed = rng.standard_normal((T, B * K, V)) * 2

    class Fake:
        def __init__(self, hp, params, memory, mem_len, st, mxu, flag):
            self.t = 0
            self.cells, self.attention, self.align = [], torch.zeros(B * K, 1), torch.zeros(B * K, 1)

        def embed(self, ids):
            return ids

        def step(self, x):
            self.t += 1
            return torch.from_numpy(feed[self.t - 1])

    monkeypatch.setattr(O, 'Speller', Fake)
    hp = O.HP(encoder=O.EncoderHP(), decoder=O.DecoderHP(target_vocab_size=V))
    eos = hp.decoder.eos_id
    mem = torch.zeros(B, T, 2, dtype=O.DT)
    z = torch.zeros(B, 2, dtype=O.DT)
    pred, scores, lengths = O.speller_beam(hp, None, mem, torch.full((B,), T), (z, z), K)
    lp = np.full((B, K), -np.inf)
    lp[:, 0] = 0
    fin, ln = np.zeros((B, K), dtype=np.int64), np.zeros((B, K), dtype=np.int64)
    ids, parents = [], []
    for t in range(scores.shape[1]):
        word, parent, lp, fin, ln, gap_out, gap_in = R.beam_step(feed[t].reshape(B, K, V), lp, fin, ln, K, eos)
        assert min(gap_out.min(), gap_in.min()) > 1e-9                                # tie-free
        assert _close(lp, scores[:, t].numpy())
        ids.append(word)
        parents.append(parent)
    assert np.array_equal(ln, lengths.numpy())
    mine = O.gather_tree(torch.from_numpy(np.stack(ids)), torch.from_numpy(np.stack(parents)), torch.from_numpy(ln.max(1)), eos)
    assert torch.equal(mine.permute(1, 0, 2), pred)


def test_beam_random_cases_stay_within_the_skip_cap():
    """At most BEAM_SKIP_CAP of the (case, utterance) pairs of the kernel test have a gap under BEAM_MARGIN: decided by the
    restatement alone, the kernel has no say in it."""
    pairs = under = 0
    for case in R.BEAM_RANDOM_CASES:
        name, B, K, V, ldl, eos, seed = case
        logits, log_probs, finished, lengths = R.beam_random_inputs(case)
        *_, gap_out, gap_in = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
        pairs += B
        under += int((np.minimum(gap_out, gap_in) <= R.BEAM_MARGIN).sum())
        assert R.beam_lds_bytes(K, V) <= 64 * 1024
    print('beam cases under the margin: %d of %d' % (under, pairs))
    assert under <= R.BEAM_SKIP_CAP * pairs
    # the LDS limit: the largest case is the last one the check admits, the refused one the first beyond
    K, V = R.BEAM_REFUSED
    assert R.beam_lds_bytes(K, V - 1) <= 64 * 1024 < R.beam_lds_bytes(K, V)
    assert any(c[2] == K and c[3] == V - 1 for c in R.BEAM_RANDOM_CASES)


def test_beam_tie_cases_are_exact_ties_and_nothing_else_is_close():
    logits, log_probs, finished, lengths, K, V, eos = R.beam_tie_inputs()
    word, parent, lp, fin, ln, gap_out, gap_in = R.beam_step(logits, log_probs, finished, lengths, K, eos)
    # bit-identical inputs behind every tie
    assert np.array_equal(logits[0, 1], logits[0, 2]) and log_probs[0, 1] == log_probs[0, 2]
    assert (logits[2] == logits[2, 0]).all() and (log_probs[2] == log_probs[2, 0]).all()
    assert np.array_equal(logits[3, 1], logits[3, 3]) and log_probs[3, 1] == log_probs[3, 3]
    a, c = int(np.argsort(-logits[0, 1])[0]), int(np.argsort(-logits[0, 1])[1])
    assert list(zip(parent[0], word[0])) == [(1, a), (2, a), (1, c), (2, c)]
    assert list(zip(parent[1], word[1]))[:3] == [(0, 2), (0, 7), (0, 9)]
    assert list(zip(parent[2], word[2])) == [(0, 3), (0, 8), (1, 3), (1, 8)] and gap_out[2] == 0      # the tie straddles the K-th place
    assert list(zip(parent[3], word[3])) == [(1, 4), (1, 10), (3, 4), (3, 10)]
    assert (gap_in == 0).all()
    # whatever is not an exact tie is far apart: float64 and fp32 agree on it
    assert R.beam_distinct_gap(logits, log_probs, finished, K, eos).min() > 1000 * R.BEAM_MARGIN
    # ... and the reversed rule would give something else
    order = np.argsort(-(log_probs[2][:, None] + logits[2]).reshape(-1)[::-1], kind='stable')
    assert (K * V - 1 - order[0]) // V == K - 1
