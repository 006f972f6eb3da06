"""The kernels between the logits and the reported numbers -- las_seq_ce_loss, las_seq_sigmoid_loss, las_log_probs_loss,
las_ctc_loss, las_beam_step -- restated in NumPy float64 from their contracts in include/las_hip.h and the formulas in the kernels'
header comments (tf.contrib.seq2seq.sequence_loss, sigmoid_cross_entropy_with_logits, compute_log_probs_loss, the alpha / beta
recursion of Graves et al. 2006, one step of BeamSearchDecoder with length_penalty_weight 0).  Nothing here follows the kernels'
code: no -1e30 in place of -inf, no fast exponentials, no bf16.  The second half holds the inputs of the kernel tests
(tests/test_gpu_loss_heads.py), so that tests/test_loss_heads_host.py can check their conditions without a GPU.  Imports nothing
from the project."""
import numpy as np

F64 = np.float64
F32_MIN = float(np.finfo(np.float32).min)          # the step score of a finished beam away from eos (_mask_probs)


def _log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def _mask(lens, U):
    n = np.minimum(np.asarray(lens, dtype=np.int64), U)
    return (np.arange(U)[None, :] < n[:, None]).astype(F64), float(n.sum()) + 1e-12


# ---- the three sums ---------------------------------------------------------------------------------------------------------
def seq_ce(logits, targets, target_len):
    """logits [B, U, V], targets [B, U], target_len [B] -> (loss, dlogits [B, U, V]): sum over t < min(len, U) of the cross
    entropy, divided by sum(min(len, U)) + 1e-12."""
    logits = np.asarray(logits, dtype=F64)
    B, U, V = logits.shape
    w, total = _mask(target_len, U)
    lp = _log_softmax(logits)
    onehot = np.zeros_like(lp)
    np.put_along_axis(onehot, np.asarray(targets, dtype=np.int64)[..., None], 1.0, -1)
    loss = float((-(lp * onehot).sum(-1) * w).sum() / total)
    return loss, (np.exp(lp) - onehot) * w[..., None] / total


def seq_sigmoid(logits, targets, seq_len):
    """logits, targets (0 / 1) [B, U, nf], seq_len [B] -> (loss, dlogits): per step the mean over nf of
    max(x, 0) - x z + log1p(exp(-|x|)); mask and divisor as seq_ce."""
    x, z = np.asarray(logits, dtype=F64), np.asarray(targets, dtype=F64)
    B, U, nf = x.shape
    w, total = _mask(seq_len, U)
    bce = np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))
    loss = float((bce.mean(-1) * w).sum() / total)
    sig = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
    return loss, (sig - z) / nf * w[..., None] / total


def log_probs_kink_distance(x, nf):
    """|e^a + e^b - 1| per element: how far each element is from the kink of the absolute value."""
    x = np.asarray(x, dtype=F64)
    return np.abs(np.exp(x[:, :nf]) + np.exp(x[:, nf:2 * nf]) - 1.0)


def log_probs_loss(x, nf):
    """x [rows, 2 nf] = [a | b] -> (loss, dx): the mean over rows x nf of |e^a + e^b - 1| + relu(a) + relu(b)."""
    x = np.asarray(x, dtype=F64)
    a, b = x[:, :nf], x[:, nf:2 * nf]
    ea, eb = np.exp(a), np.exp(b)
    v = ea + eb - 1.0
    n = a.size
    loss = float((np.abs(v) + np.maximum(a, 0.0) + np.maximum(b, 0.0)).sum() / n)
    sg = np.sign(v)
    return loss, np.concatenate([sg * ea + (a > 0), sg * eb + (b > 0)], 1) / n


# ---- CTC --------------------------------------------------------------------------------------------------------------------
def _lae(a, b):
    with np.errstate(invalid='ignore'):
        r = np.logaddexp(a, b)
    return np.where(np.isneginf(a) & np.isneginf(b), -np.inf, r)


def ctc(logits, labels, label_len, logit_len, blank):
    """logits [B, T, C], labels [B, U], label_len, logit_len [B] -> (per-example negative log likelihood [B], dlogits [B, T, C]).
    Utterance b: its first min(label_len, U) labels over its first min(logit_len, T) frames.  alpha_t(s) and beta_t(s) both include
    the emission at t, so that d nll / d logits[t, c] = y_t(c) - sum_{s: ext(s) = c} alpha_t(s) beta_t(s) / (y_t(c) p).  No path
    (more labels, repeats counted twice, than frames): +inf and a NaN gradient.  No frames and no labels: the empty path, 0."""
    logits = np.asarray(logits, dtype=F64)
    B, T, C = logits.shape
    U = np.asarray(labels).shape[1]
    nll = np.zeros(B)
    d = np.zeros_like(logits)
    for b in range(B):
        L, Tb = min(int(label_len[b]), U), min(int(logit_len[b]), T)
        if Tb <= 0:
            nll[b] = 0.0 if L == 0 else np.inf
            d[b] = 0.0 if L == 0 else np.nan
            continue
        S = 2 * L + 1
        ext = np.full(S, blank, dtype=np.int64)
        ext[1::2] = np.asarray(labels[b][:L], dtype=np.int64)
        lp = _log_softmax(logits[b, :Tb])
        em = lp[:, ext]                                            # [Tb, S]
        skip = np.zeros(S, dtype=bool)                             # s may be entered from s - 2
        skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
        ninf = np.full(2, -np.inf)
        alpha = np.full((Tb, S), -np.inf)
        alpha[0, :2] = em[0, :2]
        for t in range(1, Tb):
            p = np.concatenate([ninf, alpha[t - 1]])
            alpha[t] = _lae(_lae(p[2:], p[1:-1]), np.where(skip, p[:-2], -np.inf)) + em[t]
        beta = np.full((Tb, S), -np.inf)
        beta[Tb - 1, max(S - 2, 0):] = em[Tb - 1, max(S - 2, 0):]
        skipb = np.zeros(S, dtype=bool)                            # s may go on to s + 2
        skipb[:-2] = skip[2:]
        for t in range(Tb - 2, -1, -1):
            p = np.concatenate([beta[t + 1], ninf])
            beta[t] = _lae(_lae(p[:-2], p[1:-1]), np.where(skipb, p[2:], -np.inf)) + em[t]
        ll = _lae(alpha[Tb - 1, S - 1], alpha[Tb - 1, S - 2]) if S > 1 else alpha[Tb - 1, 0]
        nll[b] = -float(ll)
        if np.isneginf(ll):
            d[b] = np.nan
            continue
        ab = alpha + beta
        acc = np.full((Tb, C), -np.inf)
        for s in range(S):
            acc[:, ext[s]] = _lae(acc[:, ext[s]], ab[:, s])
        d[b, :Tb] = np.exp(lp) - np.exp(acc - lp - ll)
    return nll, d


# ---- beam step --------------------------------------------------------------------------------------------------------------
def beam_step(logits, log_probs, finished, lengths, K, eos):
    """logits [B, K, V], log_probs / finished / lengths [B, K] (the state before the step) -> word_ids, parent_ids, log_probs,
    finished, lengths [B, K] after it, and per utterance two float64 gaps: between the K-th and the (K+1)-th candidate (inf when
    there is no (K+1)-th) and the smallest between neighbours inside the top K (inf for K = 1).  Candidates: previous log-prob plus
    the step's log-softmax; a finished beam offers (k, eos) at step score 0 and float32 min elsewhere.  The K best of the K V
    candidates, ties to the lower flat index k V + v; a length grows by one unless the parent had finished."""
    logits = np.asarray(logits, dtype=F64)
    B, K_, V = logits.shape
    assert K_ == K
    fin = np.asarray(finished).astype(bool)
    fin_row = np.full(V, F32_MIN)
    fin_row[eos] = 0.0
    step = np.where(fin[..., None], fin_row[None, None, :], _log_softmax(logits))
    total = (np.asarray(log_probs, dtype=F64)[..., None] + step).reshape(B, K * V)
    order = np.argsort(-total, axis=1, kind='stable')
    top = order[:, :K]
    word, parent = top % V, top // V
    srt = np.take_along_axis(total, order[:, :K + 1], 1)
    with np.errstate(invalid='ignore'):
        diffs = np.nan_to_num(srt[:, :-1] - srt[:, 1:], nan=0.0, posinf=np.inf)        # -inf beside -inf: a tie
    if K * V > K:
        gap_out, inside = diffs[:, K - 1], diffs[:, :K - 1]
    else:
        gap_out, inside = np.full(B, np.inf), diffs[:, :K - 1]
    gap_in = inside.min(1) if K > 1 else np.full(B, np.inf)
    pf = np.take_along_axis(fin, parent, 1)
    new_fin = pf | (word == eos)
    new_len = np.take_along_axis(np.asarray(lengths, dtype=np.int64), parent, 1) + (~pf)
    return (word, parent, np.take_along_axis(total, top, 1), new_fin.astype(np.int64), new_len, gap_out, gap_in)


def beam_distinct_gap(logits, log_probs, finished, K, eos):
    """Per utterance the smallest NON-ZERO difference between neighbours among the K + 1 best candidates (inf if none): what the
    constructed-tie cases must keep above the margin, their exact ties aside."""
    logits = np.asarray(logits, dtype=F64)
    B, _, V = logits.shape
    fin_row = np.full(V, F32_MIN)
    fin_row[eos] = 0.0
    step = np.where(np.asarray(finished).astype(bool)[..., None], fin_row[None, None, :], _log_softmax(logits))
    total = (np.asarray(log_probs, dtype=F64)[..., None] + step).reshape(B, K * V)
    srt = -np.sort(-total, axis=1)[:, :K + 1]
    with np.errstate(invalid='ignore'):
        diffs = np.nan_to_num(srt[:, :-1] - srt[:, 1:], nan=0.0, posinf=np.inf)
    return np.where(diffs > 0, diffs, np.inf).min(1)


# =============================================================================================================================
# The inputs of the kernel tests.  Everything the device reads is fp32 or bf16, so the inputs are generated in those formats and
# the restatements see the same values exactly.
# =============================================================================================================================
def f2bf_bits(x):
    """fp32 -> bf16 bits, round to nearest even (finite inputs)."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf_bits2f(u):
    return (np.asarray(u, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def ragged_lengths(rng, B, U):
    """Lengths in [0, U + 3] that always hold a 0, a U and one beyond U (clamped by the kernels) when B allows."""
    n = rng.integers(0, U + 4, size=B)
    for i, v in enumerate((U + 2, 0, U)[:B]):
        n[i] = v
    return n.astype(np.int32)


# (id, B, U, V, ldl, ldd, with gradient): what each CE case is there for
CE_CASES = [
    ('anchor_V11', 5, 7, 11, 16, 16, True),            # the shape of the existing test: V < 64, one lap of everything
    ('V200_ldl_ne_ldd', 3, 5, 200, 208, 216, True),    # the lane loop runs four times; ldl != ldd
    ('V64', 4, 6, 64, 64, 64, True),                   # exactly one full lap, no pad columns
    ('V65', 4, 6, 65, 72, 80, True),                   # the second lap holds one lane
    ('B70', 70, 3, 33, 40, 48, True),                  # the loop that forms `total` runs twice (B > 64)
    ('rows1209_gridstride', 31, 39, 70, 72, 72, True),  # 1209 rows > 4 x 256: the grid-stride loop's second lap
    ('no_gradient', 5, 7, 65, 72, 0, False),           # dlogits == NULL
]
# (id, B, U, nf, ldl, ldt, ldd, with gradient)
SIGMOID_CASES = [
    ('anchor_nf6', 5, 7, 6, 8, 6, 8, True),
    ('nf150_ldt_ne_nf', 3, 5, 150, 152, 160, 168, True),   # three laps over the features, every stride different
    ('nf64', 4, 6, 64, 64, 64, 64, True),
    ('nf65', 4, 6, 65, 72, 66, 80, True),
    ('B70', 70, 3, 20, 24, 24, 32, True),
    ('rows1209_gridstride', 31, 39, 40, 40, 48, 40, True),
    ('no_gradient', 5, 7, 65, 72, 65, 0, False),
]
# (id, rows, nf, ldx, ldd, with gradient)
LOG_PROBS_CASES = [
    ('tiny', 35, 6, 12, 12, True),                          # one workgroup, partly filled
    ('wide_strides', 300, 24, 56, 64, True),                # ldx and ldd wider than 2 nf
    ('gridstride', 9000, 40, 80, 88, True),                 # 360 000 elements > 1024 x 256: the second lap
    ('no_gradient', 300, 24, 48, 0, False),                 # dx == NULL
]
LOG_PROBS_KINK_MIN = 1e-2


def ce_inputs(case):
    name, B, U, V, ldl, ldd, grad = case
    rng = np.random.default_rng(1000 + B * U + V)
    logits = (rng.standard_normal((B, U, ldl)) * 3).astype(np.float32)
    logits[..., V:] = np.nan                                                  # pad columns must not be read
    return logits, rng.integers(0, V, size=(B, U)).astype(np.int32), ragged_lengths(rng, B, U)


def sigmoid_inputs(case):
    name, B, U, nf, ldl, ldt, ldd, grad = case
    rng = np.random.default_rng(2000 + B * U + nf)
    logits = (rng.standard_normal((B, U, ldl)) * 3).astype(np.float32)
    logits[..., nf:] = np.nan
    targets = (rng.random((B, U, ldt)) < 0.4).astype(np.float32)
    targets[..., nf:] = np.nan
    return logits, targets, ragged_lengths(rng, B, U)


def log_probs_inputs(case):
    """bf16 bits [rows, ldx]: a and b around zero so that every sign case occurs (e^a + e^b above and below 1, a > 0, b > 0);
    an element closer than LOG_PROBS_KINK_MIN to the kink is moved away from it; NaN in the columns past 2 nf."""
    name, rows, nf, ldx, ldd, grad = case
    rng = np.random.default_rng(3000 + rows + nf)
    x = bf_bits2f(f2bf_bits(rng.standard_normal((rows, ldx)) * 0.9 - 0.6))
    for _ in range(8):
        near = log_probs_kink_distance(x, nf) < 2 * LOG_PROBS_KINK_MIN
        if not near.any():
            break
        a = x[:, :nf]
        a[near] = bf_bits2f(f2bf_bits(a[near] + np.float32(0.25)))
    bits = f2bf_bits(x)
    bits[:, 2 * nf:] = 0x7FC0
    return bits


# ---- CTC: (id, B, T, C, ldl, U, blank, kind) --------------------------------------------------------------------------------
CTC_LDS_BYTES = 160 * 1024 - 64


def ctc_lds_plan(T, C, U):
    """The host side's budget arithmetic of las_ctc_loss: (bytes every launch needs, frames of the staging area the
    96 KiB target would give, frames it gets).  Fixed part: the two alpha columns, the states, the two beta columns (5 Sp words,
    Sp = 2 U + 4) and the class counters (2 C + 2 words)."""
    Sp = 2 * U + 4
    fixed = 5 * Sp * 4 + (2 * C + 2) * 4
    want = min(T, (96 * 1024) // (Sp * 4))
    got = min(want, max(CTC_LDS_BYTES - fixed, 0) // (Sp * 4))
    return fixed, want, got


def ctc_form(T, C, U, Lmax):
    """The launch forms a case runs, read off its parameters."""
    Sp, S = 2 * U + 4, 2 * min(Lmax, U) + 1
    fixed, want, got = ctc_lds_plan(T, C, U)
    lists = S + C <= 2 * Sp
    if not lists:
        stage = 'unused(no lists)'
    elif got == 0:
        stage = 'absent'
    elif got < want:
        stage = 'cut by the budget'
    else:
        stage = 'whole' if got >= T else 'several blocks'
    return {'softmax': 'one class per lane' if C <= 64 else ('two classes per lane' if C <= 128 else 'loop'),
            'recursion': 'side by side' if S <= 256 else 'strided', 'lists': lists, 'staging': stage}


CTC_CASES = [
    # C <= 64, S <= 256, lists fit, staging area whole; the ragged edges: L = 0, label_len > U, logit_len > T, no frames
    ('edges_C9', 6, 17, 9, 16, 6, 0, 'edges'),
    ('C64', 4, 20, 64, 64, 8, 0, 'random'),                 # the last class of the first lane set, no pad columns
    ('C65', 4, 20, 65, 72, 8, 0, 'random'),                 # two classes per lane, the second set holds one
    ('C100_two_per_lane', 5, 40, 100, 104, 60, 0, 'random'),
    ('C128', 4, 20, 128, 128, 8, 0, 'random'),              # two classes per lane, both sets full
    ('C129', 4, 20, 129, 136, 8, 0, 'random'),              # the loop form's first size; lists do not fit (S + C > 2 Sp)
    ('C150_no_lists', 5, 40, 150, 152, 12, 0, 'random'),
    ('S255_blocks', 3, 300, 30, 32, 127, 0, 'full'),        # S = 255: side by side; staging in several blocks (95 frames)
    ('S257_blocks', 3, 300, 30, 32, 128, 0, 'full'),        # S = 257: the strided recursion
    ('same_label_long_list', 4, 60, 20, 24, 20, 0, 'same'),  # a non-blank class with 20 states (> LONG_LIST): a frame per lane
    ('same_label_blank5', 4, 60, 20, 24, 20, 5, 'same'),
    ('blank_last', 5, 30, 12, 16, 9, 11, 'random'),         # blank != 0
    ('staging_cut', 3, 6, 30, 32, 2498, 0, 'random'),       # Sp = 5000: the budget leaves 3 frames where 96 KiB hold 4
    ('staging_absent', 3, 5, 4500, 4504, 2728, 0, 'random'),  # Sp = 5460, C = 4500: no frame fits, lists do: the walk through memory
    ('C9000_issue', 2, 240, 9000, 9000, 50, 0, 'random'),   # 8 C + 8 bytes of counters: the staging area shrinks (never ran before)
]


def ctc_inputs(case):
    """-> logits [B, T, ldl] fp32 (NaN pads), labels [B, U] int32, label_len, logit_len [B] int32.  Every utterance has a path
    (logit_len >= labels + repeats) unless the kind says otherwise."""
    name, B, T, C, ldl, U, blank, kind = case
    rng = np.random.default_rng(4000 + T + C + U + blank)
    logits = (rng.standard_normal((B, T, ldl)) * 2).astype(np.float32)
    logits[..., C:] = np.nan
    classes = np.array([c for c in range(C) if c != blank])
    labels = classes[rng.integers(0, len(classes), size=(B, U))].astype(np.int32)
    Lcap = min(U, 18, (T - 1) // 2)
    if kind == 'same':
        labels[:] = classes[3]
        labels[-1] = classes[rng.integers(0, len(classes), size=U)]
        label_len = np.array([U] + [int(v) for v in rng.integers(9, U + 1, size=B - 1)], dtype=np.int32)
    elif kind == 'full':
        label_len = np.array([U, U - 1, 3][:B], dtype=np.int32)
        for b in range(B):                                        # no repeats: U labels fit 2 U frames whatever they are
            labels[b] = classes[(np.arange(U) + b) % len(classes)]
    else:
        label_len = rng.integers(1, Lcap + 1, size=B).astype(np.int32)
        label_len[0] = Lcap
        labels[0, 2 % U] = labels[0, 1 % U]                         # a repeated label (needs the blank between)
    need = np.array([int(n) + int((labels[b, 1:n] == labels[b, :n - 1]).sum()) for b, n in enumerate(np.minimum(label_len, U))])
    logit_len = np.array([int(rng.integers(n, T + 1)) if n <= T else T for n in need], dtype=np.int32)
    logit_len[0] = T
    if kind == 'edges':
        label_len[1], logit_len[1] = 0, 5                          # no labels: the single blank state (S = 1)
        label_len[2], logit_len[2] = U + 4, T + 9                  # both clamped (to U and T)
        labels[2] = classes[(np.arange(U)) % len(classes)]         # (U distinct labels: a path exists in T >= U frames)
        label_len[3], logit_len[3] = 0, 0                          # no frames, no labels: the empty path
        label_len[4], logit_len[4] = 1, 1                          # one frame, one label
    return logits, labels, label_len, logit_len


# ---- beam step: (id, B, K, V, ldl, eos, seed) -------------------------------------------------------------------------------
BEAM_MARGIN = 1e-4            # a random utterance counts when both of the restatement's gaps exceed this
BEAM_SKIP_CAP = 0.02          # ... and at most this share of all (case, utterance) pairs may fall below it
BEAM_LOGIT_SCALE = 3.0
BEAM_RANDOM_CASES = [
    ('K4_V40', 16, 4, 40, 40, 1, 11),                 # V < 64: one partly filled lap
    ('K5_V100', 16, 5, 100, 104, 2, 12),              # K and V multiples of nothing
    ('K3_V64', 16, 3, 64, 64, 63, 13),                # V = 64, eos the last class
    ('K8_V129', 16, 8, 129, 136, 0, 14),              # two waves' laps over the beams, eos = 0
    ('K6_V5', 8, 6, 5, 8, 4, 15),                     # more beams than classes
    ('K1_V70', 8, 1, 70, 72, 1, 16),                  # greedy: one beam
    ('K5_V3271_lds_limit', 2, 5, 3271, 3272, 1, 17),  # (5 x 3271 + 4 x 5 + 8) words = 65 532 bytes: the largest the check admits at K = 5
]
BEAM_REFUSED = (5, 3272)        # one class more: 65 552 bytes


def beam_lds_bytes(K, V):
    return (K * V + 4 * K + 8) * 4


def beam_random_inputs(case):
    """A state in the middle of a search: finite log-probs, a quarter of the beams finished, any lengths; NaN in the pad columns
    (which must not be read)."""
    name, B, K, V, ldl, eos, seed = case
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, K, ldl)) * BEAM_LOGIT_SCALE).astype(np.float32)
    logits[..., V:] = np.nan
    log_probs = (-rng.random((B, K)) * 6).astype(np.float32)
    finished = (rng.random((B, K)) < 0.25).astype(np.int32)
    lengths = rng.integers(0, 30, size=(B, K)).astype(np.int32)
    return logits, log_probs, finished, lengths


def beam_first_step_inputs(B, K, V, ldl, seed):
    """The state a search starts from: log_probs = [0, -inf, ...], nothing finished, lengths 0."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, K, ldl)) * BEAM_LOGIT_SCALE).astype(np.float32)
    logits[..., V:] = np.nan
    log_probs = np.full((B, K), -np.inf, dtype=np.float32)
    log_probs[:, 0] = 0.0
    return logits, log_probs, np.zeros((B, K), dtype=np.int32), np.zeros((B, K), dtype=np.int32)


def beam_tie_inputs():
    """Exact ties by construction, B = 4 utterances of K = 4 beams over V = 12 classes (eos = 1):
    0: beams 1 and 2 have bit-identical logit rows and equal log-probs, ahead of the others: every candidate of beam 2 ties with
       the same class of beam 1, and the lower flat index (beam 1) goes first;
    1: the best class of the leading beam appears three times in its row (classes 2, 7, 9): 2, 7, 9 in this order;
    2: all four beams identical and the best class twice in the row (classes 3 and 8): an eight-way tie that straddles the K-th
       place; the winners are (0, 3), (0, 8), (1, 3), (1, 8);
    3: beams 1 and 3 identical and their best class twice in the row (classes 4 and 10): a 2 x 2 block of equal candidates fills the
       top four, (1, 4), (1, 10), (3, 4), (3, 10).
    The logits lie on a grid of 3/4 and the log-probs off it, so that candidates that are not tied by construction are far apart."""
    B, K, V, eos = 4, 4, 12, 1
    rng = np.random.default_rng(77)
    logits = (rng.permuted(np.tile(np.arange(V), (B, K, 1)), axis=-1) * 0.75).astype(np.float32)
    log_probs = np.array([[-9.1, -1.0, -1.0, -8.3], [-0.5, -7.1, -8.3, -9.2], [-2.0, -2.0, -2.0, -2.0], [-6.1, -1.5, -7.3, -1.5]],
                         dtype=np.float32)
    logits[0, 2] = logits[0, 1]
    logits[1, 0, [2, 7, 9]] = logits[1, 0].max() + 0.75
    logits[2, 0, [3, 8]] = logits[2, 0].max() + 0.75
    logits[2, 1:] = logits[2, 0]
    logits[3, 1, [4, 10]] = logits[3, 1].max() + 1.5
    logits[3, 3] = logits[3, 1]
    finished = np.zeros((B, K), dtype=np.int32)
    lengths = np.array([[3, 4, 5, 6]] * B, dtype=np.int32)
    return logits, log_probs, finished, lengths, K, V, eos
