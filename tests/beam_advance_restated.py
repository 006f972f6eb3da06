"""las_beam_advance restated in NumPy from its contract in include/las_hip.h: the selection is loss_heads_restated.beam_step
(float64, stable sort of all K V candidates -- no per-beam lists, no merge), everything else is integer or byte bookkeeping: the
records, the fed token, the embedded feed, the row gathers and the ledger with its freeze.  Also the inputs of
tests/test_gpu_beam_advance.py that are not loss_heads_restated's."""
import numpy as np

import tests.loss_heads_restated as R


def gather_rows(rows, parents):
    """rows [B * K, ...], parents [B, K] -> the rows after the gather: row b K + j = what row b K + parents[b, j] held."""
    B, K = parents.shape
    flat = (parents + np.arange(B)[:, None] * K).reshape(-1)
    return rows[flat].copy()


def new_ledger(B):
    return dict(utt_done=np.zeros(B, dtype=np.int32), remaining=B, steps_done=0)


def advance(logits, state, K, eos, t, records, ledger, fed=None, emb=None, x_next=None, jobs=()):
    """One launch.  logits [B, K, V]; state = (log_probs, finished, lengths) [B, K]; records = (word_ids, parent_ids) [B K, U];
    fed [B K, U] or None; emb [V, E] and x_next [B K, >= E] or None; jobs: arrays [B K, ...].  Everything is updated IN PLACE, as
    the kernel does, except the log-probs, which are returned in float64 (the state array takes their fp32 rounding).  Returns
    (log-probs float64 [B, K] or None when frozen, gap_out, gap_in)."""
    if 0 < ledger['steps_done'] <= t:
        return None, None, None
    log_probs, finished, lengths = state
    B = logits.shape[0]
    word, parent, lp, fin, ln, gap_out, gap_in = R.beam_step(logits, log_probs, finished, lengths, K, eos)
    log_probs[...] = lp.astype(np.float32)
    finished[...] = fin
    lengths[...] = ln
    records[0][:, t] = word.reshape(-1)
    records[1][:, t] = parent.reshape(-1)
    if fed is not None:
        fed[:, t + 1] = word.reshape(-1)
    for rows in jobs:
        rows[...] = gather_rows(rows, parent)
    if x_next is not None:
        x_next[:, :emb.shape[1]] = emb[word.reshape(-1)]
    for b in range(B):
        if fin[b].all() and not ledger['utt_done'][b]:
            ledger['utt_done'][b] = 1
            ledger['remaining'] -= 1
            if ledger['remaining'] == 0:
                ledger['steps_done'] = t + 1
    return lp, gap_out, gap_in


# ---- states beyond the LDS limit of las_beam_step ---------------------------------------------------------------------------
# (id, B, K, V, ldl, eos, seed): K V words exceed las_beam_step's 64-KB candidate buffer in each.  The seeds are chosen on the CPU
# so that every utterance keeps both of the restatement's gaps above R.BEAM_MARGIN (tests/test_beam_device_host.py asserts it).
BEYOND_CASES = [
    ('K8_V2100', 3, 8, 2100, 2104, 1, 0),
    ('K32_V600', 2, 32, 600, 600, 2, 0),
    ('K4_V4200', 2, 4, 4200, 4200, 0, 3),
]


def beyond_inputs(case):
    """R.beam_random_inputs' state (about a quarter of the beams finished, NaN in the pad columns) with every beam of the last
    utterance finished."""
    logits, log_probs, finished, lengths = R.beam_random_inputs(case)
    finished[-1] = 1
    return logits, log_probs, finished, lengths


def beyond_skipped():
    """(utterances under the margin, all utterances) over BEYOND_CASES, from the float64 restatement alone."""
    under = pairs = 0
    for case in BEYOND_CASES:
        name, B, K, V, ldl, eos, seed = case
        logits, log_probs, finished, lengths = beyond_inputs(case)
        *_, gap_out, gap_in = R.beam_step(logits[..., :V], log_probs, finished, lengths, K, eos)
        under += int((np.minimum(gap_out, gap_in) <= R.BEAM_MARGIN).sum())
        pairs += B
    return under, pairs


# ---- hand-made states -------------------------------------------------------------------------------------------------------
def parents_0021_inputs():
    """K = 4 over V = 6 (eos = 5, not among the winners): logits = log p, so the step scores are log p exactly up to rounding.
    Winners in order: (beam 0, class 0), (0, 1), (2, 0), (1, 4): parents (0, 0, 2, 1), every neighbour gap above 0.4."""
    K, V, eos = 4, 6, 5
    p = np.array([[0.5, 0.3, 0.05, 0.05, 0.05, 0.05],
                  [0.02, 0.02, 0.02, 0.02, 0.9, 0.02],
                  [0.9, 0.02, 0.02, 0.02, 0.02, 0.02],
                  [0.2, 0.2, 0.2, 0.2, 0.1, 0.1]])
    logits = np.log(p).astype(np.float32)[None]
    log_probs = np.array([[0.0, -2.0, -1.5, -9.0]], dtype=np.float32)
    return logits, log_probs, np.zeros((1, K), dtype=np.int32), np.array([[3, 4, 5, 6]], dtype=np.int32), K, V, eos


def parents_all_7_inputs():
    """K = 8 over V = 10 (eos = 9): beam 7 is 50 ahead of the others, so its eight best classes are the winners."""
    K, V, eos = 8, 10, 9
    logits = np.tile((np.arange(V)[::-1] * 0.5).astype(np.float32), (1, K, 1))
    logits[0, 7] = np.array([3.0, 1.0, 4.5, 0.5, 2.5, 4.0, 1.5, 3.5, 2.0, 0.0], dtype=np.float32)
    log_probs = np.full((1, K), -50.0, dtype=np.float32)
    log_probs[0, 7] = -1.0
    return logits, log_probs, np.zeros((1, K), dtype=np.int32), np.arange(K, dtype=np.int32)[None], K, V, eos


def three_step_logits():
    """B = 2, K = 2, V = 4, eos = 1.  Step 0: nobody takes eos.  Step 1: every beam of utterance 0 takes eos (logit +20), utterance 1
    goes on.  Step 2: utterance 1 finishes too.  (The test asserts the restatement's gaps at every step.)"""
    K, V, eos = 2, 4, 1
    go = np.array([[1.5, -20.0, 0.5, 0.0], [0.3, -20.0, 1.6, 0.0]], dtype=np.float32)          # (a row per beam)
    stop = np.array([[0.0, 20.0, 0.75, 1.5], [0.5, 20.0, 0.1, 1.0]], dtype=np.float32)
    mk = lambda u0, u1: np.stack([u0, u1])
    return [mk(go, go), mk(stop, go), mk(go, stop)], K, V, eos
