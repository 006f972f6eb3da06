"""A NumPy / Python restatement of the reference's frame-level binary-feature accuracy (infer.py --calc_frame_binf_accuracy),
the yardstick of csrc/align.hip and phones-las_amd/frame_binf.py:

  * fastdtw 0.3.x ``dtw(range(U), range(T'), dist=lambda i, j: -A[i, j])``: a float64 table (NumPy 1.16 promotes
    ``0 + np.float32`` to float64), three sums per cell, a candidate wins only when strictly smaller in the order up, left,
    diagonal (Python's min), the path walked back from (U, T');
  * soft2hard_attention's cleanup and attention_to_segments;
  * segs_phones_to_frame_binf, segments_to_attention (--use_markup_segments; its window never leaves the first five phones),
    get_binf_markup_frames;
  * librosa 0.7.1 time_to_frames with the reference's arguments.

Plain loops, no vectorisation: slow, and meant to be read."""
import numpy as np


def dtw(A):
    """(D [U+1, T'+1] float64, path as a list of (row, column) cells in path order)."""
    A = np.asarray(A, dtype=np.float32)
    U, T = A.shape
    D = np.full((U + 1, T + 1), np.inf)
    D[0, 0] = 0.0
    back = np.zeros((U + 1, T + 1), dtype=np.int8)
    for i in range(1, U + 1):
        for j in range(1, T + 1):
            dt = float(-A[i - 1, j - 1])          # float32 negation, then float64
            cands = (D[i - 1, j] + dt, D[i, j - 1] + dt, D[i - 1, j - 1] + dt)
            best, code = cands[0], 0
            for k in (1, 2):
                if cands[k] < best:
                    best, code = cands[k], k
            D[i, j] = best
            back[i, j] = code
    path = []
    i, j = U, T
    while not (i == 0 and j == 0):
        path.append((i - 1, j - 1))
        code = back[i, j]
        if code == 0:
            i -= 1
        elif code == 1:
            j -= 1
        else:
            i, j = i - 1, j - 1
        if (i == 0) != (j == 0):
            raise IndexError('the path left the grid')
    path.reverse()
    return D, path


def hard_attention(A):
    """soft2hard_attention: the 0/1 path matrix after the cleanup (uint8 [U, T'])."""
    A = np.asarray(A, dtype=np.float32)
    U, T = A.shape
    _, path = dtw(A)
    H = np.zeros((U, T), dtype=np.uint8)
    for i, j in path:
        H[i, j] = 1
    for c in range(T):
        rows = np.flatnonzero(H[:, c])
        if len(rows) <= 1:
            continue
        lo, hi = rows[0], rows[-1]
        if A[lo, c] > A[hi, c]:
            if c < T - 1 and H[hi, c + 1] == 1:
                H[hi, c] = 0
        else:
            if c > 0 and H[lo, c - 1] == 1:
                H[lo, c] = 0
    return H


def runs(H):
    """Per column the first and the last row of the path (lo 0 / hi -1 for an empty column)."""
    T = H.shape[1]
    lo = np.zeros(T, dtype=np.int64)
    hi = np.full(T, -1, dtype=np.int64)
    for c in range(T):
        r = np.flatnonzero(H[:, c])
        if len(r):
            lo[c], hi[c] = r[0], r[-1]
    return lo, hi


def segments(H):
    """attention_to_segments on the cleaned path: a list of [st_frame, en_frame, st_phone, en_phone]."""
    U, T = H.shape
    out = []
    st_frame = st_phone = en_phone = phone = 0
    for c in range(T):
        r = np.flatnonzero(H[:, c])
        if len(r):
            phone = int(r[-1])
        if phone > en_phone and c > 0:
            out.append([st_frame, c, st_phone, phone])
            en_phone = st_phone = phone
            st_frame = c
    out.append([st_frame, T, st_phone, U])
    return out


def align(A):
    """Everything the DTW kernel outputs for one matrix: (run_lo, run_hi, ph_st, ph_en per frame, segment count).
    U = 0 or T' = 0: no segments (the reference raises in its backtrack)."""
    A = np.asarray(A, dtype=np.float32)
    U, T = A.shape
    if U == 0 or T == 0:
        return (np.zeros(T, np.int64), np.full(T, -1, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64), 0)
    H = hard_attention(A)
    lo, hi = runs(H)
    segs = segments(H)
    st = np.zeros(T, dtype=np.int64)
    en = np.zeros(T, dtype=np.int64)
    for s in segs:
        st[s[0]:s[1]] = s[2]
        en[s[0]:s[1]] = s[3]
    return lo, hi, st, en, len(segs)


def time_to_frames(segs, nsamples, encoder_frame_step=40):
    """The markup in frames as infer.py computes it: markup / 16000, np.minimum with nsamples / 16000, then librosa 0.7.1's
    time_to_samples ((t * sr).astype(int)) and samples_to_frames (floor((s - int(n_fft // 2)) // hop)), negatives to 0."""
    sr = 16000
    t = np.asarray(segs, dtype=np.float64).reshape(-1, 2) / sr
    t = np.minimum(t, nsamples / sr)
    samples = (t * sr).astype(int)
    hop = encoder_frame_step * sr / 1000
    offset = int((0.02 * sr) // 2)
    frames = np.floor((samples - offset) // hop).astype(int)
    frames[frames < 0] = 0
    return frames


def markup_frames_binf(frames, binfs):
    """get_binf_markup_frames: bool [frames[-1, -1], F], each frame the OR of the rows of the segments covering it."""
    n = int(frames[-1, -1]) if len(frames) else 0
    F = np.asarray(binfs).shape[1]
    out = np.zeros((max(n, 0), F), dtype=bool)
    for (st, en), b in zip(frames, binfs):
        out[st:en] = np.logical_or(out[st:en], np.asarray(b) != 0)
    return out


def pred_frames_dtw(A, P):
    """segs_phones_to_frame_binf on attention_to_segments: bool [T', F]; U = 0 gives all-zero frames over T'."""
    A = np.asarray(A, dtype=np.float32)
    U, T = A.shape
    F = np.asarray(P).reshape(-1, P.shape[-1]).shape[1]
    out = np.zeros((T, F), dtype=bool)
    if U == 0 or T == 0:
        return out
    H = hard_attention(A)
    for st_f, en_f, st_p, en_p in segments(H):
        v = np.zeros(F, dtype=bool)
        for r in range(st_p, en_p):
            v = np.logical_or(v, P[r] != 0)
        out[st_f:en_f] = v
    return out


def markup_phones(A, frames):
    """segments_to_attention's choice per markup segment: argmax over the first min(5, U) rows of the max of A over the frames
    [st, max(en, st + 1)) (NumPy's tie and NaN rules); -1 when U = 0 or the window holds no frame of A."""
    A = np.asarray(A, dtype=np.float32)
    U, T = A.shape
    out = []
    for st, en in frames:
        en = max(en, st + 1)
        win = A[0:min(5, U), st:en]
        if win.shape[0] == 0 or win.shape[1] == 0:
            out.append(-1)
        else:
            out.append(int(np.argmax(np.max(win, axis=1))))
    return out


def pred_frames_markup(A, P, frames):
    """get_binf_markup_frames of the rows segments_to_attention chose."""
    F = P.shape[1]
    rows = np.zeros((len(frames), F), dtype=np.uint8)
    for k, r in enumerate(markup_phones(A, frames)):
        if r >= 0:
            rows[k] = P[r] != 0
    return markup_frames_binf(frames, rows)


def count(pred, tgt):
    """The reference's clipping to the shorter of the two, then per-feature counts of equal frames: (counts, frames)."""
    n = min(pred.shape[0], tgt.shape[0])
    return np.sum(np.equal(pred[:n], tgt[:n]), axis=0).astype(np.int64), n


def sigmoid_rows(logits_binf):
    """--use_phones_from_binf: np.round(1 / (1 + np.exp(-logits[:-1]))) in float32."""
    logits = np.asarray(logits_binf, dtype=np.float32)[:-1, :]
    with np.errstate(over='ignore'):
        return (np.round(1 / (1 + np.exp(-logits))) != 0).astype(np.uint8)
