"""The arithmetic of resampy 0.2.2's resample_f (kaiser_best, as librosa 0.7.1's resample calls it) restated in NumPy, vectorised
over output samples and looped over taps, with every operation a separately rounded float64 operation and the output float32
storage.  Independent of the product: the time register is the sequential running sum (np.cumsum), not the product's segment
table, and the window / differences are formed here from whatever half window the caller passes.  Used by the GPU tests."""
import math

import numpy as np

NUM_TABLE = 512


def time_register(n_out, ratio):
    """tr_0 = 0, tr_{t+1} = fl(tr_t + 1/ratio): numpy's cumsum adds sequentially."""
    a = np.full(n_out, 1.0 / ratio)
    a[0] = 0.0
    return np.cumsum(a)


def resample(x, sr_orig, sr_new, half, idx=None, tr=None):
    """librosa.resample(x, sr_orig, sr_new, 'kaiser_best') with the half window `half` (float64, unscaled): the resampy output
    followed by fix_length's zero padding to ceil(len * ratio).  idx: compute only these output indices (returns those);
    tr: the time register of all int(len * ratio) outputs if already at hand."""
    x = np.asarray(x, dtype=np.float32)
    if sr_orig == sr_new:
        return x.copy() if idx is None else x[idx]
    ratio = float(sr_new) / sr_orig
    n_out = int(len(x) * ratio)
    n_fix = int(math.ceil(len(x) * ratio))
    if n_out < 1:
        raise ValueError('too short')
    win = half * ratio if ratio < 1 else half.copy()
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    nwin = len(win)
    scale = min(1.0, ratio)
    step = int(scale * NUM_TABLE)
    sel = np.arange(n_fix, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    valid = sel < n_out
    out = np.zeros(len(sel), dtype=np.float32)
    t = sel[valid]
    if tr is None:
        tr = time_register(n_out, ratio)
    r = tr[t]
    n = r.astype(np.int64)
    x64 = x.astype(np.float64)
    y = np.zeros(len(t), dtype=np.float32)
    frac = scale * (r - n)
    for side in (0, 1):
        if side:
            frac = scale - frac
        ix = frac * NUM_TABLE
        off = ix.astype(np.int64)
        eta = ix - off
        cnt = np.minimum(n + 1, (nwin - off) // step) if not side else np.minimum(len(x) - n - 1, (nwin - off) // step)
        for i in range(int(cnt.max(initial=0))):
            m = i < cnt
            o = off[m] + i * step
            w = win[o] + eta[m] * delta[o]
            src = n[m] - i if not side else n[m] + i + 1
            y[m] = (y[m].astype(np.float64) + w * x64[src]).astype(np.float32)
    out[valid] = y
    return out


def kaiser_table_scipy():
    """The half window built with scipy.signal.windows.kaiser, as resampy.filters does (for cross-checks)."""
    from scipy.signal.windows import kaiser
    nz, rolloff, beta = 64, 0.9475937167399596, 14.769656459379492
    n = NUM_TABLE * nz
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, nz, num=n + 1, endpoint=True))
    return kaiser(2 * n + 1, beta)[n:] * sinc_win
