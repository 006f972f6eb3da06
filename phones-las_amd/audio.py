"""Audio input: what ``librosa.load(path, sr=16000, mono=True)`` (librosa 0.7.1) does in the reference's preprocess_all.py:61,
transcribe_audio_file.py:97 and infer.py:177, for the containers the reference's recipes use.

  * ``read(path)``: RIFF WAV (PCM 8/16/24/32-bit, IEEE float 32/64-bit, WAVE_FORMAT_EXTENSIBLE of either) and NIST SPHERE
    (TIMIT; PCM, 2/3/4-byte samples, either byte order) decoded on the host to float32 as libsndfile does it when soundfile
    reads with dtype=float32: 8-bit (u - 128) / 128, 16-bit s / 2^15, 24-bit s / 2^23 (exact), 32-bit float32(s) * 2^-31 (the
    int -> float rounding first), float as stored, double rounded to float.  [N] for one channel, [C, N] for more.
  * ``to_mono(y)``: librosa 0.7.1's to_mono, the channels summed in order in float32 and divided by C.
  * ``resample(y, orig_sr, target_sr)`` / ``resample_batch``: librosa 0.7.1's resample with res_type 'kaiser_best', i.e.
    resampy 0.2.2's band-limited sinc interpolation, on the GPU (csrc/resample.hip, one launch per batch), then fix_length to
    ceil(len * ratio).  The arithmetic is restated from the published source of those releases (neither package is a
    dependency): every operation of resampy's resample_f is a separately rounded float64 operation and the output is float32
    storage; the kernel reproduces that order exactly.  Parity against librosa / resampy / libsndfile themselves is UNPINNED.
  * ``load(path, sr=16000, mono=True)``: the three above in librosa's order.

Two properties of resampy 0.2.2 are kept on purpose (tests pin both):
  * integer table stride: index_step = int(scale * 512) truncates (170 instead of 170.67 at 48 kHz -> 16 kHz), so the DC gain
    is not 1 (1.00272 at 48 kHz, 1.00274 at 44.1 kHz, 1.00057 at 22.05 kHz);
  * drifting time register: the input position is a running float64 sum of 1 / ratio, not t / ratio (later resampy releases
    compute it from t); after 10 min at 44.1 kHz the sum is 0.0036 input samples away from t * inc, which shows in the output.
    The kernel evaluates the running sum in closed form (``time_segments``), bit for bit.

Compressed formats (mp3 / flac / ogg) are out of scope: no decoder is a dependency of this project."""
import functools
import math
import struct

import numpy as np
import torch

from . import hip

__all__ = ['read', 'to_mono', 'load', 'resample', 'resample_batch', 'kaiser_best_table', 'output_length', 'time_segments',
           'KAISER_BEST']

# ---- containers ----------------------------------------------------------------------------------------------------------
WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_ALAW, WAVE_FORMAT_MULAW, WAVE_FORMAT_EXTENSIBLE = 1, 3, 6, 7, 0xFFFE
_KSDATAFORMAT_TAIL = b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'     # bytes 2..15 of the sub-format GUIDs


def _pcm_to_float(raw, width, order='<'):
    """Interleaved integer PCM of `width` bytes -> float32, libsndfile's scaling for dtype=float32."""
    if width == 1:
        u = np.frombuffer(raw, dtype=np.uint8)
        return (u.astype(np.int16) - 128).astype(np.float32) * np.float32(1.0 / 128)
    if width == 2:
        return np.frombuffer(raw, dtype=order + 'i2').astype(np.float32) * np.float32(1.0 / 32768)
    if width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        if order == '>':
            b = b[:, ::-1]
        s = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        s = np.where(s >= 1 << 23, s - (1 << 24), s)
        return s.astype(np.float32) * np.float32(2.0 ** -23)
    if width == 4:
        return np.frombuffer(raw, dtype=order + 'i4').astype(np.float32) * np.float32(2.0 ** -31)
    raise ValueError('%d-byte PCM samples are not decoded' % width)


def _shape(flat, channels):
    n = flat.size // channels
    flat = flat[:n * channels]
    if channels == 1:
        return np.ascontiguousarray(flat)
    return np.ascontiguousarray(flat.reshape(n, channels).T)


def _read_riff(path, data):
    if len(data) < 12 or data[8:12] != b'WAVE':
        raise ValueError('%s: RIFF file without a WAVE form' % path)
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack('<I', data[pos + 4:pos + 8])[0]
        body = pos + 8
        if cid == b'data':
            end = len(data) if size in (0, 0xFFFFFFFF) else min(len(data), body + size)
            payload = data[body:end]
            if fmt is not None:
                break
        elif cid == b'fmt ':
            fmt = data[body:body + size]
        if size in (0xFFFFFFFF,):
            break
        pos = body + size + (size & 1)              # chunks are padded to an even size
    if fmt is None or len(fmt) < 16:
        raise ValueError('%s: WAV without a fmt chunk' % path)
    if payload is None:
        raise ValueError('%s: WAV without a data chunk' % path)
    tag, channels, sr, _, block_align, bits = struct.unpack('<HHIIHH', fmt[:16])
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 40 or fmt[26:40] != _KSDATAFORMAT_TAIL:
            raise ValueError('%s: WAVE_FORMAT_EXTENSIBLE with an unknown sub-format GUID' % path)
        tag = struct.unpack('<H', fmt[24:26])[0]
    if channels < 1:
        raise ValueError('%s: WAV with %d channels' % (path, channels))
    width = (bits + 7) // 8
    if tag == WAVE_FORMAT_PCM:
        if width not in (1, 2, 3, 4):
            raise ValueError('%s: %d-bit PCM WAV is not decoded' % (path, bits))
        payload = payload[:len(payload) // width * width]
        y = _pcm_to_float(payload, width)
    elif tag == WAVE_FORMAT_IEEE_FLOAT:
        if bits not in (32, 64):
            raise ValueError('%s: %d-bit float WAV is not decoded' % (path, bits))
        payload = payload[:len(payload) // width * width]
        y = np.frombuffer(payload, dtype='<f4' if bits == 32 else '<f8').astype(np.float32)
    elif tag in (WAVE_FORMAT_MULAW, WAVE_FORMAT_ALAW):
        raise ValueError('%s: %s WAV (format tag %d) is not decoded' % (path, 'mu-law' if tag == WAVE_FORMAT_MULAW else 'A-law', tag))
    else:
        raise ValueError('%s: WAV format tag 0x%04X is not decoded' % (path, tag))
    return _shape(y, channels), sr


_SPHERE_ORDER = {'01': '<', '10': '>', '012': '<', '210': '>', '0123': '<', '3210': '>'}


def _read_sphere(path, data):
    lines = data[:1024 * 64].split(b'\n')
    try:
        header_size = int(lines[1].strip())
    except (IndexError, ValueError):
        raise ValueError('%s: NIST SPHERE header without its size on line 2' % path)
    fields = {}
    for ln in data[:header_size].split(b'\n')[2:]:
        parts = ln.decode('latin-1').strip().split(None, 2)
        if not parts or parts[0] == 'end_head':
            if parts:
                break
            continue
        if len(parts) == 3:
            kind, value = parts[1], parts[2]
            fields[parts[0]] = int(value) if kind == '-i' else float(value) if kind == '-r' else value
    coding = str(fields.get('sample_coding', 'pcm'))
    if coding != 'pcm':
        raise ValueError('%s: NIST SPHERE sample_coding %r is not decoded' % (path, coding))
    width = int(fields.get('sample_n_bytes', 2))
    if width not in (2, 3, 4):
        raise ValueError('%s: NIST SPHERE sample_n_bytes %d is not decoded' % (path, width))
    fmt = str(fields.get('sample_byte_format', ''))
    if fmt not in _SPHERE_ORDER:
        raise ValueError('%s: NIST SPHERE sample_byte_format %r is not decoded' % (path, fmt))
    channels = int(fields.get('channel_count', 1))
    if 'sample_rate' not in fields or channels < 1:
        raise ValueError('%s: NIST SPHERE header without sample_rate / channel_count' % path)
    payload = data[header_size:]
    n = len(payload) // (width * channels)
    if 'sample_count' in fields:
        n = min(n, int(fields['sample_count']))
    y = _pcm_to_float(payload[:n * width * channels], width, _SPHERE_ORDER[fmt])
    return _shape(y, channels), int(fields['sample_rate'])


def read(path):
    """Decode a RIFF WAV or NIST SPHERE file -> (float32 [N] or [C, N], native sample rate)."""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:4] == b'RIFF':
        return _read_riff(path, data)
    if data[:8] == b'NIST_1A\n':
        return _read_sphere(path, data)
    raise ValueError('%s: neither RIFF WAV nor NIST SPHERE (starts with %r)' % (path, data[:8]))


def to_mono(y):
    """librosa 0.7.1 to_mono: [C, N] -> [N], channels summed in order in float32, then divided by C."""
    y = np.asarray(y, dtype=np.float32)
    if y.ndim == 1:
        return y
    s = y[0].copy()
    for c in range(1, y.shape[0]):
        s += y[c]
    return s / np.float32(y.shape[0])


# ---- resampy 0.2.2 kaiser_best ---------------------------------------------------------------------------------------------
KAISER_BEST = {'num_zeros': 64, 'precision': 9, 'beta': 14.769656459379492, 'rolloff': 0.9475937167399596}
NUM_TABLE = 2 ** KAISER_BEST['precision']


@functools.lru_cache(maxsize=1)
def kaiser_best_table():
    """resampy.filters.sinc_window(64, 9, kaiser(beta), rolloff) in float64: the UNSCALED half window, 32 769 entries
    (read-only: resample scales a copy of it, or the kernel scales on the fly)."""
    nz, rolloff, beta = KAISER_BEST['num_zeros'], KAISER_BEST['rolloff'], KAISER_BEST['beta']
    n = NUM_TABLE * nz
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, nz, num=n + 1, endpoint=True))
    half = np.kaiser(2 * n + 1, beta)[n:] * sinc_win
    half.setflags(write=False)
    return half


@functools.lru_cache(maxsize=1)
def _device_table():
    # one extra entry equal to the last: delta = w[k + 1] - w[k] of the last entry is then exactly 0, as resampy's is
    h = kaiser_best_table()
    return torch.tensor(np.concatenate([h, h[-1:]]), dtype=torch.float64, device='cuda')


def output_length(n, orig_sr, target_sr):
    """(resampy's output length int(n * ratio), librosa's fix_length target int(ceil(n * ratio)))."""
    ratio = float(target_sr) / orig_sr
    return int(n * ratio), int(math.ceil(n * ratio))


def time_segments(n_out, ratio):
    """resampy 0.2.2's time register tr_t (tr_0 = 0, tr_{t+1} = fl(tr_t + 1/ratio)) as segments (t_b, start_b, step_b):
    tr_t = start_b + (t - t_b) * step_b for t_b <= t < t_{b+1}, every operation exact.

    Inside one binade [2^e, 2^(e+1)) the register is a multiple of that binade's ulp u, and fl(tr + inc) adds round(inc / u) ulps
    -- unless inc / u ends in exactly one half (a tie): round-half-even then adds floor or floor + 1 depending on the parity of
    the register, and after at most one step that parity is the one that keeps the step constant.  So a binade is one segment,
    preceded by a one-step segment where the first step differs; the step across a binade boundary is taken with the float64
    addition itself.  About 2 log2(n_out) segments."""
    inc = 1.0 / ratio
    seg_t, seg_tr, seg_step = [], [], []
    t, tr = 0, 0.0
    while t < n_out:
        if tr == 0.0:
            seg_t.append(t), seg_tr.append(tr), seg_step.append(0.0)
            t, tr = t + 1, tr + inc
            continue
        e = math.frexp(tr)[1] - 1                     # tr in [2^e, 2^(e+1))
        top = math.ldexp(1.0, e + 1)
        nxt = tr + inc
        if nxt >= top:                                # the next value is already in the next binade
            seg_t.append(t), seg_tr.append(tr), seg_step.append(0.0)
            t, tr = t + 1, nxt
            continue
        s = nxt - tr                                  # exact: both are multiples of u below 2^(e+1)
        nxt2 = nxt + inc
        if nxt2 < top and nxt2 - nxt != s:            # a tie whose first step differs: a segment of its own
            seg_t.append(t), seg_tr.append(tr), seg_step.append(0.0)
            t, tr = t + 1, nxt
            continue
        u = math.ldexp(1.0, e - 52)
        span = int((top - tr) / u)                    # ulps to the top of the binade (exact integers)
        k = -(-span // int(s / u))                    # values tr + j s below 2^(e+1): j = 0 .. k-1
        k = min(k, n_out - t)
        seg_t.append(t), seg_tr.append(tr), seg_step.append(s)
        tr = (tr + (k - 1) * s) + inc                 # the step out of the binade: the float64 addition itself
        t += k
    return np.array(seg_t, dtype=np.int64), np.array(seg_tr, dtype=np.float64), np.array(seg_step, dtype=np.float64)


def time_register(seg, n_out):
    """Evaluate the segments on the host (tests): tr_t for t < n_out, float64."""
    seg_t, seg_tr, seg_step = seg
    t = np.arange(n_out, dtype=np.int64)
    b = np.searchsorted(seg_t, t, side='right') - 1
    return seg_tr[b] + (t - seg_t[b]).astype(np.float64) * seg_step[b]


def _as_f32_vector(y):
    if isinstance(y, torch.Tensor):
        w = y.detach().to(torch.float32).reshape(-1)
    else:
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(y, dtype=np.float32).reshape(-1)))
    return w


def resample_batch(waves, srs, target_sr):
    """librosa 0.7.1 resample(y, sr, target_sr, res_type='kaiser_best') of every wave (mono; numpy, CPU or CUDA) in ONE kernel
    launch; waves at target_sr are returned unchanged.  Returns a list of CUDA float32 tensors (views of one buffer)."""
    if len(waves) != len(srs):
        raise ValueError('resample_batch: %d waves, %d rates' % (len(waves), len(srs)))
    if not len(waves):
        return []
    plan = batch_plan(waves, srs, target_sr)
    launch(plan)
    oo = plan['out_off']
    return [plan['y'][oo[u]:oo[u + 1]] for u in range(len(oo) - 1)]


def batch_plan(waves, srs, target_sr):
    """The operands of one las_resample_batch launch, on the device: the signals back to back, offsets, per-utterance
    ratio and output counts, the time-register segments, the output buffer (scripts/gpu_resample_rate.py times launch())."""
    ws = [_as_f32_vector(w) for w in waves]
    lens = [int(w.numel()) for w in ws]
    n_valid, n_fix, ratios = [], [], []
    segs = {}
    for n, sr in zip(lens, srs):
        if sr <= 0 or target_sr <= 0:
            raise ValueError('sample rates must be positive (got %r -> %r)' % (sr, target_sr))
        if n >= 1 << 31:
            raise ValueError('resample_batch: a signal of %d samples (2^31 or more) is not resampled in one piece' % n)
        if sr == target_sr:                           # librosa returns y itself
            n_valid.append(n), n_fix.append(n), ratios.append(1.0)
            continue
        nv, nf = output_length(n, sr, target_sr)
        if nv < 1:
            raise ValueError('Input signal length=%d is too small to resample from %s->%s' % (n, sr, target_sr))
        n_valid.append(nv), n_fix.append(nf), ratios.append(float(target_sr) / sr)
    seg_t, seg_tr, seg_step, seg_off = [], [], [], [0]
    for nv, r, sr in zip(n_valid, ratios, srs):
        if sr == target_sr:
            s = (np.zeros(1, np.int64), np.zeros(1), np.zeros(1))
        else:
            if (r, nv) not in segs:
                segs[(r, nv)] = time_segments(nv, r)
            s = segs[(r, nv)]
        seg_t.append(s[0]), seg_tr.append(s[1]), seg_step.append(s[2])
        seg_off.append(seg_off[-1] + len(s[0]))
    dev = 'cuda'
    if all(w.is_cuda for w in ws):
        flat = torch.cat(ws) if len(ws) > 1 else ws[0].contiguous()
    else:
        host = torch.empty(sum(lens), dtype=torch.float32, pin_memory=True)     # one copy into pinned memory, one upload
        o = 0
        for w, n in zip(ws, lens):
            host[o:o + n].copy_(w.cpu())
            o += n
        flat = host.to(dev, non_blocking=True)
    if flat.numel() == 0:
        flat = torch.zeros(1, dtype=torch.float32, device=dev)
    out_off = np.concatenate([[0], np.cumsum(n_fix)]).astype(np.int64)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    total = int(out_off[-1])
    return {'x': flat, 'in_off': i64(np.concatenate([[0], np.cumsum(lens)])), 'd_out_off': i64(out_off), 'n_valid': i64(n_valid),
            'ratio': f64(ratios), 'seg_off': torch.tensor(seg_off, dtype=torch.int32, device=dev),
            'seg_t': i64(np.concatenate(seg_t)), 'seg_tr': f64(np.concatenate(seg_tr)), 'seg_step': f64(np.concatenate(seg_step)),
            'half': _device_table(), 'n_utt': len(ws), 'total': total, 'out_off': out_off.tolist(),
            'y': torch.empty(max(total, 1), dtype=torch.float32, device=dev)}


def launch(plan):
    """One las_resample_batch launch of a batch_plan on torch's current stream."""
    if not plan['total']:
        return
    P = plan
    hip.check(hip.lib().las_resample_batch(hip.p(P['x']), hip.p(P['in_off']), hip.p(P['d_out_off']), hip.p(P['n_valid']),
                                           hip.p(P['ratio']), hip.p(P['seg_off']), hip.p(P['seg_t']), hip.p(P['seg_tr']),
                                           hip.p(P['seg_step']), hip.p(P['half']), int(P['half'].numel()) - 1, P['n_utt'],
                                           P['total'], hip.p(P['y']), hip.stream()))


def resample(y, orig_sr, target_sr):
    """librosa 0.7.1 resample(y, orig_sr, target_sr, res_type='kaiser_best') of one mono signal -> CUDA float32 tensor."""
    if orig_sr == target_sr:
        w = _as_f32_vector(y)
        return w if w.is_cuda else w.cuda()
    return resample_batch([y], [orig_sr], target_sr)[0]


def load(path, sr=16000, mono=True, res_type='kaiser_best'):
    """librosa 0.7.1 load (whole file, no offset / duration): decode, to_mono, resample to `sr` (None: the native rate).
    Returns (y, sr): y is the decoded numpy array when no resampling happens, a CUDA float32 tensor when it does."""
    if res_type != 'kaiser_best':
        raise ValueError("only res_type='kaiser_best' is provided (got %r)" % (res_type,))
    y, sr_native = read(path)
    if mono:
        y = to_mono(y)
    if sr is None or sr == sr_native:
        return y, sr_native
    if y.ndim != 1:
        raise ValueError('resampling keeps one channel: load with mono=True')
    return resample(y, sr_native, sr), sr
