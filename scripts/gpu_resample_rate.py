"""Throughput of the resampler (phones-las_amd/audio.resample_batch -> csrc/resample.hip, resampy 0.2.2 kaiser_best) on 64 seeded
8-s signals at 44.1 kHz and at 48 kHz: warm-up, then device events around REPS launches of the kernel alone (inputs, offsets and
segment tables already on the device): audio-seconds per second and microseconds per launch; the taps per output and the
resulting float64 tap rate.  Then one --gpu_batch group of preprocess_all at 48 kHz (64 x 8 s): the resampler's and the
front-end's share of the batch (device events around each).  Env: N (signals, default 64), SEC (seconds each, default 8),
REPS (default 20), OUT (a JSON file for the numbers; optional)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phones_las_amd import audio, frontend  # noqa: E402

N = int(os.environ.get('N', '64'))
SEC = float(os.environ.get('SEC', '8'))
REPS = int(os.environ.get('REPS', '20'))


def signals(sr, seed):
    rng = np.random.default_rng(seed)
    n = int(SEC * sr)
    t = np.arange(n) / sr
    return [(0.3 * np.sin(2 * np.pi * rng.uniform(100, 4000) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
            for _ in range(N)]


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


res = {}
for sr in (44100, 48000):
    waves = [torch.from_numpy(w).cuda() for w in signals(sr, sr)]
    plan = audio.batch_plan(waves, [sr] * N, 16000)            # operands on the device once: the launches time the kernel
    for _ in range(3):
        audio.launch(plan)
    ms = events_ms(lambda: audio.launch(plan), REPS)
    n_out = plan['total']
    ratio = 16000.0 / sr
    step = int(min(1.0, ratio) * 512)
    taps = 2 * ((512 * 64 + 1) // step)          # about: both wings at full length
    rate = N * SEC / (ms / 1e3)
    res[str(sr)] = {'kernel_us': ms * 1e3, 'audio_seconds_per_s': rate, 'outputs': n_out, 'taps_per_output_approx': taps,
                    'gtaps_per_s': n_out * taps / (ms / 1e3) / 1e9}
    print('%d Hz -> 16 kHz: %d x %.0f s: %.1f us per launch = %.0f audio-seconds/s (%.0f x real time); ~%d taps per output, '
          '%.1f G taps/s' % (sr, N, SEC, ms * 1e3, rate, rate, taps, res[str(sr)]['gtaps_per_s']))

# one --gpu_batch group of preprocess_all at 48 kHz: resampler vs front-end (mfcc + energy + deltas)
args = argparse.Namespace(feature_type='mfcc', backend='librosa', n_mfcc=13, n_mels=40, window=20, step=10, energy=True, deltas=True)
host = signals(48000, 7)
for _ in range(2):
    frontend.calculate_acoustic_features_batch(args, audio.resample_batch(host, [48000] * N, 16000))
torch.cuda.synchronize()
ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
t_rs = t_fe = 0.0
for _ in range(3):
    ev[0].record()
    ys = audio.resample_batch(host, [48000] * N, 16000)          # includes the upload of the 48-kHz signals
    ev[1].record()
    frontend.calculate_acoustic_features_batch(args, ys)
    ev[2].record()
    torch.cuda.synchronize()
    t_rs += ev[0].elapsed_time(ev[1]) / 3
    t_fe += ev[1].elapsed_time(ev[2]) / 3
res['gpu_batch_48k'] = {'resample_ms': t_rs, 'frontend_ms': t_fe, 'resample_share': t_rs / (t_rs + t_fe)}
print('one --gpu_batch %d group at 48 kHz (%.0f s each): resample_batch %.2f ms (upload included), front-end %.2f ms: resampler '
      'share %.0f %%' % (N, SEC, t_rs, t_fe, 100 * t_rs / (t_rs + t_fe)))
# the whole of preprocess_all on one --gpu_batch group of 48-kHz WAV files (decode, resample, features, TFRecord): wall clock,
# and the resampling kernel's share of it
import tempfile  # noqa: E402
import time  # noqa: E402
import wave  # noqa: E402
import preprocess_all  # noqa: E402
with tempfile.TemporaryDirectory() as d:
    lines = []
    for i, w in enumerate(host):
        p = os.path.join(d, 'u%d.wav' % i)
        with wave.open(p, 'wb') as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(48000)
            f.writeframes((np.clip(w, -1, 1) * 32767).astype('<i2').tobytes())
        lines.append('%s,en,a b c' % p)
    open(os.path.join(d, 'list.csv'), 'w').write('\n'.join(lines) + '\n')
    pargs = ['--input_file', os.path.join(d, 'list.csv'), '--output_file', os.path.join(d, 'out.tfr'), '--deltas', '--energy',
             '--gpu_batch', str(N)]
    preprocess_all.main(preprocess_all.parse_args(pargs))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    preprocess_all.main(preprocess_all.parse_args(pargs))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
k_ms = res['48000']['kernel_us'] / 1e3
res['preprocess_all_48k'] = {'wall_ms': wall, 'resample_kernel_ms': k_ms, 'kernel_share': k_ms / wall}
print('preprocess_all, one --gpu_batch %d group of %.0f-s 48-kHz WAV files: %.1f ms wall; the resampling kernel %.2f ms of it '
      '(%.1f %%)' % (N, SEC, wall, k_ms, 100 * k_ms / wall))
if os.environ.get('OUT'):
    with open(os.environ['OUT'], 'w') as f:
        json.dump(res, f, indent=1)
