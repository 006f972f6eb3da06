"""The GPU resampler (csrc/resample.hip through audio.resample / resample_batch) against the NumPy restatement of resampy 0.2.2's
kaiser_best arithmetic (tests/resample_restated.py): bit for bit at every rate and at lengths shorter than a wing, batch =
per item, the running time register after 10 min, and two anchors that do not depend on the restatement (the DC gain the
truncated table stride gives, an upsampled sine)."""
import numpy as np
import pytest
import torch

from phones_las_amd import audio
from tests import resample_restated as R

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)


def _signal(n, sr, seed, stereo=False):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    chans = []
    for c in range(2 if stereo else 1):
        f = rng.uniform(100, 0.45 * sr, size=3)
        x = sum(0.3 * np.sin(2 * np.pi * fi * t + rng.uniform(0, 6)) for fi in f) + 0.05 * rng.standard_normal(n)
        chans.append(x.astype(np.float32))
    return audio.to_mono(np.stack(chans)) if stereo else chans[0]


@pytest.mark.parametrize('sr', RATES)
@pytest.mark.parametrize('stereo', [False, True])
def test_bit_identical_to_the_restatement(sr, stereo):
    x = _signal(2 * sr, sr, seed=sr + stereo, stereo=stereo)
    got = audio.resample(x, sr, 16000).cpu().numpy()
    ref = R.resample(x, sr, 16000, audio.kaiser_best_table())
    assert got.dtype == np.float32 and got.shape == ref.shape == (32000,)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize('sr', RATES)
def test_short_signals(sr):
    h = audio.kaiser_best_table()
    padded = 0
    for n in (1, 2, 10, 100, 190):
        nv, nf = audio.output_length(n, sr, 16000)
        x = _signal(n, sr, seed=n)
        if nv < 1:
            with pytest.raises(ValueError):
                audio.resample(x, sr, 16000)
            continue
        got = audio.resample(x, sr, 16000).cpu().numpy()
        ref = R.resample(x, sr, 16000, h)
        assert got.shape == (nf,) and np.array_equal(got, ref), n
        if nf > nv:
            padded += 1
            assert got[-1] == 0.0
    if sr in (22050, 44100, 48000, 96000):
        assert padded > 0                # ceil > int at some of these lengths: the fix_length zero is checked


def test_against_the_scipy_table():
    x = _signal(2 * 44100, 44100, seed=9)
    got = audio.resample(x, 44100, 16000).cpu().numpy()
    ref = R.resample(x, 44100, 16000, R.kaiser_table_scipy())
    assert np.abs(got - ref).max() <= 1e-6


def test_passthrough_is_unchanged():
    x = _signal(16000, 16000, seed=1)
    got = audio.resample(x, 16000, 16000)
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), x)
    xd = torch.from_numpy(x).cuda()
    assert audio.resample(xd, 16000, 16000).data_ptr() == xd.data_ptr()


def test_batch_is_per_item():
    rng = np.random.default_rng(64)
    srs = [int(s) for s in rng.choice([8000, 16000, 22050, 44100, 48000, 96000, 11025], size=64)]
    waves = [_signal(int(rng.integers(200, 3 * s)), s, seed=i) for i, s in enumerate(srs)]
    waves[3] = torch.from_numpy(waves[3]).cuda()             # numpy, CPU and CUDA inputs mix
    waves[5] = torch.from_numpy(waves[5])
    assert 16000 in srs
    batch = audio.resample_batch(waves, srs, 16000)
    assert len(batch) == 64
    for w, s, b in zip(waves, srs, batch):
        one = audio.resample(w, s, 16000)
        assert b.is_cuda and b.dtype == torch.float32 and torch.equal(b, one)


def test_drift_after_ten_minutes():
    sr = 44100
    n = 600 * sr
    x = _signal(n, sr, seed=600)
    nv, nf = audio.output_length(n, sr, 16000)
    got = audio.resample(x, sr, 16000).cpu().numpy()
    assert got.shape == (nf,)
    idx = np.arange(nv - 4096, nv)
    ratio = 16000.0 / sr
    tr = R.time_register(nv, ratio)
    ref = R.resample(x, sr, 16000, audio.kaiser_best_table(), idx=idx, tr=tr)
    assert np.array_equal(got[idx], ref)
    # teeth: t * inc instead of the running sum would put some of these outputs elsewhere (n or the table offset)
    naive = idx * (1.0 / ratio)
    scale = min(1.0, ratio)
    off = lambda r: (scale * (r - np.floor(r)) * 512).astype(np.int64)
    assert np.any(np.floor(naive) != np.floor(tr[idx])) or np.any(off(naive) != off(tr[idx]))


@pytest.mark.parametrize('sr,gain', [(48000, 1.00272), (44100, 1.00274), (22050, 1.00057)])
def test_dc_gain_of_the_truncated_stride(sr, gain):
    y = audio.resample(np.ones(sr, np.float32), sr, 16000).cpu().numpy()
    inner = y[4000:12000]
    assert abs(float(inner.max()) - gain) <= 1e-4            # the peak gain of the interior
    assert 1.0 < float(inner.min()) <= float(inner.max())


def test_upsampled_sine_is_the_sine():
    x = np.sin(2 * np.pi * 1000 * np.arange(16000) / 8000).astype(np.float32)
    y = audio.resample(x, 8000, 16000).cpu().numpy()
    ref = np.sin(2 * np.pi * 1000 * np.arange(32000) / 16000)
    assert y.shape == (32000,)
    assert np.abs(y[2000:30000] - ref[2000:30000]).max() <= 1e-6
