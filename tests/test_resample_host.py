"""Host side of the resampler (phones-las_amd/audio.py, csrc/resample.hip) without a GPU: the kaiser_best table, the closed form
of resampy's running time register against the sequential sum, the output lengths, and the gfx950 ISA of the kernel (no f64
FMA: resampy rounds the product and the sum separately)."""
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest

from phones_las_amd import audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000)


def _cumsum_register(n, ratio):
    a = np.full(n, 1.0 / ratio)
    a[0] = 0.0
    return np.cumsum(a)                  # numpy accumulates sequentially: resampy's `time_register += time_increment`


def test_table_matches_a_scipy_kaiser_construction():
    from scipy.signal.windows import kaiser
    h = audio.kaiser_best_table()
    n = 512 * 64
    assert h.dtype == np.float64 and h.shape == (n + 1,) and not h.flags.writeable
    r, beta = 0.9475937167399596, 14.769656459379492
    ref = kaiser(2 * n + 1, beta)[n:] * (r * np.sinc(r * np.linspace(0, 64, n + 1)))
    assert np.abs(h - ref).max() <= 1e-15
    assert h[0] == pytest.approx(r, abs=1e-15) and abs(h[-1]) < 1e-7


@pytest.mark.parametrize('sr', RATES)
def test_segments_reproduce_the_running_sum(sr):
    n = 10 ** 7
    ratio = 16000.0 / sr
    seg = audio.time_segments(n, ratio)
    assert len(seg[0]) <= 64
    assert np.array_equal(audio.time_register(seg, n), _cumsum_register(n, ratio))


def test_segments_reproduce_the_running_sum_at_random_rates():
    rng = np.random.default_rng(1234)
    ties = 0
    for sr in rng.integers(1000, 192001, size=200):
        ratio = 16000.0 / int(sr)
        n = 10 ** 6
        seg = audio.time_segments(n, ratio)
        got = audio.time_register(seg, n)
        ref = _cumsum_register(n, ratio)
        assert np.array_equal(got, ref), int(sr)
        # one-step segments inside a binade: the round-half-even ties of `tr + inc`
        e = np.frexp(seg[1])[1]
        ties += int(sum(1 for b in range(1, len(seg[0]) - 1) if seg[2][b] == 0.0 and e[b] == e[b + 1]))
    assert ties > 0                      # the seeded rates do hit the tie case


def test_drift_is_real():
    """After 10 min at 44.1 kHz the running sum is measurably away from t * inc (the quirk the kernel keeps)."""
    ratio = 16000.0 / 44100
    n = int(600 * 44100 * ratio)
    tr = audio.time_register(audio.time_segments(n, ratio), n)
    drift = np.abs(tr - np.arange(n) * (1.0 / ratio)).max()
    assert 1e-3 < drift < 1e-2, drift


def test_output_lengths():
    assert audio.output_length(48000, 48000, 16000) == (16000, 16000)
    assert audio.output_length(100, 44100, 16000) == (int(100 * (16000 / 44100)), int(np.ceil(100 * (16000 / 44100))))
    assert audio.output_length(100, 44100, 16000) == (36, 37)
    assert audio.output_length(3, 8000, 16000) == (6, 6)
    assert audio.output_length(1, 48000, 16000) == (0, 1)
    for n in (1, 2, 10, 100, 190):
        nv, nf = audio.output_length(n, 22050, 16000)
        assert nv == int(n * (16000 / 22050)) and nf == int(np.ceil(n * (16000 / 22050)))
    with pytest.raises(ValueError, match='too small'):
        audio.resample_batch([np.zeros(2, np.float32)], [48000], 16000)     # int(2 / 3) = 0 outputs: resampy refuses


def _asm(tmp_path):
    spec = importlib.util.spec_from_file_location('check_wide_polls', os.path.join(ROOT, 'scripts', 'check_wide_polls.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path = str(tmp_path / 'resample.s')
    mod.compile_to_asm(path, [], name='resample.hip')
    return open(path).read()


@pytest.mark.skipif(shutil.which(os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')) is None, reason='hipcc not installed')
def test_resample_kernel_has_no_f64_fma(tmp_path):
    text = _asm(tmp_path)
    m = re.search(r'^(_Z\w*resample_kernel\w*):[^\n]*$(.*?)^\s*s_endpgm', text, re.S | re.M)
    assert m, 'resample kernel not found in the assembly'
    body = m.group(2)
    assert 'v_mul_f64' in body and 'v_add_f64' in body and 'v_cvt_f32_f64' in body
    fma = re.findall(r'\bv_(?:fma|fmac|fmaak|fmamk)_f64\w*', body)
    assert not fma, fma
