"""Any-rate audio through the CLIs on the GPU: preprocess_all on a corpus that mixes a 48-kHz stereo WAV, a 44.1-kHz 24-bit WAV,
a NIST SPHERE file and a 16-kHz PCM16 WAV (features = the front-end of audio.load of each file; the 16-kHz record byte-equal to
what the 16-kHz-only loader gave), and transcribe_audio_file.py against infer.py --batch_size 1 on a model train.py trained."""
import ast
import os
import struct
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORDS = ['ba', 'di', 'gu', 'ko']
TONES = {'ba': 300.0, 'di': 700.0, 'gu': 1300.0, 'ko': 2300.0}


def _speech(words, sr, seed, seg=0.12):
    """A tone per word (a 'phone' the model can tell apart), a little noise: float64 in [-0.5, 0.5]."""
    rng = np.random.default_rng(seed)
    n = int(seg * sr)
    t = np.arange(n) / sr
    x = np.concatenate([0.4 * np.sin(2 * np.pi * TONES[w] * t + rng.uniform(0, 6)) for w in words])
    return x + 0.01 * rng.standard_normal(len(x))


def _write_pcm16(path, x, sr, channels=1):
    s = np.clip(np.round(x * 32767), -32768, 32767).astype('<i2')
    if channels > 1:
        s = np.stack([s, (s // 2).astype('<i2')], 1)[:, :channels]
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(s.tobytes())


def _write_pcm24(path, x, sr):
    s = np.clip(np.round(x * (2 ** 23 - 1)), -2 ** 23, 2 ** 23 - 1).astype(np.int64) & 0xFFFFFF
    payload = np.stack([s & 255, (s >> 8) & 255, (s >> 16) & 255], 1).astype(np.uint8).tobytes()
    fmt = struct.pack('<HHIIHH', 1, 1, sr, sr * 3, 3, 24)
    body = b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'data' + struct.pack('<I', len(payload)) + payload
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<I', 4 + len(body)) + b'WAVE' + body)


def _write_sphere(path, x, sr):
    s = np.clip(np.round(x * 32767), -32768, 32767).astype('<i2')
    head = ('NIST_1A\n   1024\nsample_count -i %d\nsample_rate -i %d\nchannel_count -i 1\nsample_n_bytes -i 2\n'
            'sample_byte_format -s2 01\nsample_coding -s3 pcm\nsample_sig_bits -i 16\nend_head\n' % (len(s), sr)).encode()
    with open(path, 'wb') as f:
        f.write(head + b' ' * (1024 - len(head)) + s.tobytes())


def _corpus(d, n_each=2, seed=0):
    """Files of the four kinds, n_each of each; returns the CSV lines (path,lang,text)."""
    rng = np.random.default_rng(seed)
    lines = []
    kinds = [('wav48', 48000), ('wav441', 44100), ('sph', 16000), ('wav16', 16000)]
    for i in range(n_each):
        for kind, sr in kinds:
            words = [WORDS[int(k)] for k in rng.integers(0, len(WORDS), size=int(rng.integers(2, 5)))]
            x = _speech(words, sr, seed=100 * i + sr)
            p = os.path.join(d, '%s_%d.%s' % (kind, i, 'sph' if kind == 'sph' else 'wav'))
            if kind == 'wav48':
                _write_pcm16(p, x, sr, channels=2)
            elif kind == 'wav441':
                _write_pcm24(p, x, sr)
            elif kind == 'sph':
                _write_sphere(p, x, sr)
            else:
                _write_pcm16(p, x, sr)
            lines.append('%s,en,%s' % (p, ' '.join(words)))
    return lines


def _old_read_wav(path):
    """The 16-kHz-only loader preprocess_all had before any-rate decoding."""
    with wave.open(path, 'rb') as w:
        assert w.getframerate() == 16000 and w.getsampwidth() == 2
        data = np.frombuffer(w.readframes(w.getnframes()), dtype='<i2').astype(np.float32) / 32768.0
        if w.getnchannels() > 1:
            data = data.reshape(-1, w.getnchannels()).mean(1)
    return data


def test_preprocess_all_mixed_rates(tmp_path):
    import preprocess_all
    from phones_las_amd import audio, frontend
    from phones_las_amd.utils import tfrecord
    d = str(tmp_path)
    lines = _corpus(d, n_each=1)
    open(d + '/list.csv', 'w').write('\n'.join(lines) + '\n')
    args = preprocess_all.parse_args(['--input_file', d + '/list.csv', '--output_file', d + '/train.tfr', '--save_norm'])
    assert preprocess_all.main(args) == 4
    recs = list(tfrecord.tf_record_iterator(d + '/train.tfr', verify=True))
    assert len(recs) == 4
    for line, rec in zip(lines, recs):
        path, _, text = line.split(',')
        y, sr = audio.load(path)
        assert sr == 16000
        want = frontend.calculate_acoustic_features(args, y).cpu().numpy()
        x, labels = tfrecord.parse_sequence_example(rec, want.shape[1])
        assert labels == text.split()
        assert x.shape == want.shape and np.array_equal(x, want), path
        if path.endswith('wav16_0.wav'):
            old = frontend.calculate_acoustic_features(args, _old_read_wav(path)).cpu().numpy()
            assert rec == tfrecord.make_example(old, text.split())
    # the resampled signals did go through the kernel: a 48-kHz file has a third of the samples at 16 kHz
    y48, _ = audio.load(lines[0].split(',')[0])
    assert y48.numel() == int(np.ceil(len(audio.read(lines[0].split(',')[0])[0][0]) / 3))


def test_transcribe_matches_infer(tmp_path, capsys):
    import infer
    import preprocess_all
    import train
    import transcribe_audio_file as tr
    from joblib import load
    d = str(tmp_path)
    lines = _corpus(d, n_each=4, seed=1)
    open(d + '/list.csv', 'w').write('\n'.join(lines) + '\n')
    preprocess_all.main(preprocess_all.parse_args(['--input_file', d + '/list.csv', '--output_file', d + '/train.tfr',
                                                   '--save_norm', '--save_vocab']))
    train.main(train.parse_args(['--train', d + '/train.tfr', '--model_dir', d + '/model', '--encoder_layers', '2', '--encoder_units', '64',
                                 '--decoder_layers', '1', '--decoder_units', '64', '--use_pyramidal', '--bottom_only',
                                 '--pass_hidden_state', '--dropout', '0', '--sampling_probability', '0', '--batch_size', '16',
                                 '--num_channels', '13', '--learning_rate', '0.003', '--num_epochs', '60']))
    capsys.readouterr()
    wav48 = lines[0].split(',')[0]
    assert wav48.endswith('wav48_0.wav')
    open(d + '/one.csv', 'w').write(lines[0] + '\n')
    preprocess_all.main(preprocess_all.parse_args(['--input_file', d + '/one.csv', '--output_file', d + '/one.tfr']))
    common = ['--vocab', d + '/vocab.txt', '--norm', d + '/norm.dmp', '--model_dir', d + '/model']
    for beam in ('0', '3'):
        infer.main(infer.parse_args(['--data', d + '/one.tfr', '--num_channels', '13', '--batch_size', '1', '--beam_width', beam] + common))
        want = open(d + '/model/infer.txt').read().split('\n')[0]
        capsys.readouterr()
        out_file = d + '/pred%s.dmp' % beam
        preds = tr.main(tr.parse_args(['--waveform', wav48, '--beam_width', beam, '--output_file', out_file] + common))
        out = capsys.readouterr().out.strip().split('\n')
        assert 'sample_ids: ' in '\n'.join(out)
        printed = ast.literal_eval(out[-2])
        assert out[-1] == 'Predictions are saved to %s' % out_file
        assert ' '.join(printed) == want, (printed, want)
        back = load(out_file)
        assert len(back) == 1 and set(back[0]) == set(preds[0]) and np.array_equal(back[0]['sample_ids'], preds[0]['sample_ids'])
        if beam == '3':
            assert back[0]['sample_ids'].ndim == 2 and back[0]['sample_ids'].shape[1] == 3
    # several files: one block per file, each what a run on that file alone prints
    capsys.readouterr()
    paths = [l.split(',')[0] for l in lines[:4]]
    tr.main(tr.parse_args(['--waveform'] + paths + common))
    blocks = [ast.literal_eval(l) for l in capsys.readouterr().out.strip().split('\n') if l.startswith('[')]
    assert len(blocks) == 4
    for p, b in zip(paths, blocks):
        tr.main(tr.parse_args(['--waveform', p] + common))
        assert ast.literal_eval(capsys.readouterr().out.strip().split('\n')[-1]) == b
