"""infer.py --calc_frame_binf_accuracy end to end on the GPU: a tiny --binary_outputs --multitask model trained by train.py on
synthetic TIMIT-like files (NIST SPHERE and WAV, named .WAV, with .PHN markup beside them); the printed table must be the
restatement (tests/frame_binf_restated.py) applied to the same predict outputs, with and without --use_markup_segments."""
import os

import numpy as np
import pytest

import tests.frame_binf_restated as R
from tests.test_gpu_audio_cli import TONES, _write_pcm16, _write_sphere

pytestmark = pytest.mark.gpu

WORDS = ['ba', 'di', 'gu', 'ko', 'sil']
SEG = 0.12


def _speech(words, sr, seed):
    rng = np.random.default_rng(seed)
    n = int(SEG * sr)
    t = np.arange(n) / sr
    x = np.concatenate([np.zeros(n) if w == 'sil' else 0.4 * np.sin(2 * np.pi * TONES[w] * t + rng.uniform(0, 6)) for w in words])
    return x + 0.01 * rng.standard_normal(len(x))


def _corpus(d, n=12, seed=0):
    """CSV lines (path,lang,text) of n files, half SPHERE, half 16-kHz WAV, each with its .PHN (16-kHz sample positions; the
    silences labelled h# or pau, which the map folds)."""
    rng = np.random.default_rng(seed)
    lines = []
    for i in range(n):
        words = ['sil'] + [WORDS[int(k)] for k in rng.integers(0, 4, size=int(rng.integers(2, 5)))] + ['sil']
        x = _speech(words, 16000, seed=100 + i)
        p = os.path.join(d, 'S%02d.WAV' % i)
        (_write_sphere if i % 2 else _write_pcm16)(p, x, 16000)
        n16 = int(SEG * 16000)
        with open(p.replace('.WAV', '.PHN'), 'w') as f:
            for k, w in enumerate(words):
                lab = w if w != 'sil' else ('h#' if k == 0 else 'pau')
                jitter = int(rng.integers(-40, 40)) if 0 < k < len(words) - 1 else 0
                f.write('%d %d %s\n' % (k * n16 + (jitter if k else 0), (k + 1) * n16, lab))
        lines.append('%s,en,%s' % (p, ' '.join(words)))
    return lines


def _binf_csv(path, phones, nf=6, seed=3):
    rng = np.random.default_rng(seed)
    cols = []
    while len(cols) < len(phones):
        c = tuple(int(v) for v in rng.integers(0, 2, nf))
        if c not in cols and any(c):
            cols.append(c)
    with open(path, 'w') as f:
        f.write(',' + ','.join(phones) + '\n')
        for k in range(nf):
            f.write('f%d,' % k + ','.join(str(c[k]) for c in cols) + '\n')


def _expected(preds, lines, table, mapping, markup_segments, step, from_binf=False):
    """The reference's loop (infer.py:305-343) restated on the captured predict outputs: the hypothesis' table columns and
    its 'alignment' rows, or (from_binf: --use_phones_from_binf) the rounded sigmoids of logits_binf[:-1] and
    alignment_binf[:S-1]."""
    from phones_las_amd import audio
    from phones_las_amd.utils import EOS_ID
    F = len(table.index)
    correct = np.zeros(F, dtype=np.int64)
    frames = 0
    warnings = []
    k = 0
    for pred in preds:
        ids, align = pred['sample_ids'].astype(np.int64), pred.get('alignment')
        for b in range(ids.shape[0]):
            if k >= len(lines):
                break
            if from_binf:
                P = R.sigmoid_rows(pred['logits_binf'][b])
                A = pred['alignment_binf'][b, :P.shape[0], :]
            else:
                h = ids[b].tolist() + [EOS_ID]
                h = h[:h.index(EOS_ID)]
                P = (table.values[:, h] != 0).T.reshape(len(h), F).astype(np.uint8)
                A = align[b, :len(h), :]
            sound = lines[k].split(',')[0]
            segs, binfs = [], []
            for line in open(sound.replace('.WAV', '.PHN')).read().strip().split('\n'):
                st, en, ph = line.split()
                ph = mapping[ph] or 'sil'
                segs.append([int(st), int(en)])
                binfs.append(table[ph] != 0)
            y, _ = audio.load(sound, 16000)
            fr = R.time_to_frames(np.array(segs), int(y.shape[0]), step)
            tgt = R.markup_frames_binf(fr, np.array(binfs))
            pred_f = R.pred_frames_markup(A, P, fr) if markup_segments else R.pred_frames_dtw(A, P)
            if pred_f.shape[0] != tgt.shape[0]:
                warnings.append((pred_f.shape[0], tgt.shape[0]))
            c, n = R.count(pred_f, tgt)
            correct += c
            frames += n
            k += 1
    return correct / frames, warnings


KEYS = ('sample_ids', 'alignment', 'logits_binf', 'alignment_binf')


def _train(d, model_dir, binf, extra):
    import train
    train.main(train.parse_args(['--train', d + '/train.tfr', '--model_dir', model_dir, '--encoder_layers', '2',
                                 '--encoder_units', '64', '--decoder_layers', '1', '--decoder_units', '64', '--use_pyramidal',
                                 '--bottom_only', '--pass_hidden_state', '--dropout', '0', '--sampling_probability', '0',
                                 '--batch_size', '16', '--num_channels', '13', '--learning_rate', '0.003', '--num_epochs', '40',
                                 '--binary_outputs', '--output_ipa', '--binf_map', binf, '--multitask'] + extra))


def _drive(d):
    """The GPU half, run in a child process (the models it trains leave nothing in the test session's process-wide caches):
    train a --binf_projection and a sigmoid-output --multitask model, infer without and with the scoring, and save what the
    parent compares."""
    import contextlib
    import io
    import json
    import infer
    import preprocess_all
    from phones_las_amd import model_helper as mh
    lines = _corpus(d)
    open(d + '/list.csv', 'w').write('\n'.join(lines) + '\n')
    preprocess_all.main(preprocess_all.parse_args(['--input_file', d + '/list.csv', '--output_file', d + '/train.tfr',
                                                   '--save_norm', '--save_vocab']))
    binf = d + '/binf_map.csv'
    _binf_csv(binf, WORDS)
    _train(d, d + '/model', binf, ['--binf_projection'])
    _train(d, d + '/model_sig', binf, [])
    with open(d + '/frame_map.txt', 'w') as f:
        f.write('\n'.join(['%s\t%s\t%s' % (w, w, w) for w in WORDS[:4]] + ['h#\tsil', 'pau\tsil\tsil']) + '\n')
    captured = []
    orig = mh.LasModel.predict

    def spy(self, *a, **k):
        out = orig(self, *a, **k)
        captured.append({key: out[key].float().cpu().numpy() for key in KEYS if key in out})
        return out

    mh.LasModel.predict = spy
    names = ('infer.txt', 'infer.dmp', 'infer_targets.txt')
    res = {}
    for model, flags in (('model', []), ('model_sig', ['--use_phones_from_binf'])):
        md = d + '/' + model
        base = ['--data', d + '/train.tfr', '--vocab', d + '/vocab.txt', '--norm', d + '/norm.dmp', '--model_dir', md,
                '--num_channels', '13', '--batch_size', '5', '--binf_map', binf, '--plain_targets', d + '/list.csv']
        if not flags:                                    # without the scoring: the reference files
            res['per_plain'] = infer.main(infer.parse_args(base))
            files = [open(md + '/' + f, 'rb').read() for f in names]
        base += flags + ['--calc_frame_binf_accuracy', '--mapping_for_frame_accuracy', d + '/frame_map.txt',
                         '--encoder_frame_step', '20']
        for mode, extra in (('dtw', []), ('markup', ['--use_markup_segments'])):
            tag = model + '_' + mode
            captured.clear()
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                res['per_' + tag] = infer.main(infer.parse_args(base + extra))
            open(d + '/out_%s.txt' % tag, 'w').write(buf.getvalue())
            np.savez(d + '/pred_%s.npz' % tag, **{'%s_%d' % (k, i): c[k] for i, c in enumerate(captured) for k in c})
            res['n_pred_' + tag] = len(captured)
            now = [open(md + '/' + f, 'rb').read() for f in names]
            if flags and mode == 'dtw':
                files = now
            res['files_' + tag] = now == files
        if not flags:
            # --use_phones_from_binf on a --binf_projection decoder: logits_binf holds the raw 2 * nf outputs, not one per row
            try:
                infer.main(infer.parse_args(base + ['--use_phones_from_binf']))
                res['binf_error'] = ''
            except ValueError as e:
                res['binf_error'] = str(e)
    json.dump(res, open(d + '/result.json', 'w'))


def test_frame_binf_accuracy_through_infer(tmp_path):
    import json
    import subprocess
    import sys
    from phones_las_amd import utils
    d = str(tmp_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, '-c', 'import sys; sys.path.insert(0, %r); import tests.test_gpu_frame_binf_cli as t; '
                    't._drive(%r)' % (root, d)], cwd=root, check=True, timeout=900)
    res = json.load(open(d + '/result.json'))
    lines = open(d + '/list.csv').read().strip().split('\n')
    table = utils.load_binf2phone(d + '/binf_map.csv', utils.load_vocab(d + '/vocab.txt'))
    mapping = {w: w for w in WORDS[:4]}
    mapping.update({'h#': None, 'pau': 'sil'})
    F = len(table.index)
    for model in ('model', 'model_sig'):
        for mode in ('dtw', 'markup'):
            tag = model + '_' + mode
            assert res['files_' + tag]                                   # the three files do not depend on the scoring
            if model == 'model':
                assert res['per_' + tag] == res['per_plain']
            else:
                assert np.isfinite(res['per_' + tag]) and res['per_' + tag] == res['per_model_sig_dtw']
            out = open(d + '/out_%s.txt' % tag).read().strip().split('\n')
            assert out[-F - 1].split() == ['correct']
            got = [(l.split()[0], float(l.split()[1])) for l in out[-F:]]
            assert [g[0] for g in got] == list(table.index)             # <s> and </s> included
            z = np.load(d + '/pred_%s.npz' % tag)
            preds = [{k: z['%s_%d' % (k, i)] for k in KEYS if '%s_%d' % (k, i) in z.files} for i in range(res['n_pred_' + tag])]
            if model == 'model_sig':
                assert preds[0]['logits_binf'].shape[-1] == F                # the sigmoid decoder: one logit per table row
            want, warnings = _expected(preds, lines, table, mapping, mode == 'markup', 20, from_binf=model == 'model_sig')
            assert np.allclose([g[1] for g in got], want, rtol=0, atol=6e-7), (tag, got, want)
            assert sum(1 for l in out if l.startswith('Warining: sound ')) == len(warnings)
    assert 'columns' in res['binf_error'] and 'the feature table %d rows' % F in res['binf_error'], res['binf_error']
