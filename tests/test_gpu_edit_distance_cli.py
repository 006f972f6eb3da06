"""infer.py's one-launch scoring and eval.py's `ctc_edit_distance` field, end to end on the GPU: utterances of the twin corpus
(tests/twin_corpus.py) as a TFRecord set, a few training steps for a checkpoint (the error rate does not matter here), then
infer.py greedy and with --beam_width 2.  The printed PER / Optimistic PER lines must be what the host loop infer.py ran until
now gives for the same predictions (recorded from LasModel.predict), and the three files what they always were."""
import os

import numpy as np
import pytest

from tests import twin_corpus as tc

pytestmark = pytest.mark.gpu

PHONES = ['p%d' % i for i in range(tc.NPHONES)]


def _corpus(d, n=24):
    from phones_las_amd.utils import tfrecord
    from phones_las_amd.utils.features_utils import save_normalization
    open(os.path.join(d, 'vocab.txt'), 'w').write('\n'.join(PHONES) + '\n')
    truth = []
    with tfrecord.TFRecordWriter(os.path.join(d, 'train.tfr')) as w:
        for x, ys in tc.utterances(n, 11):
            w.write(tfrecord.make_example(x, [PHONES[y] for y in ys]))
            truth.append(' '.join(PHONES[y] for y in ys))
    save_normalization(os.path.join(d, 'norm.dmp'), np.zeros(tc.F, np.float32), np.ones(tc.F, np.float32))
    return truth


def _train(d, model, extra=()):
    import train
    train.main(train.parse_args(['--train', os.path.join(d, 'train.tfr'), '--model_dir', os.path.join(d, model), '--encoder_layers', '2',
                                 '--encoder_units', '64', '--decoder_layers', '1', '--decoder_units', '64', '--use_pyramidal',
                                 '--bottom_only', '--pass_hidden_state', '--dropout', '0', '--sampling_probability', '0',
                                 '--batch_size', '8', '--num_channels', str(tc.F), '--learning_rate', '0.003', '--num_epochs', '20']
                                + list(extra)))


def _cli(d, model):
    return ['--data', os.path.join(d, 'train.tfr'), '--vocab', os.path.join(d, 'vocab.txt'), '--norm', os.path.join(d, 'norm.dmp'),
            '--model_dir', os.path.join(d, model), '--num_channels', str(tc.F), '--batch_size', '8']


def test_infer_prints_what_the_host_loop_gave(tmp_path, capsys, monkeypatch):
    import infer
    from joblib import load
    from phones_las_amd import model_helper as mh
    from phones_las_amd import utils
    from phones_las_amd.utils.metrics_utils import _levenshtein
    d = str(tmp_path)
    truth = _corpus(d)
    _train(d, 'model')
    vocab_list = utils.load_vocab(os.path.join(d, 'vocab.txt'))
    recorded = []
    predict = mh.LasModel.predict

    def recording(self, *a, **kw):
        pred = predict(self, *a, **kw)
        recorded.append(pred['sample_ids'].cpu().numpy())
        return pred

    monkeypatch.setattr(mh.LasModel, 'predict', recording)

    def text_of(ids):
        syms = [vocab_list[x] for x in ids] + [utils.EOS]
        return syms[:syms.index(utils.EOS)]

    for beam in (0, 2):
        del recorded[:]
        capsys.readouterr()
        per = infer.main(infer.parse_args(_cli(d, 'model') + (['--beam_width', str(beam)] if beam else [])))
        out = capsys.readouterr().out
        beams_all = [[b.tolist() for b in (ids[k].T if ids.ndim == 3 else ids[k][None])] for ids in recorded for k in range(ids.shape[0])]
        assert len(beams_all) == len(truth) and all(len(b) == max(beam, 1) for b in beams_all)
        err = tot = optimistic = 0                                    # infer.py's host loop, as it was
        for beams, t in zip(beams_all, [t.split(' ') for t in truth]):
            texts = [text_of(i) for i in beams]
            err += _levenshtein(texts[0], t)
            optimistic += min(_levenshtein(x, t) for x in texts)
            tot += len(t)
        assert per == 100.0 * err / max(tot, 1)
        lines = out.strip().split('\n')
        assert 'PER: %2.2f%%' % per in lines
        if beam:
            assert 'Optimistic PER: %2.2f%%' % (100.0 * optimistic / max(tot, 1)) in lines and optimistic <= err
        else:
            assert not any(l.startswith('Optimistic') for l in lines)
        hyp_lines = [' '.join(text_of(b[0])) for b in beams_all]
        model_dir = os.path.join(d, 'model')
        assert open(os.path.join(model_dir, 'infer.txt')).read() == '\n'.join(hyp_lines)
        assert load(os.path.join(model_dir, 'infer.dmp')) == [{'transcription': l} for l in hyp_lines]
        assert open(os.path.join(model_dir, 'infer_targets.txt')).read() == '\n'.join(truth)
        # ... and the same numbers from the files alone (an empty transcription is an empty hypothesis)
        dmp = [p['transcription'].split(' ') if p['transcription'] else [] for p in load(os.path.join(model_dir, 'infer.dmp'))]
        tgt = [l.split(' ') for l in open(os.path.join(model_dir, 'infer_targets.txt')).read().split('\n')]
        assert sum(_levenshtein(h, t) for h, t in zip(dmp, tgt)) == err and sum(len(t) for t in tgt) == tot


def test_eval_prints_the_ctc_field_for_ctc_models_only(tmp_path, capsys):
    import eval as eval_cli
    d = str(tmp_path)
    _corpus(d, n=16)
    _train(d, 'plain')
    _train(d, 'ctc', ['--ctc_weight', '0.3'])
    capsys.readouterr()
    loss, ed = eval_cli.main(eval_cli.parse_args(_cli(d, 'ctc')))
    line = [l for l in capsys.readouterr().out.split('\n') if l.startswith('eval: ')][-1]
    assert np.isfinite(loss) and ed >= 0.0
    assert ', edit_distance = ' in line and ', ctc_edit_distance = ' in line
    assert float(line.split('ctc_edit_distance = ')[1]) >= 0.0
    eval_cli.main(eval_cli.parse_args(_cli(d, 'plain')))
    line = [l for l in capsys.readouterr().out.split('\n') if l.startswith('eval: ')][-1]
    assert 'ctc_edit_distance' not in line and ', edit_distance = ' in line
