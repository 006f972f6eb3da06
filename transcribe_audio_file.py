#!/usr/bin/env python3
"""One audio file -> features -> prediction -> symbols, with the flag surface of the reference's transcribe_audio_file.py
(transcribe_audio_file.py:13-118): the model from --model_dir (hparams.json + checkpoint.pt, as infer.py loads it), the audio
through phones-las_amd/audio.py (librosa.load(path, sr=16000, mono=True): RIFF WAV / NIST SPHERE at any rate, resampled on the
GPU), the features through phones-las_amd/frontend.py (preprocess_all's calculate_acoustic_features), normalised with --norm
as (x - mean) / std, and decoded greedily or with --beam_width.

For every file it prints, as the reference does, one `key: shape` line per prediction of that utterance and then the list of
predicted symbols: the best beam of 'sample_ids' ('sample_ids_phones_binf' with --use_phones_from_binf) cut at the first </s>.
--output_file: joblib.dump of the list of per-utterance prediction dicts.

An addition: --waveform takes several paths.  Their signals are resampled in one launch and their features formed in one
batched pass; every utterance is then decoded on its own (batch 1, as the reference's single file), so each file's block is
what a run on that file alone prints.  --feature_type lyon is out of scope and raises."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SAMPLE_RATE = 16000


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--waveform', type=str, nargs='+', required=True, help='Acoustic file (several: one block per file)')
    p.add_argument('--vocab', type=str, required=True, help='vocabulary table, listing vocabulary line by line')
    p.add_argument('--norm', type=str, default=None, help='normalization params')
    p.add_argument('--mapping', type=str, help='additional mapping when evaluation')
    p.add_argument('--model_dir', type=str, required=True, help='path of imported model')
    p.add_argument('--beam_width', type=int, default=0, help='number of beams (default 0: using greedy decoding)')
    p.add_argument('--delimiter', help='Symbols delimiter. Default: " "', type=str, default=' ')
    p.add_argument('--binf_map', type=str, default='misc/binf_map.csv', help='Path to CSV with phonemes to binary features map')
    p.add_argument('--use_phones_from_binf', help='User phonemes decoded from binary features decoder outputs.', action='store_true')
    p.add_argument('--feature_type', help='Acoustic feature type.', type=str, choices=['mfe', 'mfcc', 'lyon'], default='mfcc')
    p.add_argument('--backend', help='Library for calculating acoustic features.', type=str, choices=['speechpy', 'librosa'],
                   default='librosa')
    p.add_argument('--n_mfcc', help='Number of MFCC coeffs.', type=int, default=13)
    p.add_argument('--n_mels', help='Number of mel-filters.', type=int, default=40)
    p.add_argument('--window', help='Analysis window length in ms.', type=int, default=20)
    p.add_argument('--step', help='Analysis window step in ms.', type=int, default=10)
    p.add_argument('--deltas', help='Calculate deltas and double-deltas.', action='store_true')
    p.add_argument('--energy', help='Compute energy.', action='store_true')
    p.add_argument('--output_file', help='location for saving predictions')
    return p.parse_args(argv)


def load_waveforms(paths):
    """librosa.load(path, sr=16000, mono=True) of every path; the signals not at 16 kHz resampled in one launch."""
    from phones_las_amd import audio
    decoded = [audio.read(p) for p in paths]
    waves = [audio.to_mono(y) for y, _ in decoded]
    srs = [sr for _, sr in decoded]
    todo = [i for i, sr in enumerate(srs) if sr != SAMPLE_RATE]
    if todo:
        for i, y in zip(todo, audio.resample_batch([waves[i] for i in todo], [srs[i] for i in todo], SAMPLE_RATE)):
            waves[i] = y
    return waves


def main(args):
    import torch
    from phones_las_amd import frontend, utils
    from phones_las_amd import model_helper as mh
    from phones_las_amd.utils.dataset_utils import process_dataset
    from infer import to_text
    from train import load_checkpoint, to_device

    if args.feature_type == 'lyon':
        raise ValueError('lyon features are out of scope')
    args_h = argparse.Namespace(model_dir=args.model_dir, mapping=args.mapping)
    hparams = utils.create_hparams(args_h)              # requires an existing hparams.json (params_utils.py:96-97)
    hparams.decoder.set_hparam('beam_width', args.beam_width)
    vocab_list = utils.load_vocab(args.vocab)
    binf2phone_np = None
    if hparams.decoder.binary_outputs:                  # transcribe_audio_file.py:72-80 of the reference
        if args.mapping is not None:
            vocab_list, mapping = utils.get_mapping(args.mapping, args.vocab)
            hparams.del_hparam('mapping')
            hparams.add_hparam('mapping', mapping)
        binf2phone_np = utils.load_binf2phone(args.binf_map, vocab_list).values
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    model = mh.LasModel(hparams, binf2phone=binf2phone_np)
    load_checkpoint(model, os.path.join(args.model_dir, 'checkpoint.pt'))

    waves = load_waveforms(args.waveform)
    feats = [f.cpu().numpy() for f in frontend.calculate_acoustic_features_batch(args, waves)]
    means = stds = None
    if args.norm is not None:
        means, stds = utils.load_normalization(args.norm)
    vocab_table = utils.create_vocab_table(args.vocab)
    key = 'sample_ids_phones_binf' if args.use_phones_from_binf else 'sample_ids'
    predictions = []
    for x in feats:
        # utils.process_dataset(..., batch 1, is_infer=True): the (x - mean) / std of the reference's input_fn
        batch = next(process_dataset(lambda: iter([(x, [])]), vocab_table, utils.SOS, utils.EOS, means, stds, 1, 1, is_infer=True))
        f, _ = to_device(batch[0], None, dev)
        pred = model.predict(f, transparent_projection=bool(args.use_phones_from_binf))
        # this utterance's row of every batched prediction, as numpy (bf16 internals widened to float32, the reference's dtype)
        p = {k: (v[0].float() if v.is_floating_point() else v[0]).cpu().numpy()
             for k, v in pred.items() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 1}
        predictions.append(p)
        beams = p[key].T
        i = beams[0] if len(beams.shape) > 1 else beams
        i = i.tolist() + [utils.EOS_ID]
        i = i[:i.index(utils.EOS_ID)]
        text = to_text(vocab_list, i, args.delimiter).split(args.delimiter)
        for k in p.keys():
            print(f'{k}: {p[k].shape}')
        print(text)
    model.check_device_status()
    if args.output_file:
        from joblib import dump
        dump(predictions, args.output_file)
        print(f'Predictions are saved to {args.output_file}')
    return predictions


if __name__ == '__main__':
    main(parse_args())
