#!/usr/bin/env python3
"""Decoding with the flag surface and the OUTPUT FILES of the reference's infer.py (infer.py:21-63,192-359): reads
hparams.json and the checkpoint from --model_dir, decodes --data (TFRecord; no shuffle, the tail batch kept -- SURVEY B1)
greedily or with --beam_width, and writes, as the reference does (infer.py:345-359):

  model_dir/infer.txt          one line per utterance: to_text(ids) = the symbols up to the first </s>, joined with
                               --delimiter (infer.py:65-67 cuts at the first EOS SYMBOL; the best beam under --beam_width)
  model_dir/infer.dmp          joblib.dump([{'transcription': <that line>}, ...])
  model_dir/infer_targets.txt  the targets, joined with --delimiter (infer.py:269-271)

--plain_targets CSV (infer.py:246-271): rows `sound,lang,phrase` (tab-separated when the line holds a tab); the phrase is
split on blanks, stripped and lower-cased, zipped with the predictions in file order, and PER / Optimistic PER are the
text-level edit distances against it (infer.py:277-303,338-339; with --mapping on a binary-outputs model the target symbols
go through the 61->39 style map, infer.py:300-303).  WITHOUT --plain_targets the reference prints no PER at all; here the
labels stored in the TFRecord serve as targets (same files, same formulas) -- an addition, not a difference in the files.
--calc_frame_binf_accuracy (infer.py:75-191,233-343; TIMIT only): per frame of the encoder (--encoder_frame_step ms) the
predicted binary-feature vector against the .PHN markup beside each --plain_targets sound file, printed as the reference's
table (one row per feature-table row, <s> and </s> included; correct = equal frames / frames).  The hypothesis is aligned to
the frames by fastdtw's exact DTW on its attention matrix (the predict batch's padded T', as the reference's), on the GPU
(phones-las_amd/frame_binf.py, csrc/align.hip); --use_markup_segments gives each markup segment the phone whose attention peaks
there, --use_phones_from_binf the rounded sigmoids of the binary decoder's outputs.  Text -> IPA conversion
(--convert_targets_to_ipa, espeak-ng) is out of scope.

Deliberate deviations in the PRINTED numbers (the files are the reference's):
  * Optimistic PER, greedy decode: the reference only lowers its per-utterance `min_err = 100000` inside the beam loop
    (infer.py:278-289), so without --beam_width it adds 100000 per utterance; here the minimum runs over the hypotheses
    that exist (one, in greedy mode: Optimistic PER = PER).  In its beam loop the reference scores the beams against `t`
    BEFORE this utterance's `t` is assigned (infer.py:286 vs :296: the previous utterance's target); here against this one's.
  * blank lines of --plain_targets are skipped; the reference's split(',') would raise on them.
Frame-level accuracy (--calc_frame_binf_accuracy), reference behaviour kept and changed:
  * --mapping_for_frame_accuracy is read one line per entry, tab-separated (three columns map to the last, fewer to None =
    'sil'); the reference's read().strip().split() splits on all whitespace, so every target became 'sil'.  CHANGED.
  * segments_to_attention (--use_markup_segments) never advances last_phone: every markup segment searches the first five
    phones.  KEPT (the intended update cannot be known).
  * an empty hypothesis: the reference's to_text gives '', and ''.split(' ') == [''] keeps one attention row, whose symbol ''
    then fails as a KeyError of the feature table; here the hypothesis has U = 0 rows, no segments, and its predicted frames
    are all zero over T'.  CHANGED.  So is a markup segment whose frame window holds no column of the attention
    (the reference's np.max of an empty slice raises): it predicts no feature.
  * --beam_width > 0 makes the reference slice beams instead of steps: refused with SystemExit.  CHANGED.
  * a model built without --binary_outputs has no feature table (None) and the reference crashes: the table is loaded from
    --binf_map for scoring only (the model is still built without it).  CHANGED.
  * without --plain_targets the reference computes and says nothing: SystemExit (the markup needs the sound paths).  CHANGED.
  * the DTW runs over the batch-padded T' (padded frames have zero attention: many ties).  KEPT, with the predict batch's
    shapes.
  * --use_phones_from_binf reads logits_binf as the reference's predict returns it: the feature logits of a sigmoid-output
    decoder (--binary_outputs without --binf_projection), one per feature-table row.  Under --calc_frame_binf_accuracy the
    transparent projection is asked for only of a --binf_projection model, whose raw [p1 | p0] outputs are twice as wide and
    are refused with a ValueError naming both widths (the reference fails on the broadcast).
  * the table is printed as two plain columns (the feature-table row name, then correct with six decimals under a
    'correct' header), not through pandas' DataFrame repr, whose number formatting and row elision depend on pandas'
    display options.  The values are the reference's.  CHANGED (layout only)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='LAS inference on MI355X (HIP), drop-in for the reference CLI.')
    p.add_argument('--data', type=str, required=True, help='inference data in TFRecord format')
    p.add_argument('--plain_targets', type=str, help='Path to CSV file with targets.')
    p.add_argument('--vocab', type=str, required=True, help='vocabulary table, listing vocabulary line by line')
    p.add_argument('--norm', type=str, default=None, help='normalization params')
    p.add_argument('--mapping', type=str, help='additional mapping when evaluation')
    p.add_argument('--model_dir', type=str, required=True, help='path of imported model')
    p.add_argument('--beam_width', type=int, default=0)
    p.add_argument('--batch_size', type=int, default=8)
    p.add_argument('--num_channels', type=int, default=39)
    p.add_argument('--delimiter', help='Symbols delimiter. Default: " "', type=str, default=' ')
    p.add_argument('--take', help='Use this number of elements (0 for all).', type=int, default=0)
    p.add_argument('--binf_map', type=str, default='misc/binf_map.csv')
    p.add_argument('--use_phones_from_binf', action='store_true')
    p.add_argument('--convert_targets_to_ipa', action='store_true')
    p.add_argument('--calc_frame_binf_accuracy', action='store_true')
    p.add_argument('--mapping_for_frame_accuracy', type=str)
    p.add_argument('--encoder_frame_step', type=int, default=40)
    p.add_argument('--use_markup_segments', action='store_true')
    return p.parse_args(argv)


def to_text(vocab_list, sample_ids, delimiter=' '):
    """infer.py:65-67: the symbols of the ids up to (not including) the first </s> SYMBOL, joined with the delimiter."""
    from phones_las_amd.utils import EOS
    sym_list = [vocab_list[x] for x in sample_ids] + [EOS]
    return delimiter.join(sym_list[:sym_list.index(EOS)])


def main(args):
    if args.convert_targets_to_ipa:
        raise SystemExit('--convert_targets_to_ipa (text -> IPA with espeak-ng) is not on the HIP path')
    if args.calc_frame_binf_accuracy:
        if args.beam_width > 0:
            raise SystemExit('--calc_frame_binf_accuracy scores the greedy hypothesis: use it without --beam_width')
        if not args.plain_targets:
            raise SystemExit('--calc_frame_binf_accuracy needs --plain_targets: the TIMIT markup sits beside its sound files')
        if not args.mapping_for_frame_accuracy:
            raise SystemExit('--calc_frame_binf_accuracy needs --mapping_for_frame_accuracy')
    from phones_las_amd import utils
    from phones_las_amd import model_helper as mh
    from phones_las_amd.utils.metrics_utils import levenshtein_lists
    from train import load_checkpoint, to_device

    vocab_list = utils.load_vocab(args.vocab)
    vocab_list_orig = vocab_list
    args_h = argparse.Namespace(model_dir=args.model_dir, mapping=args.mapping)
    hparams = utils.create_hparams(args_h)              # requires an existing hparams.json (params_utils.py:96-97)
    hparams.decoder.set_hparam('beam_width', args.beam_width)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    binf2phone_np = None
    text_mapping = None                      # the reference's local `mapping` (infer.py:202-207): binary-outputs models only
    if hparams.decoder.binary_outputs:       # infer.py:203-210 of the reference
        if args.mapping is not None:
            vocab_list, mapping_list = utils.get_mapping(args.mapping, args.vocab)
            text_mapping = mapping_list
            hparams.del_hparam('mapping')
            hparams.add_hparam('mapping', mapping_list)
        binf2phone_np = utils.load_binf2phone(args.binf_map, vocab_list).values
    model = mh.LasModel(hparams, binf2phone=binf2phone_np)
    load_checkpoint(model, os.path.join(args.model_dir, 'checkpoint.pt'))

    frame_acc = None
    if args.calc_frame_binf_accuracy:
        from phones_las_amd import frame_binf
        table = utils.load_binf2phone(args.binf_map, vocab_list)    # a model without --binary_outputs: for scoring only
        frame_acc = _FrameAccuracy(frame_binf, table, frame_binf.read_mapping(args.mapping_for_frame_accuracy),
                                   _read_plain_targets(args.plain_targets), args)

    mapping = hparams.mapping
    batches = utils.input_fn(args.data, args.vocab, args.norm, num_channels=args.num_channels,
                             batch_size=args.batch_size, num_epochs=1, take=args.take, is_infer=True)
    # per utterance: the beams' id lists (greedy: one), uncut; and the TFRecord's own labels
    beams_all, record_targets = [], []
    for features, labels in batches:
        f, _ = to_device(features, None, dev)
        # transcribe_audio_file.py:90 couples the two; the frame accuracy needs the sigmoid decoder's feature logits as the
        # reference's predict returns them, so it asks for the projection's raw outputs only of a --binf_projection model
        transparent = bool(args.use_phones_from_binf) and (not args.calc_frame_binf_accuracy or model.binf_projection)
        pred = model.predict(f, transparent_projection=transparent)
        # infer.py:223: the phones decoded from the binary-feature decoder, or the phone decoder's
        ids = pred['sample_ids_phones_binf' if args.use_phones_from_binf else 'sample_ids'].cpu().numpy()   # [B,T] / [B,T,K]
        if frame_acc is not None:
            frame_acc.add_batch(pred, ids, len(beams_all))
        for b in range(ids.shape[0]):
            beams_all.append([beam.tolist() for beam in (ids[b].T if ids.ndim == 3 else ids[b][None])])
            t = labels['targets_outputs'][b][:labels['target_sequence_length'][b] - 1].tolist()
            if mapping is not None:
                t = [mapping[x] for x in t]
                t = [x for x in t if x >= 0]
            record_targets.append([vocab_list[x] for x in t])
    model.check_device_status()          # a timed-out persistent kernel would have produced invalid hypotheses

    def text_of(ids):                    # infer.py:65-67 (as a symbol list)
        syms = [vocab_list[x] for x in ids] + [utils.EOS]
        return syms[:syms.index(utils.EOS)]

    if args.plain_targets:               # infer.py:246-268
        targets = [[x.strip().lower() for x in cells[2].split()] for cells in _read_plain_targets(args.plain_targets)]
    else:
        targets = record_targets
    # Every symbol of hypotheses and targets becomes an integer through one dict (--plain_targets words outside the vocabulary
    # included); all utterances x beams are then scored in ONE launch (csrc/metrics.hip), the sequences as they are.
    sym_ids = {}
    hyps, refs, ref_of_hyp, first_hyp = [], [], [], []
    for k, (beams, t) in enumerate(zip(beams_all, targets)):      # zip: the shorter of the two, as the reference's loop (infer.py:276)
        texts = [text_of(i) for i in beams]
        if args.plain_targets and text_mapping is not None:
            # infer.py:300-303: symbols of the original vocabulary through the id map (infer_targets.txt keeps the raw phrase)
            t = [vocab_list[text_mapping[vocab_list_orig.index(x)]] for x in t]
        if frame_acc is not None:                       # infer.py:326-331, in utterance order
            frame_acc.report(k, t)
        first_hyp.append(len(hyps))
        hyps += [[sym_ids.setdefault(x, len(sym_ids)) for x in text] for text in texts]
        ref_of_hyp += [k] * len(texts)
        refs.append([sym_ids.setdefault(x, len(sym_ids)) for x in t])
    dist = levenshtein_lists(hyps, refs, ref_of_hyp, dev)
    first_hyp.append(len(hyps))
    err = sum(dist[i] for i in first_hyp[:-1])          # the best-scoring beam is the hypothesis (infer.py:286-288)
    optimistic_err = sum(min(dist[i:j]) for i, j in zip(first_hyp, first_hyp[1:]))
    tot = sum(len(t) for t in refs)
    with open(os.path.join(args.model_dir, 'infer_targets.txt'), 'w') as f:
        f.write('\n'.join(args.delimiter.join(t) for t in targets))
    predictions = [{'transcription': args.delimiter.join(text_of(beams[0]))} for beams in beams_all]      # infer.py:345-353
    with open(os.path.join(args.model_dir, 'infer.txt'), 'w') as f:
        f.write('\n'.join(p['transcription'] for p in predictions))
    from joblib import dump
    dump(predictions, os.path.join(args.model_dir, 'infer.dmp'))                                           # infer.py:358-359
    per = 100.0 * err / max(tot, 1)
    print('PER: %2.2f%%' % per)
    if args.beam_width > 0 or args.plain_targets:        # infer.py:338-339 prints both whenever it prints
        print('Optimistic PER: %2.2f%%' % (100.0 * optimistic_err / max(tot, 1)))
    if frame_acc is not None:
        print(frame_acc.render())
    return per


def _read_plain_targets(path):
    """The --plain_targets rows as cell lists (tab-separated when the line holds a tab); blank lines skipped."""
    rows = []
    for line in open(path, 'r'):
        if not line.strip():
            continue
        rows.append(line.split('\t' if '\t' in line else ','))
    return rows


class _FrameAccuracy(object):
    """--calc_frame_binf_accuracy: the markup of every --plain_targets row, read up front; per predict batch one DTW launch and
    one counting launch (frame_binf.dtw_padded / count_ragged); per utterance its counts and frame numbers, reported in
    utterance order."""

    def __init__(self, fb, table, mapping, rows, args):
        self.fb, self.table, self.args = fb, table, args
        self.F = len(table.index)
        self.markup = []
        for cells in rows:                                   # infer.py:262-264 (get_timit_binf_markup)
            segs, binfs, nsamples = fb.read_timit_markup(cells[0], table, mapping)
            self.markup.append((fb.markup_to_frames(segs, nsamples, args.encoder_frame_step), binfs))
        self.results = {}                                    # utterance index -> (counts [F], prediction frames, target frames)
        self.correct = np.zeros(self.F, dtype=np.int64)
        self.frames = 0

    def add_batch(self, pred, ids, first):
        fb = self.fb
        B = ids.shape[0]
        us = [first + b for b in range(B) if first + b < len(self.markup)]
        if not us:
            return
        if self.args.use_phones_from_binf:                  # infer.py:315-319
            logits = pred['logits_binf'].float().cpu().numpy()
            P = [fb.binf_preds_from_logits(logits[u - first], self.F) for u in us]
            att = pred['alignment_binf']
        else:                                               # the hypothesis' symbols, up to the first </s>
            from phones_las_amd.utils import EOS_ID
            P = []
            for u in us:
                h = ids[u - first].tolist() + [EOS_ID]
                P.append(fb.hypothesis_rows(self.table.values, h[:h.index(EOS_ID)]))
            att = pred['alignment']
        att = att[:len(us)].float().contiguous()
        rows = [p.shape[0] for p in P]
        n_tgt = [int(self.markup[u][0][-1, -1]) if len(self.markup[u][0]) else 0 for u in us]
        segs = [self.markup[u][0] for u in us]
        binfs = [self.markup[u][1] for u in us]
        Bn, S, T = att.shape
        if self.args.use_markup_segments:                   # infer.py:325-327: segments_to_attention + get_binf_markup_frames
            n_pred = n_tgt
            counts, _ = fb.count_ragged(P, segs, binfs, n_tgt, att=(att, np.arange(Bn) * S * T, np.full(Bn, T), np.full(Bn, T)))
        else:                                               # infer.py:322-324: attention_to_segments + segs_phones_to_frame_binf
            n_pred = [T] * len(us)
            dtw = fb.dtw_padded(att, rows)
            counts, _ = fb.count_ragged(P, segs, binfs, [min(T, n) for n in n_tgt], dtw=dtw)
            bad = dtw['n_seg'].cpu().numpy()
            if (bad < 0).any():
                raise ValueError('--calc_frame_binf_accuracy: the attention of utterance %d has no DTW path (NaN?)'
                                 % us[int(np.flatnonzero(bad < 0)[0])])
        for k, u in enumerate(us):
            self.results[u] = (counts[k], n_pred[k], n_tgt[k])

    def report(self, u, t):
        if u not in self.results:
            return
        counts, n_pred, n_tgt = self.results[u]
        if n_pred != n_tgt:
            print('Warining: sound {} prediction frames {} target frames {}'.format(t, n_pred, n_tgt))
        self.correct += counts
        self.frames += min(n_pred, n_tgt)

    def render(self):
        """The reference's DataFrame({'correct': correct / frames}, index=feature table rows), printed."""
        acc = self.correct / self.frames if self.frames else np.full(self.F, np.nan)
        names = [str(x) for x in self.table.index]
        w = max(len(x) for x in names)
        lines = [' ' * w + '   correct']
        lines += ['%-*s  %8.6f' % (w, name, a) for name, a in zip(names, acc)]
        return '\n'.join(lines)


if __name__ == '__main__':
    main(parse_args())
