"""Frame-level binary-feature accuracy on TIMIT (infer.py --calc_frame_binf_accuracy of the reference, infer.py:75-191,233-343):
how often each articulatory feature is right, frame by frame, against the .PHN markup.

Host side: the frame-accuracy map, the TIMIT markup and its conversion to encoder frames (librosa 0.7.1 time_to_frames with the
reference's arguments), the predicted feature rows of a hypothesis.  Device side (csrc/align.hip): ``dtw_ragged`` runs fastdtw's
exact DTW on every attention matrix of a ragged batch and turns the path into segments (las_attention_dtw_batch), ``count_ragged``
compares the per-frame feature vectors (las_frame_binf_count).  No host fallback: a missing library is an error."""
import numpy as np
import torch

from . import audio, hip

SAMPLE_RATE = 16000
WIN_LEN = 0.02 * SAMPLE_RATE          # the reference's n_fft argument of time_to_frames (320.0)

__all__ = ['read_mapping', 'read_timit_markup', 'markup_to_frames', 'hypothesis_rows', 'binf_preds_from_logits',
           'dtw_ragged', 'dtw_padded', 'count_ragged']


def read_mapping(path):
    """--mapping_for_frame_accuracy: one entry per line, tab-separated; three or more columns map the first to the last, fewer
    map it to None (scored as 'sil').  The reference splits the whole file on all whitespace, which leaves every entry with one
    column (every target becomes 'sil'); here each line is an entry."""
    mapping = {}
    with open(path, 'r') as f:
        for line in f.read().strip().split('\n'):
            line = line.rstrip('\r')
            if not line.strip():
                continue
            cells = line.split('\t')
            mapping[cells[0]] = cells[-1] if len(cells) >= 3 else None
    return mapping


def phn_path(sound_path):
    """The markup beside a TIMIT sound file: '.WAV' replaced by '.PHN' (upper case only, as the reference does)."""
    return sound_path.replace('.WAV', '.PHN')


def read_timit_markup(sound_path, table, mapping):
    """get_timit_binf_markup: the .PHN segments [start, end) in samples (int64 [N, 2]), their feature rows (uint8 [N, F]: the
    table column of each mapped phone, nonzero -> 1; a phone mapped to None is 'sil') and the sound's length in samples at
    16 kHz (audio.load, as librosa.load)."""
    with open(phn_path(sound_path), 'r') as f:
        lines = f.read().strip().split('\n')
    segs = np.zeros((len(lines), 2), dtype=np.int64)
    binfs = np.zeros((len(lines), len(table.index)), dtype=np.uint8)
    for i, line in enumerate(lines):
        st, en, phone = line.split()
        phone = mapping[phone]
        if phone is None:
            phone = 'sil'
        segs[i] = [int(st), int(en)]
        binfs[i] = table[phone] != 0
    y, _ = audio.load(sound_path, SAMPLE_RATE)
    return segs, binfs, int(y.shape[0])


def markup_to_frames(segs, nsamples, encoder_frame_step=40):
    """The markup in encoder frames, as the reference computes it: times = min(samples / 16000, nsamples / 16000) in float64,
    then librosa 0.7.1 time_to_frames(times, 16000, hop_length=encoder_frame_step * 16000 / 1000, n_fft=320.0) =
    floor((int(times * 16000) - 160) // hop), negative frames set to 0.  (The divide and the multiply are kept: st / 16000 *
    16000 can truncate to st - 1.)"""
    t = np.asarray(segs, dtype=np.float64).reshape(-1, 2) / SAMPLE_RATE
    t = np.minimum(t, nsamples / SAMPLE_RATE)
    samples = (t * SAMPLE_RATE).astype(int)
    hop = encoder_frame_step * SAMPLE_RATE / 1000
    frames = np.floor((samples - int(WIN_LEN // 2)) // hop).astype(int)
    frames[frames < 0] = 0
    return frames


def hypothesis_rows(table_values, ids):
    """P_u of a hypothesis: the feature-table column of each symbol id (nonzero -> 1), uint8 [U, F]."""
    ids = np.asarray(ids, dtype=np.int64)
    table_values = np.asarray(table_values)
    return np.ascontiguousarray((table_values[:, ids] != 0).T.astype(np.uint8)).reshape(len(ids), table_values.shape[0])


def binf_preds_from_logits(logits_binf, n_features):
    """--use_phones_from_binf: np.round(1 / (1 + np.exp(-logits_binf[:-1]))) in float32, as the reference writes it, nonzero -> 1
    (uint8 [S - 1, F]).  The width must be the feature table's row count (the reference fails there too)."""
    logits = np.asarray(logits_binf, dtype=np.float32)[:-1, :]
    if logits.shape[1] != n_features:
        raise ValueError('--use_phones_from_binf: logits_binf has %d columns, the feature table %d rows; the frame accuracy '
                         'compares one against the other' % (logits.shape[1], n_features))
    with np.errstate(over='ignore'):
        preds = np.round(1 / (1 + np.exp(-logits)))
    return (preds != 0).astype(np.uint8)


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def dtw_ragged(buf, offs, rows, cols, lds):
    """las_attention_dtw_batch on utterances read in place from ``buf`` (a CUDA float32 tensor): utterance u is the
    rows[u] x cols[u] matrix at element offset offs[u] with row stride lds[u].  Returns a dict of device tensors: 'run_lo' /
    'run_hi' / 'ph_st' / 'ph_en' (int32, utterance u's cols[u] entries at 'out_off'[u]), 'n_seg' (int32 [n]), and 'out_off'
    (int64 [n + 1], on the host as numpy too: 'out_off_np')."""
    if not (torch.is_tensor(buf) and buf.is_cuda and buf.dtype == torch.float32):
        raise hip.LasError('dtw_ragged: the attention buffer must be a CUDA float32 tensor')
    rows, cols, lds = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (rows, cols, lds))
    offs = np.asarray(offs, dtype=np.int64).reshape(-1)
    n = len(rows)
    if n == 0:
        raise ValueError('dtw_ragged: no utterances')
    if (rows < 0).any() or (cols < 0).any() or ((lds < cols) & (rows > 0)).any():
        raise ValueError('dtw_ragged: negative shapes or a row stride below the column count')
    last = offs + np.where(rows > 0, (rows - 1) * lds + cols, 0)
    if (offs < 0).any() or (last > buf.numel()).any():
        raise ValueError('dtw_ragged: a matrix reaches past the attention buffer')
    u_max, t_max = int(rows.max()), int(cols.max())
    out_off = np.zeros(n + 1, dtype=np.int64)
    out_off[1:] = np.cumsum(cols)
    total = max(int(out_off[-1]), 1)
    dev = buf.device
    out = {k: torch.empty(total, dtype=torch.int32, device=dev) for k in ('run_lo', 'run_hi', 'ph_st', 'ph_en')}
    out['n_seg'] = torch.empty(n, dtype=torch.int32, device=dev)
    out['out_off'] = _dev(out_off, np.int64)
    out['out_off_np'] = out_off
    out['rows_np'] = rows
    d_offs, d_rows, d_cols, d_lds = _dev(offs, np.int64), _dev(rows, np.int32), _dev(cols, np.int32), _dev(lds, np.int32)
    L = hip.lib()
    ws_bytes = int(L.las_attention_dtw_workspace_bytes(u_max, t_max, n))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    hip.check(L.las_attention_dtw_batch(hip.p(buf), hip.p(d_offs), hip.p(d_rows), hip.p(d_cols), hip.p(d_lds), n, u_max, t_max,
                                        hip.p(out['out_off']), hip.p(out['run_lo']), hip.p(out['run_hi']), hip.p(out['ph_st']),
                                        hip.p(out['ph_en']), hip.p(out['n_seg']), hip.p(ws), ws_bytes, hip.stream()))
    out['_keep'] = (d_offs, d_rows, d_cols, d_lds, ws)
    return out


def dtw_padded(att, rows):
    """dtw_ragged on the leading rows[b] rows of each [S, T'] matrix of a contiguous CUDA tensor [B, S, T'] (the predict
    batch's alignments: every utterance keeps the batch-padded T', as the reference's DTW does)."""
    if att.dim() != 3 or not att.is_contiguous():
        raise ValueError('dtw_padded: a contiguous [B, S, T\'] tensor is expected')
    B, S, T = att.shape
    rows = np.asarray(rows, dtype=np.int64)
    if len(rows) != B or (rows > S).any():
        raise ValueError('dtw_padded: %d row counts for %d matrices of %d rows' % (len(rows), B, S))
    return dtw_ragged(att, np.arange(B, dtype=np.int64) * S * T, rows, np.full(B, T), np.full(B, T))


def count_ragged(P_list, seg_list, binf_list, n_frames, dtw=None, att=None):
    """las_frame_binf_count over a batch: per utterance u, int64 counts [n, F] of the frames j < n_frames[u] on which the
    predicted and the target value of each feature agree.  P_list[u]: uint8 [U_u, F] (the rows the prediction ORs); seg_list[u]:
    the markup segments in frames (int [N_u, 2], clamped to >= 0); binf_list[u]: their uint8 target rows [N_u, F].  The
    prediction comes from ``dtw`` (dtw_ragged's outputs: each frame ORs the rows of its segment) or, with ``att`` =
    (buf, offs, cols, lds) of the same utterances (--use_markup_segments), from the rows the markup segments take.  Returns
    (counts, seg_phone): seg_phone (int32 per markup segment, -1: none) in markup mode, else None."""
    if (dtw is None) == (att is None):
        raise ValueError('count_ragged: exactly one of dtw / att')
    n = len(P_list)
    F = None
    for P, b in zip(P_list, binf_list):
        for m in (P, b):
            if m.ndim == 2 and m.shape[0] > 0:
                F = m.shape[1] if F is None else F
                if m.shape[1] != F:
                    raise ValueError('count_ragged: feature widths %d and %d' % (F, m.shape[1]))
    if F is None:
        F = binf_list[0].shape[1] if binf_list[0].ndim == 2 else 0
    if not 0 < F <= 256:
        raise ValueError('count_ragged: %d features (1 .. 256 supported)' % F)
    p_rows = np.array([P.shape[0] for P in P_list], dtype=np.int64)
    p_off = np.zeros(n, dtype=np.int64)
    p_off[1:] = np.cumsum(p_rows * F)[:-1]
    P_all = np.concatenate([np.asarray(P, dtype=np.uint8).reshape(-1) for P in P_list] + [np.zeros(1, np.uint8)])
    nseg = np.array([len(s) for s in seg_list], dtype=np.int64)
    seg_off = np.zeros(n + 1, dtype=np.int64)
    seg_off[1:] = np.cumsum(nseg)
    seg_all = np.concatenate([np.asarray(s, dtype=np.int64).reshape(-1, 2) for s in seg_list] + [np.zeros((1, 2), np.int64)])
    if (seg_all < 0).any() or (seg_all > np.iinfo(np.int32).max).any():
        raise ValueError('count_ragged: markup frames must be clamped to >= 0')
    binf_all = np.concatenate([np.asarray(b, dtype=np.uint8).reshape(-1, F) for b in binf_list] + [np.zeros((1, F), np.uint8)])
    n_frames = np.asarray(n_frames, dtype=np.int64)
    if dtw is not None:
        cols = np.diff(dtw['out_off_np'])
        if len(cols) != n or (n_frames > cols).any():
            raise ValueError('count_ragged: more frames counted than the DTW covered')
        if (p_rows < dtw['rows_np']).any():      # the phone ranges index P_u's rows: at least the DTW's U of them
            raise ValueError('count_ragged: fewer P rows than the DTW\'s phones')
    counts = torch.empty((n, F), dtype=torch.int32, device='cuda')
    seg_phone = torch.full((max(int(seg_off[-1]), 1),), -1, dtype=torch.int32, device='cuda')
    d = [_dev(P_all, np.uint8), _dev(p_off, np.int64), _dev(p_rows, np.int32), _dev(seg_all.astype(np.int32), np.int32),
         _dev(binf_all, np.uint8), _dev(seg_off, np.int64), _dev(n_frames, np.int32)]
    if dtw is not None:
        ph_st, ph_en, f_off = dtw['ph_st'], dtw['ph_en'], dtw['out_off']
        a_buf = a_off = a_cols = a_ld = None
    else:
        buf, offs, cols, lds = att
        cols, lds = np.asarray(cols, dtype=np.int64), np.asarray(lds, dtype=np.int64)
        offs = np.asarray(offs, dtype=np.int64)
        r = np.minimum(p_rows, 5)
        if ((r > 0) & (lds < cols)).any() or (offs + np.where(r > 0, (r - 1) * lds + cols, 0) > buf.numel()).any():
            raise ValueError('count_ragged: an attention matrix reaches past its buffer')
        ph_st = ph_en = f_off = None
        a_buf, a_off, a_cols, a_ld = buf, _dev(offs, np.int64), _dev(cols, np.int32), _dev(lds, np.int32)
    hip.check(hip.lib().las_frame_binf_count(hip.p(d[0]), hip.p(d[1]), hip.p(d[2]), F, hip.p(ph_st), hip.p(ph_en), hip.p(f_off),
                                             hip.p(d[3]), hip.p(d[4]), hip.p(d[5]), hip.p(a_buf), hip.p(a_off), hip.p(a_cols),
                                             hip.p(a_ld), hip.p(d[6]), n, hip.p(seg_phone), hip.p(counts), hip.stream()))
    counts = counts.cpu().numpy().astype(np.int64)
    return counts, (seg_phone[:int(seg_off[-1])].cpu().numpy() if att is not None else None)
