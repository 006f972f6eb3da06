"""Normalised edit distance with the reference's pre-processing (utils/metrics_utils.py:8-41): optional id
mapping, keep the last element of every run of equal ids, cut at the first EOS, drop -1, then
Levenshtein / len(truth) (tf.edit_distance(normalize=True)).  `edit_distance` is the pure-Python statement of it, kept as
the yardstick; `edit_distance_device` / `edit_distance_on_device` do the same integer work in one launch of
las_edit_distance_batch (csrc/metrics.hip) on ids that are already on the device."""
__all__ = ['edit_distance', 'dense_to_sparse', 'edit_distance_device', 'edit_distance_on_device', 'levenshtein_lists', 'normalised',
           'host_metrics_forced']


def _rows(t):
    if hasattr(t, 'detach'):
        return t.detach().cpu().tolist()
    return [list(r) for r in t]


def dense_to_sparse(row, eos_id):
    ext = list(row) + [eos_id]
    first_eos = ext.index(eos_id)
    return [v for i, v in enumerate(row) if ext[i + 1] != v and i < first_eos and v != -1]


def _levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        ai = a[i - 1]
        for j in range(1, len(b) + 1):
            sub = prev[j - 1] + (ai != b[j - 1])
            ins = cur[j - 1] + 1
            dele = prev[j] + 1
            cur[j] = sub if sub < ins and sub < dele else (ins if ins < dele else dele)
        prev = cur
    return prev[-1]


def edit_distance(hypothesis, truth, eos_id, mapping=None):
    out = []
    for h, t in zip(_rows(hypothesis), _rows(truth)):
        if mapping:
            h = [mapping[i] for i in h]
            t = [mapping[i] for i in t]
        hs, ts = dense_to_sparse(h, eos_id), dense_to_sparse(t, eos_id)
        d = _levenshtein(hs, ts)
        if not ts:
            out.append(float('inf') if hs else 0.0)
        else:
            out.append(d / len(ts))
    return out


def host_metrics_forced():
    """LAS_HOST_METRICS=1 (read at every call; a test hook): score on the host with `edit_distance`."""
    import os
    return os.environ.get('LAS_HOST_METRICS', '0') == '1'


def _flat_rows(t):
    """A [R, S] integer device tensor as (int32 buffer, int64 offsets [R], row length S) without a copy when it is an int32 view
    of unit inner stride whose rows do not overlap."""
    import torch
    if t.dtype != torch.int32 or t.numel() == 0 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.to(torch.int32).contiguous()
    R, S = t.shape
    if R * S == 0:                                           # empty rows: nothing to address
        return t.reshape(-1), torch.zeros(R, dtype=torch.int64, device=t.device), S
    stride = t.stride(0) if R > 1 else S
    buf = t.as_strided(((R - 1) * stride + S,), (1,))
    return buf, torch.arange(R, dtype=torch.int64, device=t.device) * stride, S


def edit_distance_device(hypothesis, truth, eos_id, mapping=None, beams=None):
    """The integer triple (dist, hyp_n, ref_n) of `edit_distance`, int32 tensors on the device, in one launch and without a
    synchronisation.  hypothesis: device ids [B, S] against truth [B, U]; or, with beams='last', [B, S, K] and with
    beams='middle' [B, K, S] against [B, U]: B * K entries, utterance-major, the K beams of an utterance sharing its row of
    truth.  CPU tensors raise hip.LasError.  Status values (hip.edit_distance_status) are left in dist."""
    import torch
    from .. import hip
    if not (torch.is_tensor(hypothesis) and torch.is_tensor(truth) and hypothesis.is_cuda and truth.is_cuda):
        raise hip.LasError('expected CUDA tensors; the LAS ops have no CPU path')
    if beams not in (None, 'last', 'middle'):
        raise ValueError("beams is None, 'last' ([B, S, K]) or 'middle' ([B, K, S])")
    if hypothesis.dim() != (2 if beams is None else 3) or truth.dim() != 2:
        raise ValueError('edit_distance_device: hypothesis %s, truth %s, beams=%r' % (tuple(hypothesis.shape), tuple(truth.shape), beams))
    dev = hypothesis.device
    K = 1
    if beams == 'last':
        hypothesis = hypothesis.permute(0, 2, 1)
    if beams is not None:
        K = hypothesis.shape[1]
        hypothesis = hypothesis.to(torch.int32).contiguous().view(-1, hypothesis.shape[2])
    B = min(hypothesis.shape[0] // K, truth.shape[0])          # zip: the shorter of the two
    hbuf, hoff, S = _flat_rows(hypothesis[:B * K])
    rbuf, roff, U = _flat_rows(truth[:B])
    if max(S, U) > hip.ED_LEN_MAX:
        raise ValueError('edit distance: %d tokens (at most %d)' % (max(S, U), hip.ED_LEN_MAX))
    hlen = torch.full((B * K,), S, dtype=torch.int32, device=dev)
    rlen = torch.full((B,), U, dtype=torch.int32, device=dev)
    roh = torch.arange(B * K, dtype=torch.int32, device=dev) // K if K > 1 else None
    m = torch.as_tensor(list(mapping), dtype=torch.int32, device=dev) if mapping else None
    return hip.edit_distance_batch(hbuf, hoff, hlen, rbuf, roff, rlen, eos_id, max(S, U), ref_of_hyp=roh, mapping=m)


def normalised(dist, hyp_n, ref_n):
    """The float64 list `edit_distance` returns, from the integer triple (host sequences): dist / ref_n, inf for an empty
    reference against a non-empty hypothesis, 0.0 when both are empty.  Status values raise (hip.edit_distance_status)."""
    from .. import hip
    hip.edit_distance_status(dist)
    return [(float('inf') if n else 0.0) if not m else d / m for d, n, m in zip(dist, hyp_n, ref_n)]


def edit_distance_on_device(hypothesis, truth, eos_id, mapping=None):
    """`edit_distance` of device ids, scored on the device: one launch, one copy of B integer triples; the same Python floats."""
    import torch
    d, n, m = torch.stack(edit_distance_device(hypothesis, truth, eos_id, mapping)).cpu().tolist()
    return normalised(d, n, m)


def levenshtein_lists(hyps, refs, ref_of_hyp=None, device='cuda'):
    """`_levenshtein(hyps[i], refs[ref_of_hyp[i]])` of every i (ref_of_hyp None: refs[i]) for lists of integer lists, scored
    as given (no mapping, no EOS rule) in ONE launch: the list of distances.  infer.py's PER / Optimistic PER."""
    import itertools
    import torch
    from .. import hip
    if not hyps:
        return []

    def ragged(rows):
        lens = [len(r) for r in rows]
        off = [0] + list(itertools.accumulate(lens))[:-1]
        return (torch.tensor(list(itertools.chain.from_iterable(rows)), dtype=torch.int32).to(device),
                torch.tensor(off, dtype=torch.int64).to(device), torch.tensor(lens, dtype=torch.int32).to(device), max(lens))

    h, hoff, hlen, hmax = ragged(hyps)
    r, roff, rlen, rmax = ragged(refs)
    if max(hmax, rmax) > hip.ED_LEN_MAX:
        raise ValueError('edit distance: %d tokens (at most %d)' % (max(hmax, rmax), hip.ED_LEN_MAX))
    roh = torch.tensor(list(ref_of_hyp), dtype=torch.int32).to(device) if ref_of_hyp is not None else None
    dist, _, _ = hip.edit_distance_batch(h, hoff, hlen, r, roff, rlen, 0, max(hmax, rmax), ref_of_hyp=roh, flags=0)
    dist = dist.cpu().tolist()
    hip.edit_distance_status(dist)
    return dist
