"""las_edit_distance_batch (csrc/metrics.hip) against the unchanged host functions of utils.metrics_utils: integers, compared
with ==.  The sequences of every launch lie in one buffer with gaps of a poison id between them that must never be read (under
a mapping a read of it would give status -2).

The layout switches from LDS to the device workspace at a raw length of 1024 on either side (ED_LDS_LEN = 1023 in the kernel
file): test_lds_and_workspace_sides_of_the_switch runs lengths 1023 and 1024."""
import numpy as np
import pytest
import torch

from phones_las_amd import hip
from phones_las_amd.utils import metrics_utils as mu

pytestmark = pytest.mark.gpu

POISON = 7777
EOS = 4


def ragged(rows, rng):
    buf, off = [], []
    for r in rows:
        buf += [POISON] * int(rng.integers(1, 4))
        off.append(len(buf))
        buf += list(r)
    buf += [POISON] * 3
    return (torch.tensor(buf, dtype=torch.int32).cuda(), torch.tensor(off, dtype=torch.int64).cuda(),
            torch.tensor([len(r) for r in rows], dtype=torch.int32).cuda())


def device(hyps, refs, eos=EOS, mapping=None, merge=True, ref_of_hyp=None, len_max=None, seed=0):
    rng = np.random.default_rng(seed)
    h, hoff, hlen = ragged(hyps, rng)
    r, roff, rlen = ragged(refs, rng)
    if len_max is None:
        len_max = max([len(x) for x in hyps] + [len(x) for x in refs])
    roh = torch.tensor(ref_of_hyp, dtype=torch.int32).cuda() if ref_of_hyp is not None else None
    m = torch.tensor(mapping, dtype=torch.int32).cuda() if mapping is not None else None
    out = hip.edit_distance_batch(h, hoff, hlen, r, roff, rlen, eos, len_max, ref_of_hyp=roh, mapping=m,
                                  flags=hip.ED_MERGE if merge else 0)
    return [tuple(t) for t in torch.stack(out).t().cpu().tolist()]


def host(h, t, eos=EOS, mapping=None, merge=True):
    if mapping is not None:
        h, t = [mapping[i] for i in h], [mapping[i] for i in t]
    if merge:
        h, t = mu.dense_to_sparse(h, eos), mu.dense_to_sparse(t, eos)
    return (mu._levenshtein(h, t), len(h), len(t))


def check(hyps, refs, **kw):
    got = device(hyps, refs, **kw)
    roh = kw.get('ref_of_hyp') or range(len(hyps))
    hk = {k: v for k, v in kw.items() if k in ('eos', 'mapping', 'merge')}
    want = [host(h, refs[q], **hk) for h, q in zip(hyps, roh)]
    assert got == want


def test_edge_lengths_identical_and_disjoint():
    rng = np.random.default_rng(1)
    sizes = [(0, 0), (0, 5), (5, 0), (1, 1), (1, 300), (300, 1)]
    for a in (63, 64, 65, 127, 128, 129):
        sizes += [(a, 64), (64, a), (a, a), (a, 7), (7, a)]
    hyps, refs, want_dist = [], [], []
    for n, m in sizes:
        same = rng.integers(0, 10, max(n, m)).tolist()
        # identical content (distance |n - m|: one is a prefix of the other), disjoint alphabets (max(n, m)), random content
        hyps += [same[:n], rng.integers(0, 10, n).tolist(), rng.integers(0, 3, n).tolist()]
        refs += [same[:m], rng.integers(10, 20, m).tolist(), rng.integers(0, 3, m).tolist()]
        want_dist += [abs(n - m), max(n, m), None]
    hyps += [[3], [3]]                                    # (1, 1) equal and unequal
    refs += [[3], [5]]
    want_dist += [0, 1]
    got = device(hyps, refs, merge=False)
    assert [g[0] for g, w in zip(got, want_dist) if w is not None] == [w for w in want_dist if w is not None]
    assert got == [host(h, t, merge=False) for h, t in zip(hyps, refs)]
    check(hyps, refs, merge=True)                          # the same pairs through the run rule (no EOS, no -1 among them)


def test_lds_and_workspace_sides_of_the_switch():
    rng = np.random.default_rng(2)
    seq = lambda n, lo=0, hi=6: rng.integers(lo, hi, n).tolist()
    assert hip.lib().las_edit_distance_workspace_bytes(1023, 4) == 0
    lds_h, lds_r = [seq(1023), seq(40), seq(1023, 0, 3)], [seq(40), seq(1023), seq(130, 0, 3)]
    check(lds_h, lds_r, merge=False)                       # len_max = 1023: LDS only, no workspace
    assert hip.lib().las_edit_distance_workspace_bytes(1024, 4) > 0
    # len_max = 1100: pairs with a side of 1024 or more go through the workspace, the short ones of the same launch through LDS
    ws_h = [seq(1024), seq(40), seq(1023), seq(1030, 0, 3), seq(5), seq(1024, 0, 2)]
    ws_r = [seq(40), seq(1024), seq(1023, 0, 6), seq(1100, 0, 3), seq(9), seq(200, 0, 2)]
    check(ws_h, ws_r, merge=False)
    check(ws_h[:3] + ws_h[4:], ws_r[:3] + ws_r[4:], merge=True)


RUN = [1] * 60 + [2] * 8 + [3] * 70          # the run of 2s straddles raw indices 63 | 64


@pytest.mark.parametrize('hyp, ref, mapping', [
    ([EOS, 1, 2, 3], [1, 2, 3], None),                                   # EOS at index 0
    ([1, 2, 3, EOS], [1, 2, 2, 3], None),                                # EOS at the last index
    ([1, 2, 2, 3, 3], [1, 2, 3, 1], None),                               # no EOS
    ([1, 2, EOS, 3, 3, EOS, 1], [1, EOS, EOS], None),                    # only the first EOS counts
    (RUN, [1, 2, 3], None),
    (RUN[:64], RUN[:63], None),                                          # the chunk boundary is the sequence end
    ([1] * 64 + [EOS] + [2] * 10, [1] * 63 + [2] + [EOS], None),         # EOS first in the second chunk / last in the first
    ([5, -1, 5], [5, 5], None),                                          # -1 separates the runs before it is dropped
    ([-1, 1, 2, -1], [-1, -1, 1, 2], None),                              # -1 at the ends
    ([-1] * 70, [1], None),
    ([0, 1, 2, 3, 0], [0, 2, 3, 0], [0, 0, 2, 3, EOS, 5]),               # the mapping collapses the neighbours 0 and 1
    ([0, 5, 0, 1, 5], [5, 5, 0], [0, 1, 2, 3, EOS, -1]),                 # ... maps 5 to -1
    ([0, 1, 3, 2, 0], [0, 1, 2, 3], [0, 1, 2, EOS, EOS, 5]),             # ... maps 3 onto eos_id
])
def test_preprocessing(hyp, ref, mapping):
    h, t = host(hyp, ref, mapping=mapping), device([hyp], [ref], mapping=mapping)[0]
    assert t == h
    check([hyp, ref, hyp], [ref, hyp, hyp], mapping=mapping)
    if mapping is None:                                    # [5, -1, 5] keeps both 5s
        assert device([[5, -1, 5]], [[5]])[0] == (1, 2, 1)


MAPPING = [0, 1, 1, 3, EOS, -1]              # 2 -> 1 merges neighbours, 5 -> -1


@pytest.mark.parametrize('merge, mapped', [(True, False), (True, True), (False, False), (False, True)])
def test_random_pairs(merge, mapped):
    """2 000 pairs over the four variants (500 each, drawn from one stream), lengths uniform in 0..200, an alphabet of 4 ids plus
    EOS plus -1: runs and ties abound.  EOS is drawn with probability 0.005 (uniformly it would cut every sequence after a few
    tokens and leave the table untested), -1 with 0.1.  Under a mapping the raw alphabet is 0..5 and -1 arises as the image of id
    5: a raw -1 is outside the mapping, which the kernel reports (status -2) where Python's list index wraps around."""
    variant = [(True, False), (True, True), (False, False), (False, True)].index((merge, mapped))
    rng = np.random.default_rng(100)
    ids = [0, 1, 2, 3, EOS, -1]
    p = [0.22, 0.22, 0.22, 0.235, 0.005, 0.1]
    pairs = []
    for k in range(2000):
        n, m = int(rng.integers(0, 201)), int(rng.integers(0, 201))
        h, t = rng.choice(6, n, p=p).tolist(), rng.choice(6, m, p=p).tolist()
        if k % 4 == variant:
            pairs.append((h, t) if mapped else ([ids[i] for i in h], [ids[i] for i in t]))
    assert len(pairs) == 500
    check([h for h, _ in pairs], [t for _, t in pairs], merge=merge, mapping=MAPPING if mapped else None)


def test_beams_share_a_reference():
    rng = np.random.default_rng(7)
    B, S, K, U = 5, 40, 4, 30
    ids = [0, 1, 2, 3, EOS, -1]
    hyp = np.asarray(ids)[rng.choice(6, (B, S, K), p=[0.24, 0.24, 0.24, 0.24, 0.02, 0.02])]
    ref = np.asarray(ids)[rng.choice(6, (B, U), p=[0.24, 0.24, 0.24, 0.24, 0.02, 0.02])]
    want = [host(hyp[b, :, k].tolist(), ref[b].tolist()) for b in range(B) for k in range(K)]
    dh, dr = torch.as_tensor(hyp, dtype=torch.int32).cuda(), torch.as_tensor(ref, dtype=torch.int32).cuda()
    for got in (mu.edit_distance_device(dh, dr, EOS, beams='last'),
                mu.edit_distance_device(dh.permute(0, 2, 1).contiguous(), dr, EOS, beams='middle')):
        assert [tuple(t) for t in torch.stack(got).t().cpu().tolist()] == want
    # ragged, through ref_of_hyp directly
    hyps = [hyp[b, :, k].tolist() for b in range(B) for k in range(K)]
    refs = [r.tolist() for r in ref]
    roh = [b for b in range(B) for _ in range(K)]
    check(hyps, refs, ref_of_hyp=roh)
    # infer.py's loop: the symbols up to the first EOS, as they are; PER takes beam 0, Optimistic PER the utterance's minimum
    cut = lambda x: x[:(x + [EOS]).index(EOS)]
    texts, targets = [cut(h) for h in hyps], [cut(r) for r in refs]
    dist = mu.levenshtein_lists(texts, targets, roh)
    assert dist == [mu._levenshtein(x, targets[q]) for x, q in zip(texts, roh)]
    for b in range(B):
        assert min(dist[b * K:(b + 1) * K]) == min(mu._levenshtein(x, targets[b]) for x in texts[b * K:(b + 1) * K])


def test_status_values_are_reported_not_read():
    hyps, refs = [[1, 2, 3], list(range(11)), [1, 2], [3]], [[1, 3], [1, 2], list(range(12)), [3, 3]]
    got = device(hyps, refs, merge=False, len_max=10)          # pairs 1 and 2 hold a length above len_max
    assert got == [host(hyps[0], refs[0], merge=False), (-1, 0, 0), (-1, 0, 0), host(hyps[3], refs[3], merge=False)]
    with pytest.raises(ValueError):
        hip.edit_distance_status([g[0] for g in got])
    # an id outside the mapping (6 entries): above it, negative, and the poison is outside it too
    mapping = [0, 1, 2, 3, EOS, 5]
    hyps, refs = [[1, 2, 3], [1, 6, 2], [1, 2], [0, 1]], [[1, 3], [1, 2], [2, -1, 1], [0, 1, 1]]
    got = device(hyps, refs, mapping=mapping)
    assert got[0] == host(hyps[0], refs[0], mapping=mapping) and got[3] == host(hyps[3], refs[3], mapping=mapping)
    assert got[1][0] == -2 and got[2][0] == -2
    with pytest.raises(IndexError):
        hip.edit_distance_status([g[0] for g in got])
    bad = torch.tensor([[1, 9, 2]], dtype=torch.int32).cuda()
    with pytest.raises(IndexError):
        mu.edit_distance_on_device(bad, bad, EOS, mapping)


def test_strided_rows_are_read_in_place():
    """evaluate's form: [B, S] against a [B, U] view of wider rows (train_edit_distance cuts the targets to the logits' width)."""
    rng = np.random.default_rng(9)
    hyp = torch.as_tensor(rng.integers(0, 6, (7, 33)).astype(np.int32)).cuda()
    wide = torch.as_tensor(rng.integers(0, 6, (7, 50)).astype(np.int64)).cuda()
    for truth in (wide[:, :33], wide.to(torch.int32)[:, :29], wide.to(torch.int32)):
        assert mu.edit_distance_on_device(hyp, truth, EOS) == mu.edit_distance(hyp, truth, EOS)
    assert mu.edit_distance_on_device(hyp[:, :0], wide[:, :5], EOS) == mu.edit_distance(hyp[:, :0], wide[:, :5], EOS)
