"""The frame-accuracy kernels (csrc/align.hip) against tests/frame_binf_restated.py, bit for bit: the cleaned path's runs, the
phone ranges of the segments, the segment counts (las_attention_dtw_batch) and the per-feature counts of equal frames
(las_frame_binf_count) for the three sources of predicted rows."""
import numpy as np
import pytest
import torch

import tests.frame_binf_restated as R

pytestmark = pytest.mark.gpu


def _softmax_rows(rng, U, T, t_valid=None, temp=3.0):
    t_valid = T if t_valid is None else t_valid
    A = np.zeros((U, T), dtype=np.float32)
    if U and t_valid:
        z = rng.standard_normal((U, t_valid)) * temp
        # a roughly monotone alignment, as a trained attention gives
        z += -0.05 * (np.arange(t_valid)[None, :] - np.linspace(0, t_valid - 1, U)[:, None]) ** 2
        e = np.exp(z - z.max(1, keepdims=True))
        A[:, :t_valid] = (e / e.sum(1, keepdims=True)).astype(np.float32)
    return A


def _run(mats, pad=3):
    """dtw_ragged on matrices laid out back to back in one buffer, each with a row stride of T' + pad (read in place)."""
    from phones_las_amd import frame_binf as fb
    offs, rows, cols, lds, chunks = [], [], [], [], []
    at = 0
    for A in mats:
        U, T = A.shape
        ld = T + pad
        M = np.full((max(U, 1), ld), -7.0, dtype=np.float32)    # the pad columns must never be read
        M[:U, :T] = A
        offs.append(at)
        rows.append(U)
        cols.append(T)
        lds.append(ld)
        chunks.append(M.reshape(-1))
        at += M.size
    buf = torch.as_tensor(np.concatenate(chunks)).cuda()
    out = fb.dtw_ragged(buf, offs, rows, cols, lds)
    torch.cuda.synchronize()
    host = {k: out[k].cpu().numpy() for k in ('run_lo', 'run_hi', 'ph_st', 'ph_en', 'n_seg')}
    return out, host, (buf, offs, cols, lds)


def _check(mats, host, out, which=None):
    oo = out['out_off_np']
    for u in (range(len(mats)) if which is None else which):
        lo, hi, st, en, ns = R.align(mats[u])
        a, b = oo[u], oo[u + 1]
        assert int(host['n_seg'][u]) == ns, (u, mats[u].shape)
        assert np.array_equal(host['run_lo'][a:b], lo), u
        assert np.array_equal(host['run_hi'][a:b], hi), u
        assert np.array_equal(host['ph_st'][a:b], st), u
        assert np.array_equal(host['ph_en'][a:b], en), u


def test_dtw_random_softmax_and_padded_columns():
    rng = np.random.default_rng(0)
    mats = []
    for U, T in [(1, 1), (1, 9), (9, 1), (5, 3), (12, 4), (3, 17), (17, 40), (40, 200), (63, 64), (64, 80), (65, 70)]:
        mats.append(rng.random((U, T), dtype=np.float32))
        mats.append(_softmax_rows(rng, U, T))
        mats.append(_softmax_rows(rng, U, T, t_valid=max(1, (2 * T) // 3)))     # zero attention on the padded frames
    out, host, _ = _run(mats)
    _check(mats, host, out)


def test_dtw_exact_ties():
    rng = np.random.default_rng(1)
    mats = [np.zeros((6, 10), np.float32), np.zeros((10, 6), np.float32), np.full((4, 4), 0.5, np.float32)]
    for U, T in [(5, 8), (8, 5), (20, 30), (70, 90)]:
        mats.append(rng.choice(np.array([0.0, 0.25, 0.5], np.float32), size=(U, T)))
        # sums that tie although their predecessors differ: values whose float64 sums round alike
        mats.append(rng.choice(np.array([1.0, 1.0 + 2.0 ** -23, 2.0 ** -30, 0.0], np.float32), size=(U, T)))
    out, host, _ = _run(mats)
    _check(mats, host, out)


def test_dtw_empty_shapes():
    mats = [np.zeros((0, 5), np.float32), np.zeros((3, 0), np.float32), np.zeros((0, 0), np.float32),
            np.ones((2, 3), np.float32)]
    out, host, _ = _run(mats)
    assert list(host['n_seg']) == [0, 0, 0, R.align(mats[3])[4]]
    _check(mats, host, out)


def test_dtw_several_bands_and_the_workspace():
    from phones_las_amd import hip
    rng = np.random.default_rng(2)
    mats = [_softmax_rows(rng, 130, 150), rng.random((129, 60), dtype=np.float32)]
    out, host, _ = _run(mats)
    assert hip.lib().las_attention_dtw_workspace_bytes(130, 150, 2) == 0          # backpointers in LDS
    _check(mats, host, out)
    mats = [_softmax_rows(rng, 300, 1000), rng.random((257, 300), dtype=np.float32), _softmax_rows(rng, 5, 7)]
    assert hip.lib().las_attention_dtw_workspace_bytes(300, 1000, 3) > 0          # the largest table does not fit
    out, host, _ = _run(mats)
    _check(mats, host, out)


def test_dtw_ragged_batch_of_1700():
    rng = np.random.default_rng(3)
    mats = []
    for k in range(1700):
        U = int(rng.integers(25, 56))
        T = int(rng.integers(150, 251))
        mats.append(_softmax_rows(rng, U, T, t_valid=T - int(rng.integers(0, 20))) if k % 3 else rng.random((U, T), dtype=np.float32))
    out, host, _ = _run(mats, pad=0)
    _check(mats, host, out, which=range(0, 1700, 11))
    # every utterance: a path whose runs are monotone and cover every column, ranges inside [0, U)
    oo = out['out_off_np']
    for u, A in enumerate(mats):
        a, b = oo[u], oo[u + 1]
        lo, hi = host['run_lo'][a:b], host['run_hi'][a:b]
        assert (lo <= hi).all() and (np.diff(hi) >= 0).all() and hi[-1] == A.shape[0] - 1 and lo[0] == 0
        assert host['n_seg'][u] >= 1 and (host['ph_en'][a:b] <= A.shape[0]).all()
    # the same batch again: the same bits
    out2, host2, _ = _run(mats, pad=0)
    for k in host:
        assert np.array_equal(host[k], host2[k])


def _markup(rng, T, nseg):
    """Markup segments in frames (ascending, a few empty or overlapping ones, the last one possibly past T')."""
    cuts = np.sort(rng.integers(0, T + 3, size=nseg + 1))
    cuts[0] = 0
    segs = np.stack([cuts[:-1], cuts[1:]], 1)
    if nseg > 3:
        segs[1, 1] = segs[1, 0]                          # empty
        segs[2, 0] = max(0, segs[2, 0] - 2)              # overlaps its predecessor
    return segs


@pytest.mark.parametrize('source', ['hypothesis', 'sigmoid', 'markup'])
def test_counts_against_the_restatement(source):
    from phones_las_amd import frame_binf as fb
    rng = np.random.default_rng({'hypothesis': 4, 'sigmoid': 5, 'markup': 6}[source])
    F, V = 9, 14
    table = (rng.random((F, V)) < 0.4).astype(np.float32)
    mats, Ps, segs, binfs, n_tgt = [], [], [], [], []
    shapes = [(0, 12), (1, 1), (1, 20), (20, 5), (6, 30), (40, 200), (70, 90)] + \
             [(int(rng.integers(1, 50)), int(rng.integers(1, 120))) for _ in range(60)]
    for U, T in shapes:
        A = _softmax_rows(rng, U, T, t_valid=max(1, T - 3)) if U % 2 else rng.choice(np.array([0, .5, 1], np.float32), (U, T))
        if source == 'sigmoid':
            logits = rng.standard_normal((U + 1, F)).astype(np.float32) * 3
            logits[0, 0] = 0.0                           # sigmoid 0.5 rounds to 0 (half to even)
            P = fb.binf_preds_from_logits(logits, F)
            assert np.array_equal(P, R.sigmoid_rows(logits))
        else:
            P = fb.hypothesis_rows(table, rng.integers(0, V, size=U))
        seg = _markup(rng, T, int(rng.integers(1, 12)))
        b = (rng.random((len(seg), F)) < 0.5).astype(np.uint8)
        mats.append(A)
        Ps.append(P)
        segs.append(seg)
        binfs.append(b)
        n_tgt.append(int(seg[-1, -1]))
    out, host, att = _run(mats)
    if source == 'markup':
        counts, seg_phone = fb.count_ragged(Ps, segs, binfs, n_tgt, att=att)
        k = 0
        for A, seg in zip(mats, segs):
            want = R.markup_phones(A, seg)
            assert list(seg_phone[k:k + len(seg)]) == want
            k += len(seg)
    else:
        counts, _ = fb.count_ragged(Ps, segs, binfs, [min(A.shape[1], n) for A, n in zip(mats, n_tgt)], dtw=out)
    for u, (A, P, seg, b) in enumerate(zip(mats, Ps, segs, binfs)):
        tgt = R.markup_frames_binf(seg, b)
        pred = R.pred_frames_markup(A, P, seg) if source == 'markup' else R.pred_frames_dtw(A, P)
        want, _ = R.count(pred, tgt)
        assert np.array_equal(counts[u], want), (u, A.shape)


def test_width_mismatch_is_refused():
    from phones_las_amd import frame_binf as fb
    with pytest.raises(ValueError, match='12 columns.*6 rows'):
        fb.binf_preds_from_logits(np.zeros((4, 12), np.float32), 6)
