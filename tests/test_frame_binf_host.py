"""Host side of the frame-level binary-feature accuracy (no GPU): the map file, the markup in frames at the truncation boundary,
the restatement's DTW on matrices worked out by hand, the ISA of the kernels, and infer.py's refusals."""
import os
import sys

import numpy as np
import pytest

import tests.frame_binf_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mapping_one_entry_per_line(tmp_path):
    from phones_las_amd import frame_binf as fb
    p = tmp_path / 'map.txt'
    p.write_text('aa\taa\taa\nao\taa\taa\nax-h\tah\tah\nq\nepi\tsil\nh#\tsil\tsil\n')
    m = fb.read_mapping(str(p))
    assert m == {'aa': 'aa', 'ao': 'aa', 'ax-h': 'ah', 'q': None, 'epi': None, 'h#': 'sil'}


def test_markup_to_frames_at_the_truncation_boundary():
    from phones_las_amd import frame_binf as fb
    # 32160 / 16000 * 16000 = 32159.999...: the sample is truncated to 32159, one below a frame boundary (160 + 50 * 640)
    assert int(np.float64(32160) / 16000 * 16000) == 32159
    f = fb.markup_to_frames(np.array([[0, 32160], [32160, 32800]]), 10 ** 6)
    assert f.tolist() == [[0, 49], [49, 51]]
    # 32800 = 160 + 51 * 640 is exact: frame 51, but a sound that ends at sample 32700 cuts it: min(t, nsamples / sr)
    assert fb.markup_to_frames(np.array([[32160, 32800]]), 32700).tolist() == [[49, 50]]
    assert fb.markup_to_frames(np.array([[32160, 32800]]), 40000).tolist() == [[49, 51]]
    # before the first half window: negative frames become 0; another frame step
    assert fb.markup_to_frames(np.array([[0, 100], [100, 800]]), 10 ** 6).tolist() == [[0, 0], [0, 1]]
    assert fb.markup_to_frames(np.array([[0, 1760]]), 10 ** 6, encoder_frame_step=10).tolist() == [[0, 10]]
    for segs, n, step in [(np.array([[0, 5000], [5000, 32160], [32160, 99999]]), 90000, 40), (np.array([[7, 1001]]), 999, 20)]:
        assert np.array_equal(fb.markup_to_frames(segs, n, step), R.time_to_frames(segs, n, step))


def test_dtw_ties_go_up_first():
    # D[2,2]: up = D[1,2] - 1, left = D[2,1] - 1, diagonal = D[1,1] - 1, all -2: the up step wins
    A = np.array([[1, 0], [0, 1]], np.float32)
    D, path = R.dtw(A)
    assert D[1, 1] == -1 and D[1, 2] == -1 and D[2, 1] == -1 and D[2, 2] == -2
    assert path == [(0, 0), (0, 1), (1, 1)]
    # column 1 holds rows 0..1; A[0,1] > A[1,1] is false and row 0 is in column 0: row 0 is dropped
    H = R.hard_attention(A)
    assert H.tolist() == [[1, 0], [0, 1]]
    assert R.segments(H) == [[0, 1, 0, 1], [1, 2, 1, 2]]
    lo, hi, st, en, ns = R.align(A)
    assert lo.tolist() == [0, 1] and hi.tolist() == [0, 1] and st.tolist() == [0, 1] and en.tolist() == [1, 2] and ns == 2


def test_dtw_more_phones_than_frames_and_a_kept_run():
    A = np.full((3, 1), 0.5, np.float32)
    D, path = R.dtw(A)
    assert D[:, 1].tolist() == [np.inf, -0.5, -1.0, -1.5]
    assert path == [(0, 0), (1, 0), (2, 0)]
    lo, hi, st, en, ns = R.align(A)                 # 0.5 > 0.5 is false and there is no column 0 - 1: the run stays
    assert (lo.tolist(), hi.tolist(), st.tolist(), en.tolist(), ns) == ([0], [2], [0], [3], 1)


def test_dtw_compares_sums_not_predecessors():
    # D[1,2] = 0 and D[2,1] = -2^-60 differ, but with dt = -1 both sums round to -1: a tie, which the up step wins
    # (comparing the predecessors would take the left step: path (0,0), (1,0), (1,1))
    A = np.array([[0, 0], [2.0 ** -60, 1]], np.float32)
    D, path = R.dtw(A)
    assert D[1, 2] == 0 and D[2, 1] == -2.0 ** -60 and D[2, 2] == -1
    assert (D[1, 2] - 1.0) == (D[2, 1] - 1.0)
    assert path == [(0, 0), (0, 1), (1, 1)]


def test_cleanup_on_a_hand_worked_path():
    # D[1,1] = -0.9, D[2,1] = -1.4 (up), D[1,2] = -0.9 (left), D[2,2] = min(-1.7, -2.2, -1.7) = -2.2 (left),
    # D[3,1] = -1.4 (up), D[3,2] = min(-3.1, -2.3, -2.3) = -3.1 (up): path (0,0), (1,0), (1,1), (2,1)
    A = np.array([[0.9, 0.0], [0.5, 0.8], [0.0, 0.9]], np.float32)
    D, path = R.dtw(A)
    assert path == [(0, 0), (1, 0), (1, 1), (2, 1)]
    assert abs(D[3, 2] - (-3.1)) < 1e-6 and abs(D[2, 2] - (-2.2)) < 1e-6
    # column 0 (rows 0..1): A[0,0] > A[1,0] and row 1 is in column 1: row 1 is dropped;
    # column 1 (rows 1..2): A[1,1] > A[2,1] is false and row 1 is not in the cleaned column 0: kept
    assert R.hard_attention(A).tolist() == [[1, 0], [0, 1], [0, 1]]
    lo, hi, st, en, ns = R.align(A)
    assert (lo.tolist(), hi.tolist(), st.tolist(), en.tolist(), ns) == ([0, 1], [0, 2], [0, 2], [2, 3], 2)


def test_markup_frames_and_markup_phones():
    binfs = np.array([[1, 0], [0, 1], [1, 1]], np.uint8)
    frames = np.array([[0, 2], [1, 3], [3, 3]])            # overlapping, then an empty segment that ends the markup at 3
    assert R.markup_frames_binf(frames, binfs).astype(int).tolist() == [[1, 0], [1, 1], [0, 1]]
    A = np.array([[0.1, 0.7, 0.2], [0.7, 0.1, 0.0], [0.0, 0.2, 0.9]], np.float32)
    # segment [0, 2): row maxima 0.7, 0.7, 0.2 -> the first maximum, row 0; [2, 3): row 2; [3, 3) has no frame of A
    assert R.markup_phones(A, [[0, 2], [2, 3], [3, 3]]) == [0, 2, -1]
    # an empty segment [1, 1) reads frame 1 (max(en, st + 1))
    assert R.markup_phones(A, [[1, 1]]) == [0]


def test_kernels_have_no_f64_fma_flat_or_scratch(tmp_path):
    import subprocess
    src = os.path.join(ROOT, 'phones-las_amd', 'csrc', 'align.hip')
    out = str(tmp_path / 'align.s')
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    subprocess.check_call([hipcc, '-O3', '--offload-arch=gfx950', '-std=c++17', '-Wno-unused-value', '-S', '--cuda-device-only',
                           src, '-o', out], stderr=subprocess.DEVNULL)
    text = open(out).read()
    import re
    assert 'dtw_kernel' in text and 'frame_binf_count_kernel' in text
    assert not re.search(r'^\s*v_fma_f64|^\s*v_fmac_f64', text, re.M)
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import check_isa
    assert check_isa.scan(out) == []
    assert 'wave_shr:1' in text                             # the row above arrives by DPP, not through LDS


def test_infer_refusals(tmp_path):
    import infer
    base = ['--data', 'x.tfr', '--vocab', 'v.txt', '--model_dir', str(tmp_path)]
    with pytest.raises(SystemExit, match='convert_targets_to_ipa'):
        infer.main(infer.parse_args(base + ['--convert_targets_to_ipa']))
    with pytest.raises(SystemExit, match='beam_width'):
        infer.main(infer.parse_args(base + ['--calc_frame_binf_accuracy', '--beam_width', '2', '--plain_targets', 'p.csv']))
    with pytest.raises(SystemExit, match='plain_targets'):
        infer.main(infer.parse_args(base + ['--calc_frame_binf_accuracy']))
    with pytest.raises(SystemExit, match='mapping_for_frame_accuracy'):
        infer.main(infer.parse_args(base + ['--calc_frame_binf_accuracy', '--plain_targets', 'p.csv']))
