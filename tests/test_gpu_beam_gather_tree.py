"""las_beam_gather_tree against the Python gather_tree of las/speller_general.py (the yardstick: tf.contrib.seq2seq.gather_tree
restated) on random records: lengths 0, 1, T and beyond T, eos inside the beams, T = 1, K = 1, a column offset."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -7


def _case(B, K, T, L, seed, eos=2, V=6):
    """Records [B K, L + T + 1] (a prefix of L columns and one column behind, both at values that must not be read as steps)."""
    rng = np.random.default_rng(seed)
    U = L + T + 1
    word = rng.integers(0, V, size=(B * K, U)).astype(np.int32)           # (eos = 2 turns up in about a sixth of the entries)
    parent = rng.integers(0, K, size=(B * K, U)).astype(np.int32)
    parent[:, :L] = K + 5                                                  # out of range: never to be followed
    parent[:, L + T:] = K + 5
    lengths = rng.integers(0, T + 3, size=(B, K)).astype(np.int32)
    for i, v in enumerate((0, 1, T, T + 2)[:B * K]):
        lengths.reshape(-1)[i] = v
    if B > 1:
        lengths[1] = 0                                                     # an utterance whose longest beam is empty
        lengths[-1, 0] = T + 2
    return word, parent, lengths, U, eos


@pytest.mark.parametrize('B,K,T,L', [(3, 4, 9, 0), (3, 4, 9, 2), (3, 4, 1, 0), (3, 1, 9, 0), (2, 5, 70, 3)],
                         ids=['B3_K4_T9', 'offset_2', 'T1', 'K1', 'T70_K5_offset_3'])
def test_gather_tree_vs_python(B, K, T, L):
    from phones_las_amd import hip
    from phones_las_amd.las.speller_general import gather_tree
    word, parent, lengths, U, eos = _case(B, K, T, L, 10 * K + T + L)
    ref = gather_tree(word[:, L:L + T].reshape(B, K, T).transpose(2, 0, 1), parent[:, L:L + T].reshape(B, K, T).transpose(2, 0, 1),
                      lengths.max(1), eos).transpose(1, 0, 2)              # [B, T, K]
    assert (ref == eos).any() and (ref != eos).any()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_word, d_parent, d_len = d(word), d(parent), d(lengths)
    out = torch.full((B, T, K), SENT, dtype=torch.int32, device='cuda')
    hip.check(hip.lib().las_beam_gather_tree(hip.p(d_word), hip.p(d_parent), U, L, T, hip.p(d_len), B, K, eos, hip.p(out),
                                             hip.stream()))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ref)


def test_gather_tree_refuses_bad_arguments():
    from phones_las_amd import hip
    lib = hip.lib()
    z = torch.zeros(8, dtype=torch.int32, device='cuda')
    out = torch.full((8,), SENT, dtype=torch.int32, device='cuda')
    for args, word in (((hip.p(z), None, 4, 0, 4, hip.p(z), 1, 2, 0, hip.p(out)), 'null argument'),
                       ((hip.p(z), hip.p(z), 4, 2, 4, hip.p(z), 1, 2, 0, hip.p(out)), 'bad shape')):
        rc = lib.las_beam_gather_tree(*args, hip.stream())
        msg = lib.las_last_error().decode()
        assert rc != 0 and msg.startswith('las_beam_gather_tree') and word in msg, msg
    torch.cuda.synchronize()
    assert (out == SENT).all()
