"""Host-side contract of the one-launch greedy decode (no GPU): the decision table of las_decoder_persist_greedy_supported,
every refusal of las_decoder_persist_fwd with the greedy flag (each comes back as an error code with a las_last_error()
message that names the field, before anything is enqueued), and the library version.  The library is loaded as
tests/test_abi.py loads it."""
import ctypes as C

import pytest

LUONG, BAHDANAU, CUSTOM, LUONG_MONO = 0, 1, 2, 3
SOFTMAX, MONO_PARALLEL = 0, 1


@pytest.fixture(scope='module')
def hip():
    from phones_las_amd import hip as h
    h.lib()
    return h


def test_version_is_105(hip):
    assert hip.lib().las_version() == 105


def test_greedy_supported_decision_table(hip):
    sup = hip.lib().las_decoder_persist_greedy_supported
    # (Hd, M, K_in, K1_in, attention, norm, wiring, A, Vp)
    for Hd in (128, 256):
        for att in (LUONG, BAHDANAU):
            assert sup(Hd, 128, 128 + Hd, 0, att, SOFTMAX, 0, 0, 16) == 1                       # one cell (lean path)
            assert sup(Hd, 128, 128 + Hd, 2 * Hd, att, SOFTMAX, 0, 0, 104) == 1                 # two cells, MultiRNNCell wiring
            assert sup(Hd, 128, 128 + Hd, 2 * 128 + Hd, att, SOFTMAX, 1, 0, 104) == 1           # two cells, --bottom_only wiring
    assert sup(128, 128, 256, 0, LUONG, SOFTMAX, 0, 0, 1024) == 1
    assert sup(128, 128, 256, 0, LUONG, SOFTMAX, 0, 0, 1025) == 0                               # the logits row in LDS
    assert sup(128, 128, 256, 0, LUONG, SOFTMAX, 0, 0, 0) == 0
    for Hd in (64, 512, 1024):                                                                  # other decoder widths: step path
        assert sup(Hd, 128, 128 + Hd, 0, LUONG, SOFTMAX, 0, 0, 16) == 0
    assert sup(128, 128, 256, 0, CUSTOM, SOFTMAX, 0, 0, 16) == 0
    assert sup(128, 128, 256, 0, LUONG_MONO, MONO_PARALLEL, 0, 0, 16) == 0                      # monotonic attentions
    assert sup(128, 128, 256, 0, LUONG, MONO_PARALLEL, 0, 0, 16) == 0
    assert sup(128, 128, 256, 0, LUONG, SOFTMAX, 0, 64, 16) == 0                                # attention layer
    assert sup(128, 128, 224, 0, LUONG, SOFTMAX, 0, 0, 16) == 0                                 # K_in: whole 128-byte lines
    assert sup(128, 2048, 2048 + 128, 0, LUONG, SOFTMAX, 0, 0, 16) == 0                         # K_in / 32 > 48
    assert sup(128, 120, 256, 0, LUONG, SOFTMAX, 0, 0, 16) == 0                                 # M % 32
    assert sup(128, 128, 256, 3 * 128, LUONG, SOFTMAX, 0, 0, 16) == 0                           # K1_in of neither wiring
    assert sup(128, 128, 256, 2 * 128, LUONG, SOFTMAX, 1, 0, 16) == 0                           # ... of the other wiring
    assert sup(128, 128, 256, 2 * 128, LUONG, SOFTMAX, 2, 0, 16) == 0


def _valid(hip, keep):
    """A greedy las_dec_persist that passes every check (one cell, Hd = 128, M = 128); the pointers are never followed: each
    case below is refused before the launch.  `keep` holds the buffers the fake addresses point into."""
    buf = C.create_string_buffer(4096 + 256)
    keep.append(buf)
    a = (C.addressof(buf) + 127) // 128 * 128            # (x and the workspace: whole 128-byte lines)
    p = hip.DecPersist()
    s = p.s
    s.B, s.Hd, s.M, s.Tm, s.attention, s.mode, s.norm = 3, 128, 128, 6, LUONG, 0, SOFTMAX
    s.tok_rows, s.tok_ids, s.tok_stride, s.drop_keep = a, a, 8, 1.0
    p.U, p.K_in, p.inc_tok = 8, 256, 1
    p.x, p.kT, p.workspace = a, a, a
    p.greedy, p.eos_id, p.V, p.Vp = 1, 2, 11, 16
    p.logits, p.ld_logits, p.sample_ids, p.ld_samples = a, 8 * 16, a, 8
    p.finished, p.final_len, p.wprojT, p.ldw, p.bproj, p.plog = a, a, a, 128, a, a
    p.step_begin, p.step_end = 0, 4
    return p


REFUSALS = [
    ('logits', lambda p: setattr(p, 'logits', 0)),
    ('sample_ids', lambda p: setattr(p, 'sample_ids', 0)),
    ('finished', lambda p: setattr(p, 'finished', 0)),
    ('final_len', lambda p: setattr(p, 'final_len', 0)),
    ('wprojT', lambda p: setattr(p, 'wprojT', 0)),
    ('bproj', lambda p: setattr(p, 'bproj', 0)),
    ('plog', lambda p: setattr(p, 'plog', 0)),
    ('inc_tok', lambda p: setattr(p, 'inc_tok', 2)),
    ('step_begin', lambda p: (setattr(p, 'step_begin', 5), setattr(p, 'step_end', 4))),
    ('step_end', lambda p: setattr(p, 'step_end', 9)),                    # beyond the capacity U = 8
    ('step_begin', lambda p: setattr(p, 'step_begin', -1)),
    ('sampling_prob', lambda p: setattr(p, 'sampling_prob', 0.1)),
    ('drop_keep', lambda p: setattr(p.s, 'drop_keep', 0.8)),
    ('not supported', lambda p: (setattr(p.s, 'Hd', 512), setattr(p, 'K_in', 640))),
    ('not supported', lambda p: setattr(p, 'Vp', 1032)),
    ('not supported', lambda p: setattr(p.s, 'attention', CUSTOM)),
    ('eos_id', lambda p: setattr(p, 'eos_id', 11)),
]


@pytest.mark.parametrize('field,spoil', REFUSALS, ids=['%s-%d' % (f, i) for i, (f, _) in enumerate(REFUSALS)])
def test_greedy_launch_refusals_name_the_field(hip, field, spoil):
    keep = []
    p = _valid(hip, keep)
    spoil(p)
    rc = hip.lib().las_decoder_persist_fwd(C.byref(p), None)
    assert rc != 0
    msg = hip.lib().las_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert 'greedy' in msg and field in msg, msg


def test_whole_capacity_window_is_zero_zero(hip):
    """step_begin = step_end = 0 means [0, U): the window check accepts it (the case is then refused for a later field only)."""
    keep = []
    p = _valid(hip, keep)
    p.step_begin, p.step_end = 0, 0
    p.emb = 1                                           # a dense token feed without the second cell: refused after the window check
    rc = hip.lib().las_decoder_persist_fwd(C.byref(p), None)
    msg = hip.lib().las_last_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert rc != 0 and 'emb' in msg, msg
