"""Host side of the device beam search: the C-ABI declares las_beam_advance / las_beam_gather_tree and the ctypes mirrors of
their structs have the header's layout (as tests/test_abi.py checks the older ones); LAS_BEAM_HOST / LAS_BEAM_WINDOW are read
when the call is made; the restatement and the inputs of tests/test_gpu_beam_advance.py hold together on the CPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, 'include', 'las_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_declares_both_entries():
    text = _header()
    assert re.search(r'\bint\s+las_beam_advance\s*\(\s*const\s+las_beam_adv\s*\*', text)
    assert re.search(r'\bint\s+las_beam_gather_tree\s*\(', text)
    from phones_las_amd import hip
    assert 'las_beam_advance' in hip.EXPORTS and 'las_beam_gather_tree' in hip.EXPORTS
    m = re.search(r'LAS_BEAM_MAX_WIDTH\s*=\s*(\d+)\s*,\s*LAS_BEAM_MAX_JOBS\s*=\s*(\d+)', text)
    assert (int(m.group(1)), int(m.group(2))) == (hip.BEAM_MAX_WIDTH, hip.BEAM_MAX_JOBS) and hip.BEAM_MAX_WIDTH >= 32


def test_beam_structs_have_the_layout_of_the_header(tmp_path):
    from phones_las_amd import hip
    pairs = {'las_beam_adv': hip.BeamAdv, 'las_beam_gather_job': hip.BeamGatherJob}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "las_hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append('  printf("%s . %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        c, f, v = line.split()
        got[(c, f)] = int(v)
    for cname, cls in pairs.items():
        assert got[(cname, '.')] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert ctypes.sizeof(hip.BeamAdv) <= 4096               # travels as a kernel argument


def test_set_jobs_refuses_more_than_the_table_holds():
    import pytest
    from phones_las_amd import hip
    with pytest.raises(hip.LasError, match='16'):
        hip.BeamAdv().set_jobs([None] * (hip.BEAM_MAX_JOBS + 1))


def test_switches_are_read_at_call_time(monkeypatch):
    """LAS_BEAM_HOST decides the route in _beam_device_ok at every call; LAS_BEAM_WINDOW is read inside the device loop and
    nowhere at import."""
    from phones_las_amd.las import model, speller_general as sg
    assert model.BEAM_WINDOW == 32
    me = sg.GeneralSpeller.__new__(sg.GeneralSpeller)
    me.NL, me.mono = 2, True
    monkeypatch.delenv('LAS_BEAM_HOST', raising=False)
    assert me._beam_device_ok(4) is model.BEAM_DEVICE_DEFAULT
    monkeypatch.setenv('LAS_BEAM_HOST', '1')
    assert me._beam_device_ok(4) is False
    monkeypatch.setenv('LAS_BEAM_HOST', '0')
    assert me._beam_device_ok(4) is True and me._beam_device_ok(33) is False
    me.NL = 8                                                # 17 state rows: more than one launch gathers
    assert me._beam_device_ok(4) is False
    src = inspect.getsource(sg.GeneralSpeller._beam_device_loop)
    assert "os.environ.get('LAS_BEAM_WINDOW'" in src
    module_level = [l for l in inspect.getsource(sg).splitlines() if l and not l.startswith((' ', '#'))]
    assert not any('LAS_BEAM' in l for l in module_level)


def test_restatement_and_inputs_on_the_cpu():
    """The restatement's own bookkeeping, and the properties the GPU tests lean on: every BEYOND case exceeds the old LDS
    limit and keeps all utterances above the margin (so nothing is skipped); the hand-made states select the parents they are
    named after."""
    import tests.beam_advance_restated as A
    import tests.loss_heads_restated as R
    under, pairs = A.beyond_skipped()
    assert under == 0 and pairs == 7 and under <= R.BEAM_SKIP_CAP * pairs
    for name, B, K, V, ldl, eos, seed in A.BEYOND_CASES:
        assert R.beam_lds_bytes(K, V) > 64 * 1024
    for make, want in ((A.parents_0021_inputs, [0, 0, 2, 1]), (A.parents_all_7_inputs, [7] * 8)):
        logits, lp, fin, ln, K, V, eos = make()
        ref = R.beam_step(logits, lp, fin, ln, K, eos)
        assert ref[1].tolist() == [want] and min(ref[5].min(), ref[6].min()) > 0.1
    rows = np.arange(8 * 3).reshape(8, 3)
    got = A.gather_rows(rows, np.array([[0, 0, 2, 1], [3, 3, 3, 3]]))
    assert got[:, 0].tolist() == [0, 0, 6, 3, 21, 21, 21, 21]
    steps, K, V, eos = A.three_step_logits()
    state = (np.array([[0.0, -np.inf]] * 2, dtype=np.float32), np.zeros((2, K), dtype=np.int32), np.zeros((2, K), dtype=np.int32))
    rec = (np.full((4, 4), -7, dtype=np.int32), np.full((4, 4), -7, dtype=np.int32))
    fed = np.full((4, 5), -7, dtype=np.int32)
    led = A.new_ledger(2)
    seen = []
    for t, logits in enumerate(steps):
        A.advance(logits, state, K, eos, t, rec, led, fed=fed)
        seen.append((led['utt_done'].tolist(), led['remaining'], led['steps_done']))
    assert seen == [([0, 0], 2, 0), ([1, 0], 1, 0), ([1, 1], 0, 3)]
    assert (fed[:, 1:4] == rec[0][:, :3]).all() and (fed[:, 0] == -7).all() and (rec[0][:, 3] == -7).all()
    before = [s.copy() for s in state]
    assert A.advance(steps[0], state, K, eos, 3, rec, led, fed=fed) == (None, None, None)
    assert all(np.array_equal(a, b) for a, b in zip(before, state)) and (rec[0][:, 3] == -7).all()
