"""Time of the frame-accuracy DTW (phones-las_amd/frame_binf.dtw_ragged -> csrc/align.hip las_attention_dtw_batch) against the
host restatement (tests/frame_binf_restated.align, the reference's arithmetic in plain Python as fastdtw runs it).

Two batches of seeded softmax-row attention matrices: N utterances with U in [30, 50] phones and T' in [180, 220] frames (the
TIMIT test set's size and shape at a 40-ms encoder step), and LONG_N utterances of U = 300, T' = 1000 (several 64-row bands,
backpointers in the device workspace).  Device events around REPS launches of the kernel alone (operands already on the
device); the host restatement is timed on the first HOST_N utterances (2 of the long batch) and scaled to the batch.  The kernel's
outputs are checked against the restatement on those utterances.  Env: N (default 1700), LONG_N (64), REPS (20), HOST_N (40),
OUT (a JSON file for the numbers; optional)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phones_las_amd import frame_binf as fb, hip  # noqa: E402
import tests.frame_binf_restated as R  # noqa: E402

N = int(os.environ.get('N', '1700'))
LONG_N = int(os.environ.get('LONG_N', '64'))
REPS = int(os.environ.get('REPS', '20'))
HOST_N = int(os.environ.get('HOST_N', '40'))


def softmax_rows(rng, U, T):
    z = rng.standard_normal((U, T)) * 3.0 - 0.05 * (np.arange(T)[None, :] - np.linspace(0, T - 1, U)[:, None]) ** 2
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def batch(shapes, seed):
    rng = np.random.default_rng(seed)
    mats = [softmax_rows(rng, U, T) for U, T in shapes]
    offs = np.cumsum([0] + [m.size for m in mats])[:-1]
    buf = torch.as_tensor(np.concatenate([m.reshape(-1) for m in mats])).cuda()
    return mats, buf, offs


def time_case(name, shapes, seed, host_n):
    mats, buf, offs = batch(shapes, seed)
    rows = [m.shape[0] for m in mats]
    cols = [m.shape[1] for m in mats]
    out = fb.dtw_ragged(buf, offs, rows, cols, cols)
    d_offs, d_rows, d_cols, d_lds, ws = out['_keep']
    n = len(mats)
    u_max, t_max = max(rows), max(cols)
    ws_bytes = 0 if ws is None else ws.numel()
    L = hip.lib()

    def launch():
        hip.check(L.las_attention_dtw_batch(hip.p(buf), hip.p(d_offs), hip.p(d_rows), hip.p(d_cols), hip.p(d_lds), n, u_max, t_max,
                                            hip.p(out['out_off']), hip.p(out['run_lo']), hip.p(out['run_hi']), hip.p(out['ph_st']),
                                            hip.p(out['ph_en']), hip.p(out['n_seg']), hip.p(ws), ws_bytes, hip.stream()))
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        launch()
    e1.record()
    torch.cuda.synchronize()
    kernel_ms = e0.elapsed_time(e1) / REPS
    # the host restatement on the first HOST_N utterances, checked against the kernel's outputs
    k = min(host_n, n)
    host = {key: out[key].cpu().numpy() for key in ('run_lo', 'run_hi', 'ph_st', 'ph_en', 'n_seg')}
    oo = out['out_off_np']
    t0 = time.perf_counter()
    ref = [R.align(mats[u]) for u in range(k)]
    host_s = (time.perf_counter() - t0) * n / k
    for u in range(k):
        a, b = oo[u], oo[u + 1]
        lo, hi, st, en, ns = ref[u]
        assert host['n_seg'][u] == ns and np.array_equal(host['run_lo'][a:b], lo) and np.array_equal(host['run_hi'][a:b], hi)
        assert np.array_equal(host['ph_st'][a:b], st) and np.array_equal(host['ph_en'][a:b], en)
    cells = float(sum(U * T for U, T in shapes))
    row = {'case': name, 'utterances': n, 'cells': cells, 'workspace_bytes': ws_bytes, 'kernel_ms': kernel_ms,
           'host_restatement_s': host_s, 'speedup': host_s * 1e3 / kernel_ms, 'gcells_per_s': cells / kernel_ms / 1e6,
           'host_sample': k}
    print('%-6s %5d utt  %.2e cells  kernel %8.3f ms  (%.2f Gcells/s)  host %8.1f s (from %d utt)  x%.0f  workspace %d B' % (
        name, n, cells, kernel_ms, row['gcells_per_s'], host_s, k, row['speedup'], ws_bytes))
    return row


def main():
    rng = np.random.default_rng(0)
    shapes = [(int(rng.integers(30, 51)), int(rng.integers(180, 221))) for _ in range(N)]
    rows = [time_case('timit', shapes, 1, HOST_N), time_case('long', [(300, 1000)] * LONG_N, 2, 2)]
    if os.environ.get('OUT'):
        with open(os.environ['OUT'], 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
