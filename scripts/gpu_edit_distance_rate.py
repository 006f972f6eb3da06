"""Time of the edit-distance metric on the device (phones-las_amd/utils/metrics_utils.edit_distance_on_device / levenshtein_lists
-> csrc/metrics.hip las_edit_distance_batch) against the host path (metrics_utils.edit_distance / _levenshtein, plain Python),
both interleaved in one process (A B A B ...: drift hits both), medians of REPS rounds after a warm-up.

Shapes: 64 x 80 and 64 x 200 random id rows (alphabet 61, EOS 2) in evaluate's form -- the host path starts from the ids on the
device, as evaluate's did (its copy to lists is part of it), the device path ends with the B integer triples on the host; and
UTT utterances x 4 beams of 25..60 symbols in infer.py's one-launch form, both sides starting from Python lists.  Wall clock
around work that ends in a synchronise (the copy back); for the device path the kernel alone is also bracketed by HIP events.
The device results are checked against the host's on every shape.

Then a whole LasModel.evaluate call of the metric-M model of bench.py's CONFIGS (B = 64, T = 800, ragged targets, trained for
TRAIN_STEPS steps on the batch so that hypotheses end at different steps), with LAS_HOST_METRICS set and unset, interleaved the
same way; the returned edit distances of the two must be equal.

Env: REPS (default 7), UTT (1344), TRAIN_STEPS (100), OUT (a JSON file for the numbers; optional).  Reads nothing outside the
repository."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phones_las_amd import hip  # noqa: E402
from phones_las_amd.utils import metrics_utils as mu  # noqa: E402

REPS = int(os.environ.get('REPS', '7'))
UTT = int(os.environ.get('UTT', '1344'))
TRAIN_STEPS = int(os.environ.get('TRAIN_STEPS', '100'))
EOS = 2


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def interleaved(variants, warmup=2):
    """{name: (median ms, min, max)} and the last result of each variant."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    ms = {k: [] for k in variants}
    out = {}
    for _ in range(REPS):
        for k, fn in variants.items():
            t, out[k] = wall(fn)
            ms[k].append(t)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}, out


def kernel_ms(launch, reps=50):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def row(name, ms, extra):
    r = {'case': name, 'host_ms': round(ms['host'][0], 3), 'host_ms_min_max': [round(x, 3) for x in ms['host'][1:]],
         'device_ms': round(ms['device'][0], 3), 'device_ms_min_max': [round(x, 3) for x in ms['device'][1:]],
         'host_over_device': round(ms['host'][0] / ms['device'][0], 1)}
    r.update(extra)
    print(json.dumps(r), flush=True)
    return r


def evaluate_form(B, S, seed):
    rng = np.random.default_rng(seed)
    hyp = torch.as_tensor(rng.integers(0, 61, (B, S)).astype(np.int32)).cuda()
    ref = torch.as_tensor(rng.integers(0, 61, (B, S)).astype(np.int32)).cuda()
    ms, out = interleaved({'host': lambda: mu.edit_distance(hyp, ref, EOS), 'device': lambda: mu.edit_distance_on_device(hyp, ref, EOS)})
    assert out['host'] == out['device']
    k = kernel_ms(lambda: mu.edit_distance_device(hyp, ref, EOS))
    return row('evaluate %d x %d' % (B, S), ms, {'device_enqueue_and_kernel_ms': round(k, 4)})


def infer_form(n_utt, K, seed):
    rng = np.random.default_rng(seed)
    refs = [rng.integers(0, 61, int(rng.integers(25, 61))).tolist() for _ in range(n_utt)]
    hyps, roh = [], []
    for u, t in enumerate(refs):
        for _ in range(K):                              # a beam: the target with a tenth of its symbols redrawn, one dropped
            h = [int(rng.integers(0, 61)) if rng.random() < 0.1 else x for x in t]
            del h[int(rng.integers(0, len(h)))]
            hyps.append(h)
            roh.append(u)

    def host():
        return [mu._levenshtein(h, refs[u]) for h, u in zip(hyps, roh)]

    ms, out = interleaved({'host': host, 'device': lambda: mu.levenshtein_lists(hyps, refs, roh)}, warmup=1)
    assert out['host'] == out['device']
    return row('infer %d utterances x %d beams' % (n_utt, K), ms, {'pairs': len(hyps)})


def whole_evaluate():
    import bench
    from phones_las_amd import model_helper as mh
    c = dict(bench.CONFIGS['metric-M'], ragged=True, dropout=0.0, sampling=0.0)
    model = mh.LasModel(bench.build_params(c, lr=2e-3), seed=11)
    feats, labels = bench.synthetic_batch(c, 0, 'cuda')
    for _ in range(TRAIN_STEPS):
        model.train_step(feats, labels)
    model.check_device_status()

    def route(host):
        def fn():
            os.environ['LAS_HOST_METRICS'] = '1' if host else '0'
            return model.evaluate(feats, labels)[1]
        return fn

    ms, out = interleaved({'host': route(True), 'device': route(False)})
    os.environ.pop('LAS_HOST_METRICS', None)
    model.check_device_status()
    assert out['host'] == out['device']
    return row('LasModel.evaluate metric-M B=%d' % c['B'], ms, {'train_steps': TRAIN_STEPS, 'mean_edit_distance': float(np.mean(out['device']))})


def main():
    hip.lib()
    rows = [evaluate_form(64, 80, 1), evaluate_form(64, 200, 2), infer_form(UTT, 4, 3), whole_evaluate()]
    if os.environ.get('OUT'):
        with open(os.environ['OUT'], 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
