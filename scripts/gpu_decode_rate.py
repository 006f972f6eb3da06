"""Decode rate of LasModel.predict (greedy): the one-launch route against the step-by-step path, interleaved in one process.

    python scripts/gpu_decode_rate.py                 # metric-M (with the window sweep 16 / 32 / 64), cfg1, default-arch
    python scripts/gpu_decode_rate.py --shape cfg1    # one shape, in this process

Without --shape the script starts one child process per shape, each under its own `timeout`, and stops at the first child
that fails (nothing more is started on a device after a fault or a hang).  A child builds the model at the shape of
bench.py's CONFIGS (B = 64, T = 800 -> T' = 200 at metric-M), trains it for --train-steps optimiser steps on ONE synthetic
ragged batch (U_i = U - (i mod 17): utterances then end at different decode steps), and times predict() after a warm-up:
--reps rounds, every round running each route once (A B A B ...: drift hits both), each run bracketed by HIP events on
the stream and by wall clock around a synchronise.  Medians are reported; the listener's forward pass is timed alone the
same way, so that `us_per_step` is the DECODER's cost per decoded step: (predict - listener) / steps.

One JSON line per shape: utterances/s, us per decoded step and launches per decode for both routes, their ratio, the decode
length, and (metric-M) the window sweep.  Reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ('metric-M', 'cfg1', 'default-arch')
WINDOWS = (16, 32, 64)


def timed(fn, torch):
    """(HIP-event ms, wall ms) of one call, the device idle before and after."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3, out


def run_shape(name, train_steps, reps, warmup, lr):
    import torch
    import bench
    from phones_las_amd import model_helper as mh
    from phones_las_amd.las import ops
    c = dict(bench.CONFIGS[name], ragged=True, dropout=0.0, sampling=0.0)
    params = bench.build_params(c, lr=lr)
    model = mh.LasModel(params, seed=11)
    feats, labels = bench.synthetic_batch(c, 0, 'cuda')
    first = last = None
    for _ in range(train_steps):
        last = float(model.train_step(feats, labels))
        first = last if first is None else first
    model.check_device_status()
    sp = model.speller
    env = os.environ

    def route(persist, window=None):
        def fn():
            env['LAS_DEC_PERSIST_GREEDY'] = '1' if persist else '0'
            if window:
                env['LAS_DEC_GREEDY_WINDOW'] = str(window)
            else:
                env.pop('LAS_DEC_GREEDY_WINDOW', None)
            pred = model.predict(feats)
            return pred['sample_ids'].shape[1], sp.last_decode_route, sp.last_decode_launches, pred['final_sequence_length']
        return fn

    def listener():
        return model.listener.forward(feats['encoder_inputs'], feats['source_sequence_length'], ops.PREDICT)

    variants = {'steps': route(False), 'persist': route(True)}
    if name == 'metric-M':
        for w in WINDOWS:
            variants['persist_w%d' % w] = route(True, w)
    variants['listener'] = listener
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    wall = {k: [] for k in variants}
    info = {}
    for _ in range(reps):
        for k, fn in variants.items():
            e, w, out = timed(fn, torch)
            ev[k].append(e)
            wall[k].append(w)
            if k != 'listener':
                info[k] = out
    model.check_device_status()
    B = c['B']
    lis_e, lis_w = statistics.median(ev['listener']), statistics.median(wall['listener'])
    res = {'shape': name, 'B': B, 'T': c['T'], 'train_steps': train_steps, 'lr': lr, 'train_loss': [round(first, 4), round(last, 4)],
           'reps': reps, 'listener_ms': round(lis_e, 3), 'routes': {}}
    for k in variants:
        if k == 'listener':
            continue
        steps, rt, launches, fl = info[k]
        e, w = statistics.median(ev[k]), statistics.median(wall[k])
        res['routes'][k] = {
            'route': rt, 'decode_steps': steps, 'final_len_min_max': [int(fl.min()), int(fl.max())],
            'launches_per_decode': launches, 'predict_ms_events': round(e, 3), 'predict_ms_wall': round(w, 3),
            'predict_ms_events_min_max': [round(min(ev[k]), 3), round(max(ev[k]), 3)],
            'utterances_per_s': round(B / (w * 1e-3), 1),
            'us_per_step': round((e - lis_e) * 1e3 / steps, 2), 'us_per_step_wall': round((w - lis_w) * 1e3 / steps, 2)}
    r = res['routes']
    res['max_it'] = int(round(int(model.listener.forward(feats['encoder_inputs'], feats['source_sequence_length'], ops.PREDICT)[0][1].max())
                              * params.decoder.decoding_length_factor))
    res['speedup_predict_wall'] = round(r['steps']['predict_ms_wall'] / r['persist']['predict_ms_wall'], 2)
    res['speedup_decoder_per_step'] = round(r['steps']['us_per_step_wall'] / r['persist']['us_per_step_wall'], 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=SHAPES)
    ap.add_argument('--train-steps', type=int, default=300)
    ap.add_argument('--lr', type=float, default=2e-3)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=280, help='seconds per shape (child process)')
    a = ap.parse_args()
    if a.shape:
        run_shape(a.shape, a.train_steps, a.reps, a.warmup, a.lr)
        return 0
    for name in SHAPES:
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--shape', name,
               '--train-steps', str(a.train_steps), '--lr', str(a.lr), '--reps', str(a.reps), '--warmup', str(a.warmup)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print('gpu_decode_rate: %s ended with status %d; nothing more is started' % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
