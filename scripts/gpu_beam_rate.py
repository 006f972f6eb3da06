"""Beam-search rate of LasModel.predict (beam_width > 0): the device route (one las_beam_advance per step, one ledger read per
window, las_beam_gather_tree) against the host loop (LAS_BEAM_HOST=1: the token-by-token loop with gather_tree in Python),
interleaved in one process.

    python scripts/gpu_beam_rate.py                   # metric-M K 4, cfg1 K 8, default-arch K 4, cfg1 with 2 100 classes K 8
    python scripts/gpu_beam_rate.py --shape cfg1      # one shape, in this process

Without --shape the script starts one child process per shape, each under its own `timeout`, and stops at the first child that
fails (nothing more is started on a device after a fault or a hang).  A child builds the model at the shape of bench.py's
CONFIGS, trains it for --train-steps optimiser steps on ONE synthetic ragged batch (so that beams end at different steps), and
times predict() after --warmup rounds: --reps rounds, every round running each route once (A B A B ...: drift hits both), wall
clock around a synchronise (the host route's cost is mostly on the host, so HIP events would miss it).  Medians are reported; the
listener's forward pass is timed alone the same way, so that `us_per_step` is the DECODER's cost per search step:
(predict - listener) / steps.  The large-vocabulary shape runs the device route alone: the host loop's las_beam_step refuses it.

One JSON line per shape: ms per decode, us per step, advance launches and host synchronisations per decode for both routes, and
whether the two routes returned the same beams.  Reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (bench.py config, overrides, beam width, host route runs)
SHAPES = {
    'metric-M': ('metric-M', {}, 4, True),
    'cfg1': ('cfg1', {}, 8, True),
    'default-arch': ('default-arch', {}, 4, True),
    'cfg1-V2100': ('cfg1', {'V': 2100}, 8, False),
}


def timed(fn, torch):
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - w0) * 1e3, out


def run_shape(name, train_steps, reps, warmup, lr):
    import torch
    import bench
    from phones_las_amd import model_helper as mh
    from phones_las_amd.las import ops
    cfg, over, K, host_runs = SHAPES[name]
    c = dict(bench.CONFIGS[cfg], ragged=True, dropout=0.0, sampling=0.0)
    c.update(over)
    params = bench.build_params(c, lr=lr)
    model = mh.LasModel(params, seed=11)
    feats, labels = bench.synthetic_batch(c, 0, 'cuda')
    first = last = None
    for _ in range(train_steps):
        last = float(model.train_step(feats, labels))
        first = last if first is None else first
    model.check_device_status()
    model.params.decoder.set_hparam('beam_width', K)
    env = os.environ

    def route(host):
        def fn():
            env['LAS_BEAM_HOST'] = '1' if host else '0'
            pred = model.predict(feats)
            sp = model._beam_speller()
            return (pred['sample_ids'], pred['beam_lengths'], pred['beam_log_probs'], sp.last_decode_route, sp.last_decode_launches,
                    sp.last_decode_syncs)
        return fn

    def listener():
        return model.listener.forward(feats['encoder_inputs'], feats['source_sequence_length'], ops.PREDICT)

    variants = {'device': route(False)}
    if host_runs:
        variants['host'] = route(True)
    variants['listener'] = listener
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    wall = {k: [] for k in variants}
    info = {}
    for _ in range(reps):
        for k, fn in variants.items():
            w, out = timed(fn, torch)
            wall[k].append(w)
            if k != 'listener':
                info[k] = out
    model.check_device_status()
    lis = statistics.median(wall['listener'])
    res = {'shape': name, 'B': c['B'], 'T': c['T'], 'V': c['V'], 'beam_width': K, 'train_steps': train_steps,
           'train_loss': [round(first, 4), round(last, 4)] if train_steps else None, 'reps': reps, 'listener_ms': round(lis, 3),
           'routes': {}}
    for k, out in info.items():
        ids, lens, lps, rt, launches, syncs = out
        steps = int(ids.shape[1])
        w = statistics.median(wall[k])
        # the host loop synchronises once per step (bool(finished.all())) and three times at the end (the copies for gather_tree)
        res['routes'][k] = {'route': rt, 'search_steps': steps, 'beam_len_min_max': [int(lens.min()), int(lens.max())],
                            'advance_launches': launches, 'host_syncs': syncs if rt == 'beam_device' else steps + 3,
                            'predict_ms': round(w, 3), 'predict_ms_min_max': [round(min(wall[k]), 3), round(max(wall[k]), 3)],
                            'decode_ms': round(w - lis, 3), 'us_per_step': round((w - lis) * 1e3 / max(steps, 1), 2)}
    if host_runs:
        d, h = info['device'], info['host']
        res['routes_agree'] = bool(d[0].shape == h[0].shape and torch.equal(d[0], h[0]) and torch.equal(d[1], h[1]) and
                                   torch.equal(d[2].view(torch.int32), h[2].view(torch.int32)))
        res['host_over_device_decode'] = round(res['routes']['host']['decode_ms'] / res['routes']['device']['decode_ms'], 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=sorted(SHAPES))
    ap.add_argument('--train-steps', type=int, default=100)
    ap.add_argument('--lr', type=float, default=2e-3)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--timeout', type=int, default=240, help='seconds per shape (child process)')
    a = ap.parse_args()
    if a.shape:
        run_shape(a.shape, a.train_steps, a.reps, a.warmup, a.lr)
        return 0
    for name in SHAPES:
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--shape', name,
               '--train-steps', str(a.train_steps), '--lr', str(a.lr), '--reps', str(a.reps), '--warmup', str(a.warmup)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print('gpu_beam_rate: %s ended with status %d; nothing more is started' % (name, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == '__main__':
    sys.exit(main())
