#!/usr/bin/env python3
"""Cost of the KFAC device calls beside the log-psi VJP: bcc-Li 24 e-, float64, B = 4096 walkers, device events around single calls
of `ds_kfac_factors`, `ds_kfac_inverses`, `ds_kfac_precondition` and `ds_logpsi_vjp` in ONE process, 3 warm-up + 10 timed calls
each, the four alternating.  The factor pass is the VJP plus the symmetric rank-k contractions of csrc/ds_kfac.h (by count about
10 GFLOP per one-electron layer); the inverses and the preconditioner do not depend on the batch.  `share_of_iteration` relates
each call to one KFAC training iteration counted as energy gradient (`ds_logpsi_vjp`) + factor pass + inverses + preconditioner:
the local energy and the moves, which both optimizers pay alike, are left out, so the shares are upper bounds.
usage: python tools/kfac_bench.py [--batch 4096] [--calls 10] [--out FILE.json]   -> one JSON line"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepsolid_amd import network, systems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a timing from anywhere else says nothing'
    cell, klist = systems.build('bcc_li')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    x = torch.as_tensor(systems.synthetic_walkers(cell, a.batch), device='cuda')
    cot = torch.as_tensor(np.random.default_rng(1).normal(size=(a.batch, 2)) / a.batch, device='cuda')
    factors, grad_seed = sysd.kfac_factors(params, x, flat=True)
    factors = factors.clone()
    inverses = sysd.kfac_inverses(factors, 1.0, 1e-3)
    v = grad_seed.index_select(0, sysd.kfac_index(params)['v_src'])
    calls = {'ds_kfac_factors': lambda: sysd.kfac_factors(params, x),
             'ds_kfac_inverses': lambda: sysd.kfac_inverses(factors, 1.0, 1e-3),
             'ds_kfac_precondition': lambda: sysd.kfac_precondition(inverses, v),
             'ds_logpsi_vjp': lambda: sysd.logpsi_vjp(params, x, cot)}
    ms = {k: [] for k in calls}
    for i in range(a.warmup + a.calls):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    out = {'system': 'bcc_li', 'dtype': 'f64', 'batch': a.batch, 'calls': a.calls, 'warmup': a.warmup}
    for k, v in ms.items():
        out[k] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)}
    out['ratio_factors_over_vjp'] = out['ds_kfac_factors']['median_ms'] / out['ds_logpsi_vjp']['median_ms']
    total = sum(out[k]['median_ms'] for k in calls)
    out['share_of_iteration'] = {k: out[k]['median_ms'] / total for k in calls}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
