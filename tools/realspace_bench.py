#!/usr/bin/env python3
"""Cost of one `RealSpaceAccumulator.update` (density on a 48^3 grid of the primitive cell and 256 radial bins up to the
Wigner-Seitz radius) beside `ds_observables` at nq = 4 and one `total_energy` step on the same walkers: device events around
single calls in ONE process, the calls alternating, 3 warm-up + 10 timed calls each.
  bcc_li : bcc-Li 2x2x2, 24 e-, B = 4096, float64
  diamond: diamond 2x2x2, 96 e-, B = 1024, float32
The density-only and pair-only calls are timed as well, to say which part of the launch dominates.  Every time is also given as a
fraction of the `total_energy` step of the same run.
usage: python tools/realspace_bench.py [--case bcc_li|diamond|both] [--calls 10] [--out FILE.json]   -> one JSON line per case"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepsolid_amd import estimator, network, systems, train

CASES = {'bcc_li': dict(system='bcc_li', batch=4096, dtype=torch.float64), 'diamond': dict(system='diamond', batch=1024, dtype=torch.float32)}


def run(name, a):
    c = CASES[name]
    cell, klist = systems.build(c['system'])
    B, dtype = a.batch or c['batch'], c['dtype']
    x = torch.as_tensor(systems.synthetic_walkers(cell, B), dtype=dtype, device='cuda')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', dtype=dtype, **systems.DETNET_DEFAULTS)
    params = net.init(0)
    total_energy = train.make_loss(net.apply, None, cell)
    both = estimator.RealSpaceAccumulator(cell, density_grid=a.grid, pair_bins=a.bins)
    dens = estimator.RealSpaceAccumulator(cell, density_grid=a.grid)
    pair = estimator.RealSpaceAccumulator(cell, pair_bins=a.bins)
    obs = estimator.make_observables(cell, polarization_direction=0, nq=4)
    calls = {'realspace_update': lambda: both.update(x), 'realspace_density_only': lambda: dens.update(x),
             'realspace_pairs_only': lambda: pair.update(x), 'ds_observables_nq4': lambda: obs(x),
             'total_energy': lambda: total_energy(params, x)}
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
    out = {'case': name, 'dtype': 'f64' if dtype == torch.float64 else 'f32', 'batch': B, 'electrons': int(sum(cell.nelec)),
           'grid': [a.grid] * 3, 'radial_bins': a.bins, 'r_max': both.r_max, 'calls': a.calls, 'warmup': a.warmup,
           'density_atomics_per_call': B * int(sum(cell.nelec)), 'pairs_per_call': B * int(sum(cell.nelec)) * (int(sum(cell.nelec)) - 1) // 2}
    step = statistics.median(ms['total_energy'])
    for k, v in ms.items():
        out[k] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v), 'fraction_of_total_energy': statistics.median(v) / step}
    assert both.n_walkers == (a.warmup + a.calls) * B and int(both.density_counts().sum()) == both.n_walkers * int(sum(cell.nelec))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='both', choices=['bcc_li', 'diamond', 'both'])
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--grid', type=int, default=48)
    ap.add_argument('--bins', type=int, default=256)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a timing from anywhere else says nothing'
    lines = [json.dumps(run(name, a)) for name in (('bcc_li', 'diamond') if a.case == 'both' else (a.case,))]
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
