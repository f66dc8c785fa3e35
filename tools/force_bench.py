#!/usr/bin/env python3
"""Time `ds_ion_forces` (the ionic-force call, csrc/ds_force.h) beside `ds_ewald` (the Ewald energy of the same walkers: the same
real-space pairs and structure factors, one number per walker instead of 6 A) and `ds_logpsi_grad` (the drift the zero-variance
term needs: what an `IonForces.update` pays on top).  Case: bcc-Li (24 electrons, 8 ions), B = 4096, float64.
Prints one JSON line: ms per call of `ion_forces` with the walker outputs, with the packed sums only (what the accumulator runs),
of `ewald` and of `logpsi_grad`, and the ratios forces / ewald and forces / logpsi_grad.
usage: python tools/force_bench.py [--reps R] [--batch B] [--case NAME] [--once]
`--once`: one call and no timing -- the run to put under `rocprofv3 --kernel-trace --stats` for k_ion_forces / k_force_part /
k_force_final."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepsolid_amd import network, systems


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--case', default='bcc_li', choices=sorted(systems.SYSTEMS))
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    cell, klist = systems.build(args.case)
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    B = args.batch
    A = len(cell.atom_charges())
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), device='cuda')
    drift = sysd.logpsi_grad(params, x)[1].real.contiguous()
    sums = torch.zeros(12 * A + 1, dtype=torch.float64, device='cuda')
    if args.once:
        sysd.ion_forces(x, drift, sums=sums)
        torch.cuda.synchronize()
        return
    ms_walker = timed(lambda: sysd.ion_forces(x, drift), args.reps)
    ms_sums = timed(lambda: sysd.ion_forces(x, drift, sums=sums, want_walker=False), args.reps)
    ms_hf = timed(lambda: sysd.ion_forces(x), args.reps)
    ms_ewald = timed(lambda: sysd.ewald(x), args.reps)
    ms_grad = timed(lambda: sysd.logpsi_grad(params, x), max(1, args.reps // 3))
    out = sysd.ion_forces(x, drift)
    print(json.dumps({'case': args.case, 'electrons': sysd.n, 'ions': A, 'B': B, 'dtype': 'float64',
                      'ion_forces_ms': round(ms_walker, 4), 'ion_forces_sums_only_ms': round(ms_sums, 4),
                      'ion_forces_hf_only_ms': round(ms_hf, 4), 'ewald_ms': round(ms_ewald, 4), 'logpsi_grad_ms': round(ms_grad, 3),
                      'forces_over_ewald': round(ms_walker / ms_ewald, 2), 'forces_over_logpsi_grad': round(ms_walker / ms_grad, 4),
                      'n_bad': int(out['n_bad']), 'good_walkers_in_sums': float(sums[12 * A]) / (args.reps + 1)}))


if __name__ == '__main__':
    main()
