#!/usr/bin/env python3
"""Time `ds_stress` (the strain derivative of the energy, csrc/ds_stress.h) beside `ds_ewald` (the Ewald energy of the same walkers:
the same real-space pairs and structure factors, three numbers per walker instead of 24), `ds_ion_forces` and `ds_logpsi_grad` (the
gradient the kinetic row needs: what a `StressTensor.update` pays on top).  Case: bcc-Li (24 electrons, 8 ions), B = 4096, float64.
Prints one JSON line: ms per call of `stress` with the walker outputs, with the packed sums only, without a gradient (the Ewald rows
alone), of `ewald`, `ion_forces` and `logpsi_grad`, and the ratios stress / ewald and stress / logpsi_grad.
usage: python tools/stress_bench.py [--reps R] [--batch B] [--case NAME] [--once]
`--once`: one call and no timing -- the run to put under `rocprofv3 --kernel-trace --stats` for k_stress / k_stress_part /
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
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), device='cuda')
    grad = sysd.logpsi_grad(params, x)[1]
    drift = grad.real.contiguous()
    sums = torch.zeros(49, dtype=torch.float64, device='cuda')
    if args.once:
        sysd.stress(x, grad, sums=sums)
        torch.cuda.synchronize()
        return
    ms_walker = timed(lambda: sysd.stress(x, grad), args.reps)
    ms_sums = timed(lambda: sysd.stress(x, grad, sums=sums, want_walker=False), args.reps)
    ms_ewald_rows = timed(lambda: sysd.stress(x), args.reps)
    ms_ewald = timed(lambda: sysd.ewald(x), args.reps)
    ms_forces = timed(lambda: sysd.ion_forces(x, drift), args.reps)
    ms_grad = timed(lambda: sysd.logpsi_grad(params, x), max(1, args.reps // 3))
    out = sysd.stress(x, grad)
    print(json.dumps({'case': args.case, 'electrons': sysd.n, 'ions': len(cell.atom_charges()), 'B': B, 'dtype': 'float64',
                      'stress_ms': round(ms_walker, 4), 'stress_sums_only_ms': round(ms_sums, 4),
                      'stress_no_grad_ms': round(ms_ewald_rows, 4), 'ewald_ms': round(ms_ewald, 4), 'ion_forces_ms': round(ms_forces, 4),
                      'logpsi_grad_ms': round(ms_grad, 3), 'stress_over_ewald': round(ms_walker / ms_ewald, 2),
                      'stress_over_logpsi_grad': round(ms_walker / ms_grad, 4), 'n_bad': int(out['n_bad']),
                      'good_walkers_in_sums': float(sums[48]) / (args.reps + 1)}))


if __name__ == '__main__':
    main()
