#!/usr/bin/env python3
"""Time one step of `ds_dmc_step` (csrc/ds_dmc.h) beside what it is made of and what it replaces, on the same box in the same run:
`ds_local_energy` (energy chain + Ewald: the cost model of a step -- one chain pass) and one move of `ds_mcmc_step_importance`
(two gradient-chain passes per move) at the same B.  Case: bcc-Li (24 electrons), B = 4096, float64.
Prints one JSON line: ms per DMC step with the comb on every step and without any, ms per `ds_local_energy`, ms per importance
move, the ratio step / local_energy, `outside_chain` = 1 - local_energy / step (the share of a step that the chain pass does not
account for: the kernels of ds_dmc.h, the gradient half of k_combine, launch gaps) and ms of the comb alone (`ds_dmc_branch`).
usage: python tools/dmc_bench.py [--reps R] [--steps S] [--batch B] [--once]
`--once`: one call and no timing -- the run to put under a kernel trace for the share of the k_dmc_* kernels."""
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
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--tau', type=float, default=0.01)
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    cell, klist = systems.build('bcc_li')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    B, S = args.batch, args.steps
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), device='cuda')
    state = sysd.dmc_state(x)
    sysd.dmc_step(params, state, 1, args.tau, branch_every=0, state_valid=False)          # initialise once
    e0 = float(state['eloc'][torch.isfinite(state['eloc'])].mean())
    kw = dict(e_trial=e0, e_ref=e0, e_cut=0.2 * (sysd.n / args.tau) ** 0.5)
    step = lambda every: sysd.dmc_step(params, state, S, args.tau, branch_every=every, **kw)
    if args.once:
        step(1)
        torch.cuda.synchronize()
        return
    ms_comb = timed(lambda: step(1), args.reps) / S
    ms_plain = timed(lambda: step(0), args.reps) / S
    ms_energy = timed(lambda: sysd.local_energy(params, x), args.reps)
    lp = torch.empty(B, dtype=x.dtype, device='cuda')
    xi = x.clone()
    ms_imp = timed(lambda: sysd.mcmc_step(params, xi, lp, S, 0.05, importance=True), args.reps) / S
    ms_branch = timed(lambda: sysd.dmc_branch(state, 0.5, want_parents=False), args.reps)
    print(json.dumps({'case': 'bcc_li', 'electrons': sysd.n, 'B': B, 'steps_per_call': S, 'tau': args.tau,
                      'dmc_step_ms': round(ms_comb, 3), 'dmc_step_no_comb_ms': round(ms_plain, 3), 'local_energy_ms': round(ms_energy, 3),
                      'importance_move_ms': round(ms_imp, 3), 'ratio': round(ms_comb / ms_energy, 4),
                      'outside_chain': round(1.0 - ms_energy / ms_comb, 4), 'branch_ms': round(ms_branch, 3),
                      'total_weight': float(state['weight'].sum())}))


if __name__ == '__main__':
    main()
