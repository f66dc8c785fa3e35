#!/usr/bin/env python3
"""Time one step of `ds_dmc_step` (csrc/ds_dmc.h) beside what it is made of and what it replaces, on the same box in the same run:
`ds_local_energy` (energy chain + Ewald: the cost model of a step -- one chain pass) and one move of `ds_mcmc_step_importance`
(two gradient-chain passes per move) at the same B.  Case: bcc-Li (24 electrons), B = 4096, float64.
Prints one JSON line: ms per DMC step with the comb on every step and without any, ms per `ds_local_energy`, ms per importance
move, the ratio step / local_energy, `outside_chain` = 1 - local_energy / step (the share of a step that the chain pass does not
account for: the kernels of ds_dmc.h, the gradient half of k_combine, launch gaps) and ms of the comb alone (`ds_dmc_branch`).
usage: python tools/dmc_bench.py [--reps R] [--steps S] [--batch B] [--once] [--ecp [FILE.npz]] [--r-cut-nl R] [--tmoves]
                                 [--forward-walking [LAG,LAG,...]]
`--once`: one call and no timing -- the run to put under a kernel trace for the share of the k_dmc_* kernels.
`--ecp`: the cost of the locality approximation instead, one JSON line: (a) ms per `ds_dmc_step` step, (b) ms per stand-alone
`ds_ecp_energy` call on the same walkers, (c) ms per `ds_dmc_step_ecp` step, and (c) / ((a) + (b)); all with the comb on every
step.  The potential is the one saved in FILE.npz (`SemiLocalECP.save`, built for the bcc-Li cell) or, without a file, the
synthetic species of tools/ecp_bench.py on all 8 atoms with the non-local cutoff `--r-cut-nl` (default 2.747 Bohr), N_q = 12.
`--tmoves` (with `--ecp`): also (d) ms per `ds_dmc_step_tmove` step from the same walkers with the same potential, (d) / (c), the
excess (d) - (c) beside ms per `ds_local_energy` (one chain pass, what the cost model says the excess is), and the T-moves per
walker and step.
`--forward-walking` (without `--ecp`): one JSON line with ms per `dmc.ForwardWalking.update` (lags 0, 4, 16 unless given; density
grid 32^3 on the primitive cell, 128 radial bins, the three built-in scalars) once the ring is full, beside ms per `ds_dmc_step`
step with the comb on every step from the same process, their ratio per block of `--steps` steps, and the bytes the ring holds."""
import argparse
import json
import os
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
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


def bench_ecp(args, cell, sysd, params, x):
    from deepsolid_amd.device import EcpTables
    from deepsolid_amd.pseudopotential import SemiLocalECP
    from ecp_bench import SPECIES
    B, S = args.batch, args.steps
    if args.ecp:
        pot = SemiLocalECP.load(args.ecp, cell)
    else:
        pot = SemiLocalECP(cell, [dict(SPECIES, r_cut_loc=0.8 * args.r_cut_nl, r_cut_nl=args.r_cut_nl)], [0] * 8, n_quad=12)
    ecp = EcpTables(pot)
    plain, state = sysd.dmc_state(x), sysd.dmc_state(x, ecp=True)
    sysd.dmc_step(params, plain, 1, args.tau, branch_every=0, state_valid=False)
    first = sysd.dmc_step(params, state, 1, args.tau, branch_every=0, state_valid=False, ecp=ecp, want_pairs=True)
    cap = first['pair_capacity']
    e0 = float(state['eloc'][torch.isfinite(state['eloc'])].mean())
    kw = dict(e_trial=e0, e_ref=e0, e_cut=0.2 * (sysd.n / args.tau) ** 0.5, branch_every=1)
    offset = [10]

    def step_ecp():
        offset[0] += S
        return sysd.dmc_step(params, state, S, args.tau, ecp=ecp, pair_capacity=cap, offset=offset[0], **kw)

    def ecp_alone():
        offset[0] += 1
        return sysd.ecp_energy(params, x, ecp, offset=offset[0], pair_capacity=cap)
    state_t, moves = None, [0.0, 0]
    if args.tmoves:
        state_t = sysd.dmc_state(x, ecp=True)
        sysd.dmc_step(params, state_t, 1, args.tau, branch_every=0, state_valid=False, ecp=ecp, pair_capacity=cap, tmoves=True)

    def step_tmove():
        offset[0] += S
        out = sysd.dmc_step(params, state_t, S, args.tau, ecp=ecp, pair_capacity=cap, offset=offset[0], tmoves=True, **kw)
        moves[0] += float(out['ecp_stats'][:, 3].sum())
        moves[1] += S
        return out
    if args.once:                                      # (the run to put under a kernel trace: one call of each kind)
        sysd.dmc_step(params, plain, S, args.tau, **kw)
        ecp_alone()
        step_ecp()
        if args.tmoves:
            step_tmove()
        torch.cuda.synchronize()
        return
    ms_a = timed(lambda: sysd.dmc_step(params, plain, S, args.tau, **kw), args.reps) / S
    ms_b = timed(ecp_alone, args.reps)
    ms_c = timed(step_ecp, args.reps) / S
    pairs = first['pairs'].cpu().numpy()
    extra = {}
    if args.tmoves:
        ms_d = timed(step_tmove, args.reps) / S
        ms_e = timed(lambda: sysd.local_energy(params, x), args.reps)
        extra = {'dmc_step_tmove_ms': round(ms_d, 3), 'ratio_d_over_c': round(ms_d / ms_c, 4), 'excess_ms': round(ms_d - ms_c, 3),
                 'local_energy_ms': round(ms_e, 3), 'tmoves_per_walker_step': moves[0] / (moves[1] * B),
                 'tmove_workspace_bytes': int(sysd.lib.ds_dmc_tmove_workspace_bytes(sysd.handle, ecp.handle, B, cap)),
                 'total_weight_tmove': float(state_t['weight'].sum())}
    print(json.dumps({'case': 'bcc_li', 'electrons': sysd.n, 'B': B, 'steps_per_call': S, 'tau': args.tau, 'n_quad': pot.n_quad,
                      'r_cut_nl': pot.r_cut_nl.tolist(), 'pair_capacity': cap, 'pairs_per_walker': float(pairs[0]) / B,
                      'workspace_bytes': int(sysd.lib.ds_dmc_ecp_workspace_bytes(sysd.handle, ecp.handle, B, cap)),
                      'dmc_step_ms': round(ms_a, 3), 'ecp_energy_ms': round(ms_b, 3), 'dmc_step_ecp_ms': round(ms_c, 3),
                      'ratio_c_over_a_plus_b': round(ms_c / (ms_a + ms_b), 4), 'total_weight': float(state['weight'].sum()), **extra}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--tau', type=float, default=0.01)
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--ecp', nargs='?', const='', default=None)
    ap.add_argument('--r-cut-nl', type=float, default=2.747)
    ap.add_argument('--tmoves', action='store_true')
    ap.add_argument('--forward-walking', nargs='?', const='0,4,16', default=None)
    args = ap.parse_args()
    if args.tmoves and args.ecp is None:
        ap.error('--tmoves needs --ecp')
    cell, klist = systems.build('bcc_li')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    B, S = args.batch, args.steps
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), device='cuda')
    if args.ecp is not None:
        return bench_ecp(args, cell, sysd, params, x)
    state = sysd.dmc_state(x)
    sysd.dmc_step(params, state, 1, args.tau, branch_every=0, state_valid=False)          # initialise once
    e0 = float(state['eloc'][torch.isfinite(state['eloc'])].mean())
    kw = dict(e_trial=e0, e_ref=e0, e_cut=0.2 * (sysd.n / args.tau) ** 0.5)
    step = lambda every: sysd.dmc_step(params, state, S, args.tau, branch_every=every, **kw)
    if args.forward_walking is not None:
        from deepsolid_amd import dmc
        lags = tuple(int(v) for v in args.forward_walking.split(','))
        tracker = dmc.ForwardWalking(cell, lags=lags, density_grid=32, pair_bins=128)
        parents = [None]

        def block():
            parents[0] = sysd.dmc_step(params, state, S, args.tau, branch_every=1, want_parents=True, **kw)['parents']
        block()
        for _ in range(max(lags) + 1):                     # fill the ring: every lag's slot exists from here on
            tracker.update(sysd, state, parents[0])
        if args.once:
            torch.cuda.synchronize()
            return
        ms_step = timed(block, args.reps) / S
        ms_update = timed(lambda: tracker.update(sysd, state, parents[0]), args.reps)
        ring = sum(t.numel() * t.element_size() for t in (tracker.ring_x, tracker.ring_v, tracker.anc))
        print(json.dumps({'case': 'bcc_li', 'electrons': sysd.n, 'B': B, 'steps_per_call': S, 'tau': args.tau, 'lags': list(lags),
                          'dmc_step_ms': round(ms_step, 3), 'fw_update_ms': round(ms_update, 3),
                          'update_over_block': round(ms_update / (ms_step * S), 5), 'ring_bytes': ring,
                          'q_sum': [int(v) for v in tracker.q_sum], 'lost': [tracker.lost(l) for l in lags]}))
        return
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
