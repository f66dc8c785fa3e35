#!/usr/bin/env python3
"""Time `ds_spin_exchange_ratios` (the <S^2> call, csrc/ds_spin.h) beside `ds_logpsi` on the same number of configurations: a call
with M pairs per walker runs (M + 1) forwards per walker, so B (M + 1) walkers through `ds_logpsi` are its cost model.  Case:
bcc-Li (24 electrons, P = 144 pairs), B = 4096, float64, for M = P = 144 (every pair) and for M = 12.
Prints one JSON line per M: ms per call, ms of the (M + 1) B forwards, their ratio, and `outside_value_chain` = 1 - forwards / call,
the share of the call that is not accounted for by the forwards alone (the kernels of ds_spin.h, the extra pass of the B walkers
themselves, chunk tails).  usage: python tools/s2_bench.py [--reps R] [--pairs M] [--batch B] [--once]
`--once`: one call per M and no timing -- the run to put under `rocprofv3 --kernel-trace --stats` for the share of the call
spent in k_spin_propose / k_spin_ratio / k_spin_walker / k_spin_final."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepsolid_amd import network, systems

PAIRS = (144, 12)


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
    ap.add_argument('--pairs', type=int, default=None)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    cell, klist = systems.build('bcc_li')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    B = args.batch
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), device='cuda')
    for M in ([args.pairs] if args.pairs else PAIRS):
        sums = torch.zeros(4, dtype=torch.float64, device='cuda')
        call = lambda: sysd.spin_exchange_ratios(params, x, M, sums=sums)
        if args.once:
            call()
            torch.cuda.synchronize()
            continue
        ms_call = timed(call, args.reps)
        xl = torch.as_tensor(systems.synthetic_walkers(cell, B * (M + 1), seed=4321), device='cuda')
        ms_logpsi = timed(lambda: sysd.logpsi(params, xl), args.reps)
        del xl
        s = sums.cpu().numpy()
        print(json.dumps({'case': 'bcc_li', 'electrons': sysd.n, 'pairs': sysd.nelec[0] * sysd.nelec[1], 'B': B, 'M': M,
                          'configurations': B * (M + 1), 'spin_exchange_ratios_ms': round(ms_call, 3),
                          'logpsi_ms': round(ms_logpsi, 3), 'ratio': round(ms_call / ms_logpsi, 4),
                          'outside_value_chain': round(1.0 - ms_logpsi / ms_call, 4),
                          'good_walkers_per_call': s[3] / (args.reps + 1)}))


if __name__ == '__main__':
    main()
