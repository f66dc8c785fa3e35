#!/usr/bin/env python3
"""Time `ds_one_body_ratios` (the momentum-distribution call, csrc/ds_onebody.h) beside `ds_logpsi` on the same number of
configurations: a call with M samples per walker runs (M + 1) forwards per walker, so B (M + 1) walkers through `ds_logpsi`
are its cost model.  Cases: bcc-Li (24 electrons) B = 4096, M = 24 and LiH (4 electrons) B = 4096, M = 4, float64, 27 k points.
Prints one JSON line per case.  usage: python tools/momentum_bench.py [--reps R] [--case bcc_li|lih] [--once]
`--once`: one call per case and no timing -- the run to put under `rocprofv3 --kernel-trace --stats` for the share of the
call spent in k_onebody_propose / k_onebody_accumulate / k_onebody_final."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepsolid_amd import estimator, network, systems

CASES = {'bcc_li': (4096, 24), 'lih': (4096, 4)}


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
    ap.add_argument('--case', default=None, choices=sorted(CASES))
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    for name in ([args.case] if args.case else sorted(CASES)):
        B, M = CASES[name]
        cell, klist = systems.build(name)
        net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
        params = net.init(0)
        sysd = net.apply.system
        x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), device='cuda')
        kv = torch.as_tensor(estimator.momentum_kpoints(cell, klist, 1)[0], device='cuda')
        sums = torch.zeros(2, len(kv), 2, dtype=torch.float64, device='cuda')
        call = lambda: sysd.one_body_ratios(params, x, M, kvec=kv, nk_sums=sums, seed=1)
        if args.once:
            call()
            torch.cuda.synchronize()
            continue
        ms_call = timed(call, args.reps)
        xl = torch.as_tensor(systems.synthetic_walkers(cell, B * (M + 1), seed=4321), device='cuda')
        ms_logpsi = timed(lambda: sysd.logpsi(params, xl), args.reps)
        print(json.dumps({'case': name, 'electrons': sysd.n, 'B': B, 'M': M, 'n_k': len(kv), 'configurations': B * (M + 1),
                          'one_body_ratios_ms': round(ms_call, 3), 'logpsi_ms': round(ms_logpsi, 3),
                          'ratio': round(ms_call / ms_logpsi, 4)}))


if __name__ == '__main__':
    main()
