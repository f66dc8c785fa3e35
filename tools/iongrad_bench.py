#!/usr/bin/env python3
"""Time `ds_logpsi_ion_vjp` (the ion gradient of log psi, csrc/ds_iongrad.h) beside `ds_logpsi_vjp` (the parameter gradient: the
same forward, seed and one-electron cotangent chain, plus every parameter sum and the pair-stream backward) and `ds_ion_forces`
(the other device call of a `PrimitiveForces.update`), in ONE process with device events around single calls.
Default case: bcc-Li (24 electrons, one primitive atom), B = 4096, float64.
Prints one JSON line: median / min / max ms per call, the ratio ion_vjp / vjp, and the library's own event time of the chunks of
one ion call (`ds_profile_read`, kind ion_vjp).
usage: python tools/iongrad_bench.py [--case NAME] [--batch B] [--dtype f64|f32] [--calls C] [--warmup W] [--once]
`--once`: one `ds_logpsi_ion_vjp` call and no timing -- the run to put under `rocprofv3 --kernel-trace --stats` for k_ion_grad."""
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
    ap.add_argument('--case', default='bcc_li', choices=sorted(systems.SYSTEMS))
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--dtype', default='f64', choices=('f64', 'f32'))
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    dtype = torch.float64 if args.dtype == 'f64' else torch.float32
    cell, klist = systems.build(args.case)
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', dtype=dtype, **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    B = args.batch
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), dtype=dtype, device='cuda')
    cot = torch.as_tensor(np.random.default_rng(5).normal(size=(B, 2)), dtype=dtype, device='cuda')
    if args.once:
        sysd.logpsi_ion_vjp(params, x, cot)
        torch.cuda.synchronize()
        return
    drift = sysd.logpsi_grad(params, x)[1].real.contiguous()
    calls = {'ds_logpsi_ion_vjp': lambda: sysd.logpsi_ion_vjp(params, x, cot),
             'ds_logpsi_vjp': lambda: sysd.logpsi_vjp(params, x, cot),
             'ds_ion_forces': lambda: sysd.ion_forces(x, drift)}
    out = {'case': args.case, 'electrons': sysd.n, 'prim_atoms': sysd.n_atoms_prim, 'batch': B, 'dtype': args.dtype, 'calls': args.calls,
           'warmup': args.warmup}
    for name, fn in calls.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.calls):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1))
        out[name] = {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}
    out['ratio_ion_vjp_over_vjp'] = out['ds_logpsi_ion_vjp']['median_ms'] / out['ds_logpsi_vjp']['median_ms']
    sysd.profile(True, only='ion_vjp')
    sysd.logpsi_ion_vjp(params, x, cot)
    ms, n = sysd.profile_read()['ion_vjp']
    sysd.profile(False)
    out['ion_vjp_chunks'] = n
    out['ion_vjp_chunks_event_ms'] = ms
    res = sysd.logpsi_ion_vjp(params, x, cot)[0]
    out['finite'] = bool(torch.isfinite(res).all())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
