#!/usr/bin/env python3
"""Cost of a SPRING step's device calls beside the gradient pass and the KFAC calls on the same cell and batch: device events
around single calls of `ds_logpsi_jacobian`, `ds_minsr_gram`, `ds_minsr_solve`, `ds_minsr_matvec` (both modes), `ds_logpsi_vjp`,
`ds_kfac_factors`, `ds_kfac_inverses` and `ds_kfac_precondition` in ONE process, warm-up + timed calls each, the calls
alternating.  Reports the median / min / max of every call, the footprint of J, and the Gram kernel's FLOP/s (R^2 P: the upper
triangle, a multiply and an add per term) as a fraction of the float64 MFMA peak the project uses (78.6 TFLOP/s).
usage: python tools/spring_bench.py [--system bcc_li] [--batch 1024] [--dtype f64] [--calls 5] [--out FILE.json]  -> one JSON line"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepsolid_amd import network, systems
from deepsolid_amd.device import DeviceSystem

PEAK_F64_MFMA = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--system', default='bcc_li')
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--dtype', default='f64', choices=['f64', 'f32'])
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-kfac', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a timing from anywhere else says nothing'
    dtype = torch.float64 if a.dtype == 'f64' else torch.float32
    cell, klist = systems.build(a.system)
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', dtype=dtype, **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    B, P = a.batch, sysd.param_count
    x = torch.as_tensor(systems.synthetic_walkers(cell, B), device='cuda', dtype=dtype)
    jac = torch.empty(2 * B, P, dtype=dtype, device='cuda')
    J, _, _ = sysd.logpsi_jacobian(params, x, out=jac)
    G = DeviceSystem.minsr_gram(J)
    gen = torch.Generator(device='cuda').manual_seed(1)
    v_r = torch.randn(2 * B, dtype=torch.float64, device='cuda', generator=gen)
    v_p = torch.randn(P, dtype=torch.float64, device='cuda', generator=gen)
    cot = torch.randn(B, 2, dtype=torch.float64, device='cuda', generator=gen).to(dtype)
    lam = 1e-3
    calls = {'ds_logpsi_jacobian': lambda: sysd.logpsi_jacobian(params, x, out=jac),
             'ds_minsr_gram': lambda: DeviceSystem.minsr_gram(J),
             'ds_minsr_solve': lambda: DeviceSystem.minsr_solve(G, v_r, scale=1.0 / B, damping=lam, block=B),
             'ds_minsr_matvec_Jv': lambda: DeviceSystem.minsr_matvec(J, v_p),
             'ds_minsr_matvec_JTv': lambda: DeviceSystem.minsr_matvec(J, v_r, transpose=True),
             'ds_logpsi_vjp': lambda: sysd.logpsi_vjp(params, x, cot)}
    if not a.no_kfac:
        factors, grad = sysd.kfac_factors(params, x, flat=True)
        inv = sysd.kfac_inverses(factors, 1.0, lam)
        vk = grad.index_select(0, sysd.kfac_index(params)['v_src'])
        calls.update({'ds_kfac_factors': lambda: sysd.kfac_factors(params, x, flat=True),
                      'ds_kfac_inverses': lambda: sysd.kfac_inverses(factors, 1.0, lam),
                      'ds_kfac_precondition': lambda: sysd.kfac_precondition(inv, vk)})
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
    out = {'system': a.system, 'dtype': a.dtype, 'batch': B, 'param_count': P, 'rows': 2 * B, 'calls': a.calls, 'warmup': a.warmup,
           'jacobian_bytes': J.numel() * J.element_size(), 'jacobian_gib': J.numel() * J.element_size() / 2.0 ** 30,
           'jacobian_workspace_bytes': int(sysd.lib.ds_jacobian_workspace_bytes(sysd.handle, B))}
    for k, v in ms.items():
        out[k] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)}
    flop = float(2 * B) ** 2 * P
    out['gram_flop'] = flop
    out['gram_tflops'] = flop / (out['ds_minsr_gram']['median_ms'] * 1e-3) / 1e12
    out['gram_fraction_of_f64_mfma_peak'] = out['gram_tflops'] * 1e12 / PEAK_F64_MFMA
    out['jacobian_store_gbps'] = out['jacobian_bytes'] / (out['ds_logpsi_jacobian']['median_ms'] * 1e-3) / 1e9
    out['jacobian_over_vjp'] = out['ds_logpsi_jacobian']['median_ms'] / out['ds_logpsi_vjp']['median_ms']
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
