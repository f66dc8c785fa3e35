#!/usr/bin/env python3
"""Cost of the pseudopotential forces beside the pseudopotential energy and a walker gradient: LiH (4 e-, 2 ions) and bcc-Li (24 e-,
8 ions), float64, B walkers uniform in the cell, the synthetic species of tools/ecp_bench.py with l = 0, 1, 2 channels on every atom,
N_q = 12.  Device events around single calls of `ds_ecp_forces`, `ds_ecp_energy` and `ds_logpsi_grad` in ONE process, 3 warm-up + 10
timed calls each, the calls alternating.

`ds_ecp_forces` runs the forward-Laplacian chain with the gradient output once per quadrature configuration (and once per walker);
`ds_ecp_energy` runs the value chain on the same configurations.  `forces_over_energy` is the measured ratio of the two calls;
`chain_passes_per_walker` = configurations / B + 1, `ms_per_chain_batch` = the force call's time / chain_passes_per_walker is what
one batch of B chain passes costs INSIDE the call, and `overhead_over_logpsi_grad` relates it to `ds_logpsi_grad` on B walkers alone.
usage: python tools/ecp_force_bench.py [--batch 1024] [--calls 10] [--systems lih,bcc_li] [--out FILE.json]   -> one JSON line per system"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepsolid_amd import network, systems
from deepsolid_amd.device import EcpTables
from deepsolid_amd.pseudopotential import SemiLocalECP

SPECIES = dict(local=[(1, 1.2, -1.5), (3, 0.9, 0.7), (2, 1.5, 2.0)],
               channels=[[(2, 1.1, 3.0), (4, 0.8, -0.6)], [(2, 0.9, -1.2)], [(2, 0.7, 0.8)]])
R_CUT_NL = {'lih': 2.18, 'bcc_li': 2.747}         # just below half the smallest height of each cell


def measure(name, a):
    cell, klist = systems.build(name)
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    x = torch.as_tensor(systems.synthetic_walkers(cell, a.batch), device='cuda')
    n_atoms = len(cell.atom_coords())
    r_nl = R_CUT_NL[name]
    ecp = EcpTables(SemiLocalECP(cell, [dict(SPECIES, r_cut_loc=0.8 * r_nl, r_cut_nl=r_nl)], [0] * n_atoms, n_quad=12))
    first = sysd.ecp_energy(params, x, ecp, want_pairs=True)
    pairs, cap = int(first['pairs'].sum()), first['pair_capacity']
    offset = [0]

    def run(fn):
        offset[0] += 1
        return fn(params, x, ecp, seed=7, offset=offset[0], pair_capacity=cap)
    calls = {'ds_ecp_forces': lambda: run(sysd.ecp_forces), 'ds_ecp_energy': lambda: run(sysd.ecp_energy),
             'ds_logpsi_grad': lambda: sysd.logpsi_grad(params, x)}
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
    out = {'system': name, 'dtype': 'f64', 'batch': a.batch, 'calls': a.calls, 'warmup': a.warmup, 'r_cut_nl': r_nl, 'n_quad': 12,
           'pairs_per_walker': pairs / a.batch, 'configurations_per_walker': pairs * 12 / a.batch,
           'workspace_bytes': int(sysd.lib.ds_ecp_forces_workspace_bytes(sysd.handle, ecp.handle, a.batch, cap))}
    for k, v in ms.items():
        out[k] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)}
    passes = out['configurations_per_walker'] + 1
    out['chain_passes_per_walker'] = passes
    out['ms_per_chain_batch'] = out['ds_ecp_forces']['median_ms'] / passes
    out['overhead_over_logpsi_grad'] = out['ms_per_chain_batch'] / out['ds_logpsi_grad']['median_ms']
    out['forces_over_energy'] = out['ds_ecp_forces']['median_ms'] / out['ds_ecp_energy']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--systems', default='lih,bcc_li')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a timing from anywhere else says nothing'
    lines = [json.dumps(measure(name, a)) for name in a.systems.split(',')]
    print('\n'.join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
