#!/usr/bin/env python3
"""Cost of the pseudopotential energy beside a log-psi forward and a local energy: bcc-Li 24 e-, float64, B = 4096 walkers uniform
in the cell, one synthetic species with l = 0, 1, 2 channels on all 8 atoms, r_cut_nl = 2.747 Bohr, N_q = 12.  Device events
around single calls of `ds_ecp_energy`, `ds_logpsi` and `total_energy` (kinetic + Ewald, `train.make_loss` without a
pseudopotential) in ONE process, 3 warm-up + 10 timed calls each, the calls alternating.

The call's cost is forwards: one of the B walkers and one per displaced configuration.  `forwards_per_walker` = configurations / B
+ 1, `ms_per_forward_batch` = the call's time / forwards_per_walker is what one batch of B forwards costs INSIDE the call, and
`overhead_over_logpsi` relates it to `ds_logpsi` on B walkers alone: what the scan, fill, propose, term and walker kernels, the
read-back and the chunking add on top of the forwards.  `ecp_no_pair_ms` times the same call with a non-local cutoff that holds no
pair: scan, offsets, fill, the read-back and the walker kernel alone, no forward.
usage: python tools/ecp_bench.py [--batch 4096] [--calls 10] [--out FILE.json]   -> one JSON line"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deepsolid_amd import network, systems, train
from deepsolid_amd.device import EcpTables
from deepsolid_amd.pseudopotential import SemiLocalECP

SPECIES = dict(local=[(1, 1.2, -1.5), (3, 0.9, 0.7), (2, 1.5, 2.0)],
               channels=[[(2, 1.1, 3.0), (4, 0.8, -0.6)], [(2, 0.9, -1.2)], [(2, 0.7, 0.8)]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--r-cut-nl', type=float, default=2.747)
    ap.add_argument('--n-quad', type=int, default=12)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a timing from anywhere else says nothing'
    cell, klist = systems.build('bcc_li')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    x = torch.as_tensor(systems.synthetic_walkers(cell, a.batch), device='cuda')
    channels = SPECIES['channels'][:3 if a.n_quad == 12 else 2]
    make = lambda r_nl: EcpTables(SemiLocalECP(cell, [dict(SPECIES, channels=channels, r_cut_loc=0.8 * a.r_cut_nl, r_cut_nl=r_nl)],
                                               [0] * 8, n_quad=a.n_quad))
    ecp, empty = make(a.r_cut_nl), make(1e-6)
    total_energy = train.make_loss(net.apply, None, cell)
    first = sysd.ecp_energy(params, x, ecp, want_pairs=True)
    pairs = int(first['pairs'].sum())
    assert int(sysd.ecp_energy(params, x, empty, want_pairs=True)['pairs'].sum()) == 0
    cap = first['pair_capacity']
    offset = [0]

    def run_ecp(tables):
        offset[0] += 1
        return sysd.ecp_energy(params, x, tables, seed=7, offset=offset[0], pair_capacity=cap)
    calls = {'ds_ecp_energy': lambda: run_ecp(ecp), 'ecp_no_pair': lambda: run_ecp(empty),
             'ds_logpsi': lambda: sysd.logpsi(params, x), 'total_energy': lambda: total_energy(params, x)}
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
    out = {'system': 'bcc_li', 'dtype': 'f64', 'batch': a.batch, 'calls': a.calls, 'warmup': a.warmup, 'r_cut_nl': a.r_cut_nl,
           'n_quad': a.n_quad, 'pairs_per_walker': pairs / a.batch, 'configurations_per_walker': pairs * a.n_quad / a.batch,
           'workspace_bytes': int(sysd.lib.ds_ecp_workspace_bytes(sysd.handle, ecp.handle, a.batch, cap))}
    for k, v in ms.items():
        out[k] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)}
    fw = out['configurations_per_walker'] + 1
    out['forwards_per_walker'] = fw
    out['ms_per_forward_batch'] = out['ds_ecp_energy']['median_ms'] / fw
    out['overhead_over_logpsi'] = out['ms_per_forward_batch'] / out['ds_logpsi']['median_ms']
    out['ecp_over_total_energy'] = out['ds_ecp_energy']['median_ms'] / out['total_energy']['median_ms']
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
