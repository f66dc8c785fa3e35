#!/usr/bin/env python3
"""Cost of the Hartree-Fock target evaluation beside the gradient pass and one Metropolis move of a pretraining iteration:
device events around single calls of `ds_hf_orbitals`, `ds_pretrain_loss_vjp` and a one-move `ds_mcmc_step` in ONE process,
the three alternating, 3 warm-up + 10 timed calls each, float64.
  bcc_li : bcc-Li 2x2x2, 24 e-, B = 4096; one atom with s (3 primitives), s, s, p, p -> 9 AOs, n_k = 8
  diamond: diamond 2x2x2, 96 e-, B = 1024; two atoms with s, s, s, p, p, d -> 28 AOs, n_k = 8
The basis tables and MO coefficients are made up (the cost does not depend on their values).  Next to the times the line
carries what the kernel executes, counted from the shapes: images (padded), exponentials and matrix-pipe flops per electron.
usage: python tools/hf_bench.py [--case bcc_li|diamond|both] [--calls 10] [--only-hf] [--out FILE.json]   -> one JSON line per case
(--only-hf: the orbital kernel alone, in a loop, for a counter or kernel-trace run)"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepsolid_amd import hf, network, supercell, systems

CASES = {
    'bcc_li': dict(system='bcc_li', batch=4096, per_atom=[(0, [2.0, 0.5, 0.15]), (0, [0.9]), (0, [0.25]), (1, [0.6]), (1, [0.2])]),
    'diamond': dict(system='diamond', batch=1024,
                    per_atom=[(0, [2.0, 0.6, 0.2]), (0, [1.0]), (0, [0.3]), (1, [1.2, 0.4]), (1, [0.25]), (2, [0.8])]),
}


def make_orbitals(cell, per_atom, seed=1):
    prim = cell.original_cell
    atoms = np.asarray(prim.atom_coords(), dtype=np.float64).reshape(-1, 3)
    shells = [(at, l, ex, hf.normalize_shell(l, ex, np.ones(len(ex)))) for at in range(atoms.shape[0]) for l, ex in per_atom]
    nao = sum(2 * l + 1 for _, l, _, _ in shells)
    kpts = supercell.get_supercell_kpts(cell)
    rng = np.random.default_rng(seed)
    mo = []
    for ns in cell.nelec:
        base, rem = divmod(int(ns), kpts.shape[0])
        mo.append([rng.normal(size=(nao, base + (i < rem))) + 1j * rng.normal(size=(nao, base + (i < rem))) for i in range(kpts.shape[0])])
    return hf.GaussianOrbitals(prim.lattice_vectors(), atoms, shells, kpts, mo, tuple(cell.nelec))


def run(name, a):
    c = CASES[name]
    cell, _ = systems.build(c['system'])
    go = make_orbitals(cell, c['per_atom'])
    B = a.batch or c['batch']
    x = torch.as_tensor(systems.synthetic_walkers(cell, B), device='cuda')
    xs = x.reshape(B, -1, 3)
    n_img = go.images.shape[0]
    n_pad = (n_img + 63) // 64 * 64
    n_prim = sum(s[2].size for s in go.shells)
    tiles = (go.nao + 15) // 16
    nt = 1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 8
    out = {'case': name, 'dtype': 'f64', 'batch': B, 'electrons': int(sum(cell.nelec)), 'n_k': int(go.kpts.shape[0]), 'nao': go.nao,
           'images': int(n_img), 'images_padded': n_pad, 'exp_per_electron': n_pad * n_prim,
           'mfma_flops_per_electron': 2 * 16 * 16 * nt * n_pad * ((go.kpts.shape[0] + 7) // 8), 'calls': a.calls, 'warmup': a.warmup}
    if a.only_hf:
        for _ in range(a.warmup + a.calls):
            go.eval_orb_mat(xs)
        torch.cuda.synchronize()
        return out
    kw = dict(systems.DETNET_DEFAULTS)
    mats = network.make_solid_fermi_net(klist=go.klist, simulation_cell=cell, method_name='eval_mats', **kw)
    slog = network.make_solid_fermi_net(klist=go.klist, simulation_cell=cell, method_name='eval_slogdet', **kw)
    params = mats.init(0)
    sysd, syss = mats.apply.system, slog.apply.system
    targets = [t for t in go.eval_orb_mat(xs) if t.shape[-1]]
    xm = x.clone()
    lp = torch.empty(B, dtype=torch.float64, device='cuda')
    syss.mcmc_step(params, xm, lp, 1, 0.02, seed=1)                   # leaves lp valid for the timed one-move calls
    calls = {'ds_hf_orbitals': lambda i: go.eval_orb_mat(xs),
             'ds_pretrain_loss_vjp': lambda i: sysd.pretrain_loss_vjp(params, x, targets),
             'ds_mcmc_step': lambda i: syss.mcmc_step(params, xm, lp, 1, 0.02, seed=1, offset=1 + i, lp_valid=True)}
    ms = {k: [] for k in calls}
    for i in range(a.warmup + a.calls):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f(i)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    for k, v in ms.items():
        out[k] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)}
    out['ratio_targets_over_gradient'] = out['ds_hf_orbitals']['median_ms'] / out['ds_pretrain_loss_vjp']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', default='both', choices=['bcc_li', 'diamond', 'both'])
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only-hf', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU: a timing from anywhere else says nothing'
    lines = [json.dumps(run(name, a)) for name in (('bcc_li', 'diamond') if a.case == 'both' else (a.case,))]
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
