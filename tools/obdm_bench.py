#!/usr/bin/env python3
"""Time `ds_obdm_accumulate` (the one-body density-matrix fold, csrc/ds_obdm.h) beside the `ds_one_body_ratios` call of the same
`estimator.OneBodyDensityMatrix.update`: the ratio call runs M + 1 network forwards per walker, the fold 2 basis evaluations per
sample and 8 Mb^2 flop per sample and spin matrix.  Case: bcc-Li (24 electrons), B = 4096, M = 24, float64, a made-up s / p basis
(two s and two p shells on the one atom of the primitive cell: 8 AOs) with 32 random orbitals per spin, four on each of the eight
k points of the cell.  Prints one JSON line.  usage: python tools/obdm_bench.py [--reps R] [--batch B] [--once]
`--once`: one update and no timing -- the run to put under `rocprofv3 --kernel-trace --stats` for the share of the fold spent in
k_obdm_basis / k_obdm_accumulate / k_obdm_final."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deepsolid_amd import hf, network, systems
from deepsolid_amd.supercell import get_supercell_kpts


def made_up_basis(cell, bands=4, seed=7):
    prim = cell.original_cell
    shell = lambda l, exps: (0, l, np.asarray(exps, dtype=np.float64), hf.normalize_shell(l, exps, np.ones(len(exps))))
    shells = [shell(0, [1.1, 0.3]), shell(0, [0.12]), shell(1, [0.6]), shell(1, [0.15])]
    kpts = get_supercell_kpts(cell)
    rng = np.random.default_rng(seed)
    mo = [[rng.normal(size=(8, bands)) + 1j * rng.normal(size=(8, bands)) for _ in kpts] for _ in range(2)]
    n = bands * len(kpts)
    return hf.GaussianOrbitals(prim.lattice_vectors(), prim.atom_coords(), shells, kpts, mo, (n, n))


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
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    B, M = args.batch, 24
    cell, klist = systems.build('bcc_li')
    net = network.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **systems.DETNET_DEFAULTS)
    params = net.init(0)
    sysd = net.apply.system
    basis = made_up_basis(cell)
    x = torch.as_tensor(systems.synthetic_walkers(cell, B, seed=1234), device='cuda')
    tab = basis._device_tables(x.device)
    nelec = (int(cell.nelec[0]), int(cell.nelec[1]))
    mb = max(basis.nelec)
    dm = torch.zeros(2, mb, mb, 2, dtype=torch.float64, device='cuda')
    ov = torch.zeros_like(dm)
    ratios = lambda: sysd.one_body_ratios(params, x, M, seed=1, want_ratios=True, want_shifts=True)
    out = ratios()
    fold = lambda: tab.obdm_accumulate(x, nelec, M, 0, out['ratios'], out['shifts'], dm_sums=dm, ov_sums=ov)
    if args.once:
        fold()
        torch.cuda.synchronize()
        return
    ms_ratio = timed(ratios, args.reps)
    ms_fold = timed(fold, args.reps)
    print(json.dumps({'case': 'bcc_li', 'electrons': sysd.n, 'B': B, 'M': M, 'basis_per_spin': mb, 'n_k': len(basis.kpts),
                      'images': int(basis.images.shape[0]), 'samples': B * M, 'one_body_ratios_ms': round(ms_ratio, 3),
                      'obdm_accumulate_ms': round(ms_fold, 3), 'ratio': round(ms_fold / ms_ratio, 4),
                      'workspace_mib': round(int(tab.lib.ds_obdm_workspace_bytes(tab.handle, B, M)) / 2 ** 20, 1)}))


if __name__ == '__main__':
    main()
