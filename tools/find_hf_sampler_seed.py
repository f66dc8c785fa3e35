"""Finds tests/hf_helpers.py::SAMPLER_SEED on the CPU, from the helper alone: the first noise seed at which every Metropolis
decision of the HF-density sampler test (LiH-like cell, 32 walkers, 2 iterations of 3 moves) is decidable -- for every walker and
every move |lp2 - lp1 - log u| exceeds the margin of the test -- and the run holds an acceptance and a rejection.
Prints the seed, the smallest |margin| and the acceptance count.  Usage: python tools/find_hf_sampler_seed.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import hf_helpers as hh                          # noqa: E402

if __name__ == '__main__':
    s = hh.lih_system()
    sim_a = hh.lih_cell().a
    x0 = hh.sampler_start(s, sim_a)
    for seed in range(1, 200):
        normals, uniforms = hh.sampler_noise(seed, sum(s.nelec))
        _, dec, margin = hh.replay_sampler(s, sim_a, x0, normals, uniforms)
        smallest = float(np.abs(margin).min())
        print(f'seed {seed}: smallest |margin| {smallest:.3e}, accepted {int(dec.sum())} of {dec.size}', flush=True)
        if smallest > hh.SAMPLER_MARGIN and dec.any() and (~dec).any():
            print('SAMPLER_SEED =', seed)
            break
