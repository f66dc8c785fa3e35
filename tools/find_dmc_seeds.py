#!/usr/bin/env python
"""Oracle only, on the CPU (like find_sampler_seeds.py): run the numpy DMC model of tests/dmc_helpers.py on the replay fixtures of
tests/test_gpu_dmc.py for a range of seeds and print the margins each seed gives -- the smallest |A - log u|, the smallest distance
from a tooth to a cumulative edge over W, and how often every kind of event happened.  The seeds and margins listed in
tests/dmc_helpers.py come from this output.

    python tools/find_dmc_seeds.py [--seeds 1 2 3] [--case lih24]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import dmc_helpers as dh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, nargs='*', default=[1, 2, 3])
    ap.add_argument('--case', nargs='*', default=list(dh.REPLAYS))
    ap.add_argument('--node', action='store_true', help='also search the node_mode = 1 fixture')
    a = ap.parse_args()
    for key in a.case:
        name, B, tau, steps, _, wk = dh.REPLAYS[key]
        for seed in a.seeds:
            t0 = time.time()
            dh.REPLAYS[key] = (name, B, tau, steps, seed, wk)
            dh.replay_reference.cache_clear()
            c = dh.replay_reference(key)['cond']
            print(f'{key} seed {seed}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}' for k, v in c.items()) +
                  f'  ({time.time() - t0:.1f} s)', flush=True)
    if a.node:
        for seed in a.seeds:
            r = dh.node_reference(seed)
            print(f'node seed {seed}: {r["cond"]}', flush=True)


if __name__ == '__main__':
    main()
