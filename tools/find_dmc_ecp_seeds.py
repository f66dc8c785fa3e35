#!/usr/bin/env python
"""Oracle only, on the CPU (like find_dmc_seeds.py): run the numpy model of DMC with a pseudopotential (tests/dmc_ecp_helpers.py) on
the replay fixture of tests/test_gpu_dmc_ecp.py for a range of seeds and print what each seed gives -- the margins of
find_dmc_seeds.py, the smallest distance of a pair from a cutoff over all visited positions, the smallest distance of an energy
from a clip edge in units of its tolerance, and whether it meets the conditions the tests assert.

    python tools/find_dmc_ecp_seeds.py [--case lih_twist] [--seeds 1 2 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import dmc_ecp_helpers as deh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, nargs='*', default=[1, 2, 3])
    ap.add_argument('--case', default=deh.NAME, choices=sorted(deh.REPLAYS), help='the replay of dmc_ecp_helpers.REPLAYS')
    a = ap.parse_args()
    for seed in a.seeds:
        t0 = time.time()
        c = deh.replay_reference(a.case, seed)['cond']
        try:
            deh.assert_conditions(c)
            ok = 'meets the conditions'
        except AssertionError:
            ok = 'FAILS the conditions'
        print(f'seed {seed}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}' for k, v in c.items()) +
              f'  -- {ok}  ({time.time() - t0:.1f} s)', flush=True)


if __name__ == '__main__':
    main()
