#!/usr/bin/env python
"""Oracle only, on the CPU (like find_dmc_ecp_seeds.py): run the numpy model of DMC with T-moves (tests/dmc_tmove_helpers.py) on the
replay fixture of tests/test_gpu_dmc_tmove.py for a range of seeds and print what each seed gives -- the margins of
find_dmc_ecp_seeds.py, the number of T-moves, the smallest distance of a T-move decision from an interval edge in units of the
a-priori bound on r_c (tau tol_q() sum |W / N_q| max(1, |q|)), the rejected walkers that were evaluated in place, the walkers that
died -- and whether it meets the conditions the tests assert: every Metropolis decision further than TOL_A from its threshold,
every T-move decision further than 10 bounds from an edge.

    python tools/find_dmc_tmove_seeds.py [--case lih_twist] [--seeds 1 2 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import dmc_tmove_helpers as th  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seeds', type=int, nargs='*', default=[1, 2, 3])
    ap.add_argument('--case', default=th.NAME, choices=sorted(th.REPLAYS), help='the replay of dmc_tmove_helpers.REPLAYS')
    a = ap.parse_args()
    for seed in a.seeds:
        t0 = time.time()
        r = th.replay_reference(a.case, seed)
        c = r['cond']
        try:
            th.assert_conditions(c, died=a.case == th.NAME)
            ok = 'meets the conditions'
        except AssertionError:
            ok = 'FAILS the conditions'
        print(f'seed {seed}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}' for k, v in c.items()) +
              f'  -- {ok}  ({time.time() - t0:.1f} s)', flush=True)
        for i, s in enumerate(r['steps']):
            print(f'    step {i}: T-moves {[(int(k), int(c_)) for k, c_ in enumerate(s["choice"]) if c_ >= 0]}', flush=True)


if __name__ == '__main__':
    main()
