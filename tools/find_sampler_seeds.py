"""Finds the (seed, width) entries of tests/sampler_helpers.py::CHAINS / SINGLE_MOVES on the CPU, from the oracle alone: the first
seed (and the first width of a short list) at which every Metropolis decision of the test is decidable (its margin ratio - log u
exceeds the tolerance on lp), the test holds an acceptance and a rejection, and a proposed electron crosses a cell face.
Prints one table line per test with the smallest |margin|.  Usage: python tools/find_sampler_seeds.py [chains|single]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sampler_helpers as sh                      # noqa: E402

WIDTHS = {'mh': (0.05, 0.1, 0.2, 0.4), 'one': (0.5, 1.0, 2.0), 'imp': (0.05, 0.1, 0.2, 0.4), 'asym': (0.02, 0.05, 0.1)}


def ok(c):
    return c['undecidable'] == 0 and c['accepted'] >= 1 and c['rejected'] >= 1 and c['crossings'] >= 1


def search(make):
    for seed in range(1, 60):
        for width in make.widths:
            c = make(seed, width)
            if ok(c):
                return seed, width, c
    return None


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'all'
    if what in ('chains', 'all'):
        for (name, kind), (_, _, steps) in sh.CHAINS.items():
            f = lambda s, w: sh.chain_reference(name, kind, s, w, sh.CHAIN_BATCH, steps)['cond3']
            f.widths = WIDTHS[kind]
            print('chain', name, kind, steps, search(f), flush=True)
    if what in ('single', 'all'):
        for (name, f32, kind), (_, _, B, i) in sh.SINGLE_MOVES.items():
            f = lambda s, w: sh.single_move_reference(name, kind, s, w, B, i, f32)['cond3']
            f.widths = WIDTHS[kind]
            print('single', name, 'f32' if f32 else 'f64', kind, B, i, search(f), flush=True)
