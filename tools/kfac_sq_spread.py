#!/usr/bin/env python3
"""How far does the float32 loss of the KFAC preconditioner depend on the order of summation?  CPU only.
For every block of a case: P = A^- V G^- / R and <P, V> in float32 (the restatement of tests/kfac_step_helpers.py, as
test_precondition_vs_restatement runs it for its budget), the same two products with both contraction axes permuted (12 other
summation orders of the same float32 arithmetic), and with one sequential float32 accumulator per entry, each against the float64
products of the same float32 inputs.  The inverses are the restatement's own, at 3 synthetic walkers (seed 91), damping 1e-3.
    python tools/kfac_sq_spread.py diamond"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np
import torch
import kfac_helpers as kh
import kfac_step_helpers as ks
from common import load_case
from deepsolid_amd import systems

name = sys.argv[1]
fx, cell, klist, net_kw, params = load_case(name)
x = systems.synthetic_walkers(cell, 3, seed=91).astype(np.float32).astype(np.float64)
factors = kh.reference_factors(cell, klist, net_kw, params, x)[0]
shapes = kh.block_shapes(params, cell.nelec)
v = torch.as_tensor(np.random.default_rng(3).normal(size=sum(s[3] * s[4] for s in shapes))).float()
rng = np.random.default_rng(0)
off = 0
for s, (A, G) in zip(shapes, factors):
    d_in, d_out, rep = s[3], s[4], s[5]
    vb = v[off:off + d_in * d_out].view(d_in, d_out)
    off += d_in * d_out
    Ai, Gi = (t.float() for t in ks.pi_adjusted_inverse(A.float().double(), G.float().double(), 1e-3 / rep))
    ref, dot = ks.precondition(Ai, Gi, vb, rep)

    def losses(p):
        return float((p.double() - ref).abs().max() / ref.abs().max()), abs(float((p.double() * vb.double()).sum()) - dot) / abs(dot)
    plain = losses(ks.precondition(Ai, Gi, vb, rep, dtype=torch.float32)[0])
    perm = []
    for trial in range(12):
        p0, p1 = torch.as_tensor(rng.permutation(d_in)), torch.as_tensor(rng.permutation(d_out))
        t = Ai[:, p0].contiguous() @ vb[p0, :].contiguous()
        perm.append(losses((t[:, p1].contiguous() @ Gi[p1, :].contiguous()) / rep))
    t = torch.zeros(d_in, d_out)
    for k in range(d_in):
        t += Ai[:, k:k + 1] * vb[k:k + 1, :]
    p = torch.zeros(d_in, d_out)
    for k in range(d_out):
        p += t[:, k:k + 1] * Gi[k:k + 1, :]
    seq = losses(p / rep)
    sq = np.array([q[1] for q in perm])
    out = np.array([q[0] for q in perm])
    print(f'{s[0]}[{s[1]}] {d_in} x {d_out}: <P, V> loss {plain[1]:.2e}; permuted {sq.min():.2e} .. {sq.max():.2e} (median {np.median(sq):.2e}); '
          f'sequential {seq[1]:.2e} | out loss {plain[0]:.2e}; permuted {out.min():.2e} .. {out.max():.2e}; sequential {seq[0]:.2e}', flush=True)
