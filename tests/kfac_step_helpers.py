"""Shared by test_kfac_step_cpu.py and test_gpu_kfac_step.py: a torch-float64 CPU restatement of the KFAC step the reference's
driver runs (process.py:209-228: num_burnin_steps = 0, momentum = 0, norm_constraint = 1e-3, curvature_ema = 0.95, l2_reg = 0,
damping passed every step), written from the formulas of utils.py:130-218,265-298, curvature_blocks.py:111-281 and
optimizer.py:572-614.  `pi_adjusted_inverse` is held to reference-executed numbers (tests/golden/kfac_inverse.npz); the rest of the
step is pinned by this restatement only."""
import math

import numpy as np
import torch


def leaves(tree):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from leaves(tree[k])
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            yield from leaves(v)
    else:
        yield tree


def pi_adjusted_inverse(A, G, damping):
    """utils.py:155-218 for factors with more than one entry each: `damping` is lambda = (l2_reg + damping) / repeats."""
    A, G = torch.as_tensor(A, dtype=torch.float64), torch.as_tensor(G, dtype=torch.float64)
    d_in, d_out = A.shape[0], G.shape[0]
    n0, n1 = torch.trace(A), torch.trace(G)
    s = n0 * n1
    if not bool(s > 0):
        r = 1.0 / math.sqrt(damping)
        return torch.eye(d_in, dtype=torch.float64) * r, torch.eye(d_out, dtype=torch.float64) * r
    d0 = torch.sqrt(damping * d_out / (s * d_in))
    d1 = torch.sqrt(damping * d_in / (s * d_out))
    eye0, eye1 = torch.eye(d_in, dtype=torch.float64), torch.eye(d_out, dtype=torch.float64)
    a_inv = torch.linalg.solve(A / n0 + d0 * eye0, eye0) / torch.sqrt(s)
    g_inv = torch.linalg.solve(G / n1 + d1 * eye1, eye1) / torch.sqrt(s)
    return a_inv, g_inv


def damped(A, G, damping):
    """The two matrices `pi_adjusted_inverse` inverts (None on the zero branch): for conditioning checks."""
    A, G = torch.as_tensor(A, dtype=torch.float64), torch.as_tensor(G, dtype=torch.float64)
    n0, n1 = torch.trace(A), torch.trace(G)
    s = n0 * n1
    if not bool(s > 0):
        return None
    d_in, d_out = A.shape[0], G.shape[0]
    return (A / n0 + torch.sqrt(damping * d_out / (s * d_in)) * torch.eye(d_in, dtype=torch.float64),
            G / n1 + torch.sqrt(damping * d_in / (s * d_out)) * torch.eye(d_out, dtype=torch.float64))


def precondition(a_inv, g_inv, v, repeats, dtype=torch.float64):
    """curvature_blocks.py:233-281: P = A^- V G^- / R; -> (P, <P, V> accumulated in float64)."""
    a_inv, g_inv, v = (torch.as_tensor(t).to(dtype) for t in (a_inv, g_inv, v))
    p = (a_inv @ v) @ g_inv / repeats
    return p, float((p.double() * v.double()).sum())


def block_matrix(tree, kind, index):
    """V = [w.reshape(-1, d_out) ; b] of one tagged layer, reference row order."""
    p = tree[kind][index]
    w = torch.as_tensor(np.asarray(p['w'].detach().cpu() if isinstance(p['w'], torch.Tensor) else p['w']), dtype=torch.float64)
    rows = [w.reshape(-1, w.shape[-1])]
    if 'b' in p:
        b = torch.as_tensor(np.asarray(p['b'].detach().cpu() if isinstance(p['b'], torch.Tensor) else p['b']), dtype=torch.float64)
        rows.append(b.reshape(1, -1))
    return torch.cat(rows)


def init_state(shapes, params_tree):
    """shapes: [(kind, index, has_bias, d_in, d_out, repeats)] (kfac_helpers.block_shapes)."""
    return {'count': 0, 'ema_weight': 0.0,
            'factors': [(torch.zeros(s[3], s[3], dtype=torch.float64), torch.zeros(s[4], s[4], dtype=torch.float64)) for s in shapes],
            'diag': [{k: torch.zeros(tuple(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v).shape), dtype=torch.float64)
                      for k, v in e.items()} for e in params_tree['envelope']],
            'inverses': None}


def kfac_step(state, shapes, params_tree, grad_tree, factors, grad_seed_tree, B, lr, damping=1e-3, l2_reg=0.0, norm_constraint=1e-3,
              ema=0.95, invert_every=1):
    """One step on one rank.  factors: [(A, G)] of this step; grad_tree / grad_seed_tree: trees shaped like the parameters.
    -> (state, delta tree with the tagged layers and the envelope; every leaf float64)."""
    cpu = lambda t: torch.as_tensor(np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t), dtype=torch.float64)
    state['ema_weight'] = w = ema * state['ema_weight'] + 1.0
    state['factors'] = [(ema * a + cpu(na), ema * g + cpu(ng)) for (a, g), (na, ng) in zip(state['factors'], factors)]
    state['diag'] = [{k: ema * d[k] + cpu(gs[k]) ** 2 / B for k in d} for d, gs in zip(state['diag'], grad_seed_tree['envelope'])]
    lam = l2_reg + damping
    if state['count'] % invert_every == 0:
        state['inverses'] = [pi_adjusted_inverse(a / w, g / w, lam / s[5]) for (a, g), s in zip(state['factors'], shapes)]
    pre, q = [], 0.0
    for (a_inv, g_inv), s in zip(state['inverses'], shapes):
        p, dot = precondition(a_inv, g_inv, block_matrix(grad_tree, s[0], s[1]), s[5])
        pre.append(p)
        q += dot
    pdiag = []
    for d, g in zip(state['diag'], grad_tree['envelope']):
        e = {k: cpu(g[k]) / (d[k] / w + lam) for k in d}
        q += sum(float((e[k] * cpu(g[k])).sum()) for k in d)
        pdiag.append(e)
    q *= lr ** 2
    c = min(1.0, math.sqrt(norm_constraint / q)) if q > 0 else 1.0
    delta = {'single': {}, 'double': {}, 'orbital': {}, 'envelope': [{k: -lr * c * v for k, v in e.items()} for e in pdiag]}
    for p, s in zip(pre, shapes):
        delta[s[0]][s[1]] = -lr * c * p
    state['count'] += 1
    state['c'], state['q'] = c, q
    return state, delta
