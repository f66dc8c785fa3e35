"""A float64 numpy model of the SPRING step and the oracle's per-walker Jacobian, for the tests of
`deepsolid_amd.spring`, `ds_logpsi_jacobian` and `ds_minsr_*`.  Nothing here needs a GPU."""
import numpy as np
import torch


def centre(a, B):
    """H2 a: each half of the leading axis (2B) minus its mean over the B walkers."""
    a = np.asarray(a, dtype=np.float64)
    out = a.copy()
    out[:B] -= a[:B].mean(axis=0, keepdims=True)
    out[B:] -= a[B:].mean(axis=0, keepdims=True)
    return out


def rhs_of(d):
    """e = [Re d ; Im d] / sqrt(B)."""
    d = np.asarray(d, dtype=np.complex128)
    return np.concatenate([d.real, d.imag]) / np.sqrt(len(d))


def spring_direction(J, d, phi, damping, mu):
    """phi' = mu phi + Jbar^T (T + lambda I)^-1 (e - mu Jbar phi), exactly as defined."""
    J = np.asarray(J, dtype=np.float64)
    B = J.shape[0] // 2
    Jb = centre(J, B) / np.sqrt(B)
    T = Jb @ Jb.T
    zeta = np.linalg.solve(T + damping * np.eye(2 * B), rhs_of(d) - mu * (Jb @ phi))
    return mu * phi + Jb.T @ zeta


def spring_step(J, d, state, theta, lr, damping=1e-3, mu=0.99, norm_constraint=1e-3):
    """One step on the packed vectors: -> (state', theta').  state = {'count', 'phi'}; lr a number or a callable of count."""
    phi = np.asarray(state['phi'], dtype=np.float64)
    new = spring_direction(J, d, phi, damping, mu)
    rate = lr(state['count']) if callable(lr) else lr
    scale = min(rate, np.sqrt(norm_constraint) / np.linalg.norm(new))
    return {'count': state['count'] + 1, 'phi': new}, np.asarray(theta, dtype=np.float64) - scale * new


def sr_direction(J, d, damping):
    """The P x P form (Jbar^T Jbar + lambda I)^-1 Jbar^T e: damped stochastic reconfiguration."""
    J = np.asarray(J, dtype=np.float64)
    B = J.shape[0] // 2
    Jb = centre(J, B) / np.sqrt(B)
    return np.linalg.solve(Jb.T @ Jb + damping * np.eye(J.shape[1]), Jb.T @ rhs_of(d))


def tree_flat(tree):
    """Leaves of a parameter tree in the reference's order, concatenated (float64 numpy)."""
    from deepsolid_amd.params import tree_leaves
    return np.concatenate([(t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)).reshape(-1)
                           for t in tree_leaves(tree)])


def oracle_jacobian(case, x, param_map):
    """(2B, param_count) float64: rows from `oracle.train.logpsi_vjp` with one-hot cotangents (1 on log|psi_b| for row b, 1 on
    arg psi_b for row B + b), flattened through `ParamMap.pack`'s gather so that columns are packed columns (padding 0).
    case = (cell, klist, net_kw, params) of `common.load_case`."""
    from common import oracle_net
    from oracle import train as otrain
    cell, klist, net_kw, params = case
    net = oracle_net(cell, klist, net_kw, 'eval_logdet')
    x = torch.as_tensor(np.asarray(x)).detach().cpu().double()
    B = len(x)
    gather = param_map.layout(params).gather
    J = np.zeros((2 * B, param_map.param_count))
    for half, c in enumerate((1.0 + 0.0j, 0.0 + 1.0j)):
        for b in range(B):
            tree = otrain.logpsi_vjp(net.apply, params, x[b:b + 1], torch.tensor([c], dtype=torch.complex128))
            flat = np.append(tree_flat(tree), 0.0)
            J[half * B + b] = flat[np.where(gather < 0, flat.size - 1, gather)]
    return J


def leaf_columns(param_map, params):
    """[(leaf path, packed columns of its entries)] in the reference's leaf order."""
    lay = param_map.layout(params)
    return [(path, lay.pos[idx.reshape(-1)]) for path, idx in lay.idx.items()]
