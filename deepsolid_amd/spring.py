"""The SPRING optimizer (Goldshlager, Abrahamsen, Lin, J. Comput. Phys. 2024) on the per-walker Jacobian; with mu = 0 it is
stochastic reconfiguration in its sample-space form (MinSR).

With log psi_b = u_b + i phi_b, B walkers and P packed parameters:
  J  (2B, P)   row b = d u_b / d theta, row B + b = d phi_b / d theta            (`DeviceSystem.logpsi_jacobian`)
  H2           centres each half over its B walkers;  Jbar = H2 J / sqrt(B)
  e            [Re d ; Im d] / sqrt(B),  d = clip(E_L - loss), the cotangent numerator of `train.make_loss`
  T     = Jbar Jbar^T = H2 (J J^T) H2 / B                                        (`minsr_gram`)
  zeta  = (T + lambda I)^-1 (e - mu Jbar phi)                                    (`minsr_matvec`, `minsr_solve`)
  phi'  = mu phi + Jbar^T zeta                                                   (`minsr_matvec`)
  theta <- theta - min(lr, sqrt(C) / |phi'|) phi';  phi <- phi' (unscaled);  count <- count + 1
The Gram matrix, the two matrix-vector products and the solve are HIP (csrc/ds_minsr.h); the centring of the length-2B vectors,
the norm and the update are element-wise torch on device buffers.  The defaults lambda = 1e-3, mu = 0.99, C = 1e-3 are the paper's
values as recalled; no fixture pins them.  The state is `{'count': int, 'phi': packed float64 device tensor}` (phi appears with
the first step: its size belongs to the system, which `init` does not see), so `checkpoint.save` takes it as it is.
"""
import math

import numpy as np
import torch

from . import constants
from .device import DeviceSystem
from .params import tree_leaves


def _centre(v, B):
    """H2 v for a (2B,) vector: each half minus its mean."""
    h = v.view(2, B)
    return (h - h.mean(dim=1, keepdim=True)).reshape(-1)


def spring(learning_rate, damping=1e-3, mu=0.99, norm_constraint=1e-3):
    """-> (init(params) -> state, step(system, params, state, jac, d, check_nan=False) -> (state, params, phi') or None).

    `learning_rate`: callable of the optimizer's own step count, or a number.  `step` arguments: jac -- what
    `system.logpsi_jacobian(params, x)` returned at this step's walkers; d -- clip(E_L - loss), complex (B,).  params is updated
    in place through `unpack_grad` of the packed direction.  With `check_nan` a direction that is not finite leaves parameters and
    state untouched and the step returns None (one device -> host read)."""
    if not damping > 0.0:
        raise ValueError('spring: damping must be positive')
    if not 0.0 <= mu < 1.0:
        raise ValueError('spring: mu must lie in [0, 1)')
    if not norm_constraint > 0.0:
        raise ValueError('spring: norm_constraint must be positive')

    def init(params):
        del params
        return {'count': 0}

    def ensure(system, state):
        n = system.param_count
        v = state.get('phi')
        if v is None:
            v = torch.zeros(n, dtype=torch.float64, device=system.device)
        else:
            if not isinstance(v, torch.Tensor):
                v = torch.as_tensor(np.asarray(v))
            v = v.to(device=system.device, dtype=torch.float64).reshape(-1)
            if v.numel() != n:
                raise ValueError(f'spring state: phi holds {v.numel()} entries, this system needs {n}')
        return int(np.asarray(state.get('count', 0)).reshape(-1)[0]), v

    def step(system, params, state, jac, d, check_nan=False):
        count, phi = ensure(system, state)
        B = jac.shape[0] // 2
        lr = float(learning_rate(count) if callable(learning_rate) else learning_rate)
        rb = 1.0 / math.sqrt(B)
        d = d.to(torch.complex128)
        rhs = torch.cat([d.real, d.imag]) * rb
        if mu != 0.0:
            rhs = rhs - (mu * rb) * _centre(DeviceSystem.minsr_matvec(jac, phi), B)
        gram = DeviceSystem.minsr_gram(jac)
        zeta = DeviceSystem.minsr_solve(gram, rhs, scale=1.0 / B, damping=damping, block=B)
        new = DeviceSystem.minsr_matvec(jac, _centre(zeta, B) * rb, transpose=True)
        if mu != 0.0:
            new = new + mu * phi
        if check_nan and not bool(torch.isfinite(new).all()):
            return None
        scale = torch.clamp(math.sqrt(norm_constraint) / torch.linalg.vector_norm(new), max=lr)
        delta = system.unpack_grad((new * scale).to(system.dtype), params)
        for leaf, dl in zip(tree_leaves(params), tree_leaves(delta)):
            leaf.sub_(dl)                                  # in place: bumps the tensor version, the packed cache refreshes
        state['phi'] = new
        state['count'] = count + 1
        return state, params, new
    return init, step


def make_spring_training_step(mcmc_step, total_energy, opt, check_nan=False):
    """`train.make_training_step` for SPRING: `opt` is the (init, step) pair of `spring`, `total_energy` what `train.make_loss`
    returns.  Same seven-tuple, same discard rule: with `check_nan` the loss and the non-finite count decide BEFORE the Jacobian
    pass (one host read), the direction phi' is checked before the in-place update (a second one), and a discarded step leaves
    walkers, parameters and optimizer state untouched.  Order within a step: move, energy and clip(E_L - loss) at the new walkers,
    Jacobian pass at the same walkers, Gram matrix, solve, update.  The seventh entry is phi' as a parameter tree.
    One rank only: T = Jbar Jbar^T needs every rank's rows of J, which are never gathered."""
    opt_step = opt[1] if isinstance(opt, (tuple, list)) else opt
    system = total_energy.system
    value_and_clip_diff = total_energy.value_and_clip_diff

    def step(t, data, params, state, key, mcmc_width):
        del t                                                          # the optimizer counts its own steps
        if constants.world_size() > 1:
            raise NotImplementedError('spring runs on one rank only: T = Jbar Jbar^T needs the Jacobian rows of every rank, '
                                      'and the ranks\' rows are not gathered')
        new_data, pmove = mcmc_step(params, data, key, mcmc_width)
        (loss, aux_data), d = value_and_clip_diff(params, new_data)
        if check_nan:
            bad = ~torch.isfinite(loss)
            if aux_data.n_nonfinite is not None:
                bad = bad | (aux_data.n_nonfinite != 0)
            if bool(bad):
                return data, params, state, None, None, pmove, None
        jac, _, _ = system.logpsi_jacobian(params, new_data)
        out = opt_step(system, params, state, jac, d, check_nan=check_nan)
        if out is None:
            return data, params, state, None, None, pmove, None
        state, params, direction = out
        return new_data, params, state, loss, aux_data, pmove, system.unpack_grad(direction.to(system.dtype), params)
    return step
