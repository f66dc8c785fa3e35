"""The KFAC optimizer step of the reference driver (process.py:209-228,291-318: kfac_ferminet_alpha.Optimizer with
num_burnin_steps = 0, momentum = 0, estimation_mode = 'fisher_exact', norm_constraint = 1e-3, curvature_ema = 0.95,
inverse_update_period = invert_every, l2_reg = 0 and the damping passed every step).

Per step, with the rank-averaged packed energy gradient g and the factors of this step's walkers (`ds_kfac_factors`):
  1. every moving average takes  weight <- ema weight + 1,  array <- ema array + new  (utils.py:265-298); the tagged layers'
     `new` are A and G, the untagged leaves' (envelope pi, sigma: NaiveDiagonal, curvature_blocks.py:111-154) grad_seed^2 / B;
     `new` is averaged over the ranks in ONE all-reduce of the flat factor buffer concatenated with the diagonal entries
  2. when step % invert_every == 0: the damped inverses of utils.py:155-218 (`ds_kfac_inverses`)
  3. P = A^- V G^- / R per tagged block (`ds_kfac_precondition`), P = g / (diag + l2_reg + damping) for the diagonal set
  4. q = <P, g> lr^2,  c = min(1, sqrt(norm_constraint / q)),  delta = -lr c P,  params += delta  (optimizer.py:572-614)
The arithmetic of 2 and 3 is HIP (csrc/ds_kfac.h); 1 and 4 are element-wise torch on device buffers.  Nothing is read back to
the host: c and q are device scalars.  The state is a dict of tensors and python scalars, so `checkpoint.save` takes it as it is.
"""
import numpy as np
import torch

from . import constants
from .params import tree_leaves


def kfac(learning_rate_schedule, damping=1e-3, l2_reg=0.0, norm_constraint=1e-3, cov_ema_decay=0.95, invert_every=1, momentum=0.0,
         adaptive_damping=False, register_only_generic=False):
    """-> (init(params) -> state, step(system, params, state, grad, factors, grad_seed, batch) -> (state, params, delta)).

    `learning_rate_schedule`: callable of the optimizer's own step count, or a number.  state: 'count' (int), 'ema_weight'
    (float: every moving average is updated every step, so they share one weight), 'factors' (flat raw A / G arrays in the layout of
    `DeviceSystem.kfac_layout`), 'diag' (raw array of the untagged leaves), 'inverses' (flat), 'velocities' (tree-flat delta:
    momentum is 0, the reference's checkpoint carries them all the same).  The tensors are allocated by the first `step` (their
    sizes belong to the system, which `init` does not see).
    `step` arguments: grad -- packed gradient, already averaged over the ranks; factors, grad_seed -- what
    `system.kfac_factors(params, x, flat=True)` returned on THIS rank; batch -- walkers of this rank.  params is updated in place
    (which bumps the leaves' version counters: the packed-parameter cache of the system refreshes).  delta is the tree-flat update."""
    if momentum != 0.0:
        raise NotImplementedError('kfac: momentum != 0 is not supported (process.py:216 fixes momentum = 0)')
    if adaptive_damping:
        raise NotImplementedError('kfac: adaptive damping is not supported (it is not available in the reference either)')
    if register_only_generic:
        raise NotImplementedError('kfac: register_only_generic is not supported (every linear layer is a repeated_dense block here)')
    if invert_every < 1:
        raise ValueError('kfac: invert_every must be at least 1')
    if not damping + l2_reg > 0.0:
        raise ValueError('kfac: l2_reg + damping must be positive')

    def init(params):
        del params
        return {'count': 0, 'ema_weight': 0.0}

    def ensure(system, state, index):
        layout = system.kfac_layout()
        for b in layout:
            if b['d_in'] == 1 or b['d_out'] == 1:
                raise NotImplementedError('kfac: a tagged block with d_in == 1 or d_out == 1 is not supported (pi_adjusted_inverse '
                                          'treats it specially, utils.py:179-191)')
        total = layout[-1]['g_offset'] + layout[-1]['d_out'] ** 2
        sizes = {'factors': total, 'inverses': total, 'diag': index['diag_src'].numel(), 'velocities': sum(index['leaf_sizes'])}
        for k, n in sizes.items():
            v = state.get(k)
            if v is None:
                state[k] = torch.zeros(n, dtype=system.dtype, device=system.device)
            else:
                if not isinstance(v, torch.Tensor):
                    v = torch.as_tensor(np.asarray(v))
                v = v.to(device=system.device, dtype=system.dtype).reshape(-1)
                if v.numel() != n:
                    raise ValueError(f'kfac state: {k} holds {v.numel()} entries, this system needs {n}')
                state[k] = v
        state['count'] = int(np.asarray(state.get('count', 0)).reshape(-1)[0])
        state['ema_weight'] = float(np.asarray(state.get('ema_weight', 0.0)).reshape(-1)[0])
        return state

    def step(system, params, state, grad, factors, grad_seed, batch):
        index = system.kfac_index(params)
        state = ensure(system, state, index)
        count = state['count']
        lr = float(learning_rate_schedule(count) if callable(learning_rate_schedule) else learning_rate_schedule)
        lam = float(l2_reg + damping)
        # 1. moving averages; the ranks' `new` in one packed all-reduce
        diag_new = grad_seed.index_select(0, index['diag_src']) ** 2 / float(batch)
        nf = factors.numel()
        new = constants.pmean_if_pmap(torch.cat([factors, diag_new]))
        state['ema_weight'] = w = cov_ema_decay * state['ema_weight'] + 1.0
        state['factors'].mul_(cov_ema_decay).add_(new[:nf])
        state['diag'].mul_(cov_ema_decay).add_(new[nf:])
        # 2. inverses
        if count % invert_every == 0:
            state['inverses'] = system.kfac_inverses(state['factors'], w, lam)
        # 3. precondition
        v = grad.index_select(0, index['v_src'])
        p_v, sq = system.kfac_precondition(state['inverses'], v)
        g_d = grad.index_select(0, index['diag_src'])
        p_d = g_d / (state['diag'] / w + lam)
        # 4. norm constraint and update
        q = (sq.sum() + (p_d.double() * g_d.double()).sum()) * lr ** 2
        c = torch.clamp(torch.sqrt(norm_constraint / q), max=1.0)
        scale = (-lr * c).to(system.dtype)
        delta = torch.zeros_like(state['velocities'])
        delta.index_copy_(0, index['v_tree'], p_v * scale)
        delta.index_copy_(0, index['diag_tree'], p_d * scale)
        off = 0
        for leaf, n in zip(tree_leaves(params), index['leaf_sizes']):
            leaf.add_(delta[off:off + n].view(leaf.shape))        # in place: bumps the tensor version, the packed cache refreshes
            off += n
        state['velocities'] = delta
        state['count'] = count + 1
        return state, params, delta
    return init, step


def make_kfac_training_step(mcmc_step, total_energy, optimizer, check_nan=False):
    """`train.make_training_step` for the KFAC optimizer: `optimizer` is the (init, step) pair of `kfac`, `total_energy` what
    `train.make_loss` returns.  Same seven-tuple, same discard rule: with `check_nan` the all-reduced loss, gradient and
    non-finite count decide BEFORE anything is updated, and a discarded step leaves walkers, parameters and the whole optimizer
    state (moving averages included) untouched.  Order within a step, as in the reference (optimizer.py:368-490): move, energy and
    gradient at the new walkers, gradient all-reduce, factor pass at the same walkers, factor all-reduce, moving averages,
    inverses, precondition, update."""
    opt_step = optimizer[1] if isinstance(optimizer, (tuple, list)) else optimizer
    system = total_energy.system
    packed = total_energy.value_and_grad_packed

    def step(t, data, params, state, key, mcmc_width):
        del t                                                          # the optimizer counts its own steps
        new_data, pmove = mcmc_step(params, data, key, mcmc_width)
        (loss, aux_data), flat = packed(params, new_data)
        flat = constants.pmean_if_pmap(flat)
        finite = not check_nan or bool(torch.isfinite(flat).all() & torch.isfinite(loss))
        if check_nan and finite and aux_data.n_nonfinite is not None:
            finite = float(aux_data.n_nonfinite) == 0.0
        if not finite:
            return data, params, state, None, None, pmove, None
        factors, grad_seed = system.kfac_factors(params, new_data, flat=True)
        search_direction = system.unpack_grad(flat, params)
        state, params, _ = opt_step(system, params, state, flat, factors, grad_seed, new_data.shape[0])
        return new_data, params, state, loss, aux_data, pmove, search_direction
    return step
