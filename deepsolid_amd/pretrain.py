"""Orbital-matching pretraining (reference DeepSolid/pretrain.py:43-169, `pretrain.method = 'net'`).

Before the first energy step the reference fits the network's orbital matrices to target orbitals (Hartree-Fock there) by
Adam on a mean-square loss, moving the walkers with one Metropolis step per iteration (process.py:148-177).  Here

    loss, d loss / d params   is ONE call of the HIP library (`ds_pretrain_loss_vjp`: the value chain up to the orbital head,
                              the residual seed of csrc/ds_grad.h and the reverse sweep the energy gradient uses),
    the move                  is the fused `ds_mcmc_step` with one step,
    loss and gradient         cross the ranks in one packed all-reduce.

The targets enter as plain arrays, the way `klist` enters the network: `scf_approx` is any object with
``eval_orb_mat(x (B, N, 3) float64) -> [up (B, n_up, n_up), dn (B, n_dn, n_dn)]`` ([walker, electron, orbital], complex) --
the one method of the reference's `hf.SCF` the loop uses (hf.py:136-153); it is handed a numpy array on the host, as the reference
hands it one, unless the object has a true attribute `on_device`.  `PlaneWaveOrbitals` is a PySCF-free free-electron provider;
`deepsolid_amd.hf.GaussianOrbitals` evaluates real Hartree-Fock crystalline orbitals on the device from dumped arrays.
`pretrain_hartree_fock_usingHF` (`method = 'hf'`, pretrain.py:172-302) moves the walkers on the HF density instead of the
network's; it needs `eval_slogdet` of the provider as well.
"""
import functools
import logging

import numpy as np
import torch

from . import constants
from .network import NetworkApply


class PlaneWaveOrbitals:
    """Free-electron target: orbital m of spin s is the plane wave exp(i k_m . r) of the `klist` the network was built with
    (supercell.make_klist), so the target determinant is the one the network's phase factors alone would give.
    A fitting target, not a sampling density: a k vector repeated within a spin makes the target matrix singular, which the
    loss does not mind."""

    on_device = True        # pretrain_hartree_fock hands it the walkers where they are (no host round trip)

    def __init__(self, klist):
        self.klist = [np.asarray(k, dtype=np.float64).reshape(-1, 3) for k in klist]
        self.nelec = tuple(k.shape[0] for k in self.klist)

    def eval_orb_mat(self, x):
        """x (B, N, 3) -> [up (B, n_up, n_up), dn (B, n_dn, n_dn)] complex128, [walker, electron, orbital]; evaluated where
        `x` lives (a device tensor stays on the device; a numpy array gives tensors on the host)."""
        x = torch.as_tensor(x).to(torch.float64)
        if x.dim() != 3 or x.shape[1] != sum(self.nelec) or x.shape[2] != 3:
            raise ValueError(f'walkers must be (B, {sum(self.nelec)}, 3), got {tuple(x.shape)}')
        out, i0 = [], 0
        for k in self.klist:
            kt = torch.as_tensor(k, device=x.device)
            phase = torch.einsum('bic,mc->bim', x[:, i0:i0 + k.shape[0]], kt)
            out.append(torch.polar(torch.ones_like(phase), phase))
            i0 += k.shape[0]
        return out


def block_diagonal_target(target_up, target_dn):
    """The dense target of `full_det` (pretrain.py:79-86): blockdiag(up, dn) with zero off-diagonal blocks.  The library
    implies these zeros inside its kernel; this host version is what tests and other consumers compare with."""
    B, na, nb = target_up.shape[0], target_up.shape[1], target_dn.shape[1]
    z = lambda r, c: torch.zeros(B, r, c, dtype=target_up.dtype, device=target_up.device)
    return torch.cat([torch.cat([target_up, z(na, nb)], dim=-1), torch.cat([z(nb, na), target_dn], dim=-1)], dim=-2)


def _philox_seed(key):
    """Philox key of one move: an int is a pure key (the rank is folded in), a torch.Generator is stateful (the key is drawn on
    the host) -- the rule of qmc.make_mcmc_step.  An int is a key PER CALL, like a JAX PRNGKey: a caller who drives
    `pretrain_step` itself passes a new one every iteration (or a generator), else every move draws the same noise."""
    if isinstance(key, torch.Generator):
        from .qmc import _host_generator
        g = key if key.device.type == 'cpu' else _host_generator(key)
        r = torch.randint(0, 2 ** 31 - 1, (2,), generator=g).tolist()
        return (r[0] << 31) | r[1]
    return int(key) * max(1, constants.world_size()) + constants.rank()


def make_pretrain_step(batch_orbitals, batch_network, latvec, optimizer, full_det=False, mcmc_width=0.02):
    """pretrain.py:43-107.  `batch_orbitals` / `batch_network`: the `.apply` of ``make_solid_fermi_net`` with
    ``method_name='eval_mats'`` / ``'eval_slogdet'`` (batched natively); `optimizer`: the ``(init, update)`` pair of
    `train.adam`; `full_det` must be the network's own setting (the reference passes cfg.network.detnet.full_det to both).
    `mcmc_width`: the move width (the default of the reference's `mh_update`, which pretraining never overrides).
    -> ``pretrain_step(data, target, params, state, key)`` -> (data, params, state, loss_val, logprob, num_accepts);
    `target`: the reference's list, one (B, n_s, n_s) complex matrix per spin with electrons; `params` is updated in place."""
    for f, m in ((batch_orbitals, 'eval_mats'), (batch_network, 'eval_slogdet')):
        if not isinstance(f, NetworkApply) or f.method_name != m:
            raise TypeError(f"expected the .apply of make_solid_fermi_net(method_name='{m}')")
    if bool(batch_orbitals.net_kw.get('full_det', False)) != bool(full_det):
        raise ValueError('full_det differs from the setting the network was built with')
    _, opt_update = optimizer

    def pretrain_step(data, target, params, state, key):
        system = batch_orbitals.system
        from .qmc import _check_latvec
        _check_latvec(latvec, system)
        loss, flat = system.pretrain_loss_vjp(params, data, target)                       # :70-92
        # :89-94: loss and gradient averaged over the ranks in one message
        packed = constants.pmean_vector(torch.cat([flat.to(torch.float64), loss.reshape(1)]))
        loss_val, flat = packed[-1], packed[:-1].to(flat.dtype)
        state, params = opt_update(state.get('count', 0), system.unpack_grad(flat, params), params, state)   # :95-96
        # :97-104: logprob = 2 log|psi_new(x)|, then one symmetric all-electron move
        data = data.clone()
        logprob = torch.empty(data.shape[0], dtype=data.dtype, device=data.device)
        num_accepts = batch_network.system.mcmc_step(params, data, logprob, 1, mcmc_width, seed=_philox_seed(key))
        return data, params, state, loss_val, logprob, num_accepts[0]

    return pretrain_step


def pretrain_hartree_fock(params, data, batch_network, batch_orbitals, sharded_key, cell, scf_approx, full_det=False,
                          iterations=1000, learning_rate=5e-3, history=None):
    """pretrain.py:110-169: `iterations` steps of Adam(learning_rate) on the orbital-matching loss, the walkers following the
    network's own density.  `sharded_key`: int seed or torch.Generator; `cell`: the simulation cell; `scf_approx`: see the
    module docstring.  One log line per iteration with the reference's five quantities; a list passed as `history` receives
    them as dicts (iteration, loss, pmove, logprob, logprob_target).  -> (params, data)."""
    from . import train
    from .inference import _rank_generator
    optimizer = train.adam(learning_rate)
    state = optimizer[0](params)
    pretrain_step = make_pretrain_step(batch_orbitals, batch_network, cell.lattice_vectors(), optimizer, full_det=full_det)
    gen = _rank_generator(sharded_key, data.device)
    n = int(cell.nelectron) if hasattr(cell, 'nelectron') else int(sum(cell.nelec))
    batch = data.shape[0]
    for t in range(iterations):
        xs = data.reshape(-1, n, 3).to(torch.float64)
        # :152 -- numpy float64 on the host, what hf.SCF takes; a provider marked `on_device` gets the device tensor
        # (`_targets` below restates these lines for pretrain_hartree_fock_usingHF: keep the two in step)
        target = scf_approx.eval_orb_mat(xs if getattr(scf_approx, 'on_device', False) else xs.cpu().numpy())
        target = [torch.as_tensor(np.asarray(tar)) if not isinstance(tar, torch.Tensor) else tar for tar in target]
        target = [tar.to(data.device).reshape(batch, ne, ne) for tar, ne in zip(target, cell.nelec) if ne > 0]   # :154-155
        # :157-158 (a singular target gives -inf here and nothing else)
        slogprob_target = functools.reduce(lambda a, b: a + b, [2 * torch.linalg.slogdet(tar)[1] for tar in target])
        data, params, state, loss, logprob, num_accepts = pretrain_step(data, target, params, state, gen)
        pmove, lp, lpt = constants.pmean_packed(num_accepts / batch, logprob.mean(), slogprob_target.mean())
        row = {'iteration': t, 'loss': float(loss), 'pmove': float(pmove), 'logprob': float(lp), 'logprob_target': float(lpt)}
        logging.info('Pretrain iter %05d: Loss=%03.6f, pmove=%0.2f, Norm of Net prob=%03.4f, Norm of HF prob=%03.4f',
                     t, row['loss'], row['pmove'], row['logprob'], row['logprob_target'])
        if history is not None:
            history.append(row)
    return params, data


def _targets(scf_approx, data, n, nelec):
    """pretrain.py:152-155 / :286-287: the target list at walkers `data` (B, 3N), empty spin channels dropped.  The same lines
    stand inline in `pretrain_hartree_fock`, which is kept as it was: keep the two in step."""
    batch = data.shape[0]
    xs = data.reshape(-1, n, 3)
    if getattr(scf_approx, 'on_device', False):
        target = scf_approx.eval_orb_mat(xs)
    else:
        target = scf_approx.eval_orb_mat(xs.to(torch.float64).cpu().numpy())
    target = [torch.as_tensor(np.asarray(tar)) if not isinstance(tar, torch.Tensor) else tar for tar in target]
    return [tar.to(data.device).reshape(batch, ne, ne) for tar, ne in zip(target, nelec) if ne > 0]


def _hf_logprob(scf_approx, data, n):
    """2 log|det_HF| at walkers `data` (B, 3N) as a device tensor of data's dtype (pretrain.py:265-266)."""
    xs = data.reshape(-1, n, 3)
    if getattr(scf_approx, 'on_device', False):
        logabs = scf_approx.eval_slogdet(xs)[1]
    else:
        logabs = torch.as_tensor(np.asarray(scf_approx.eval_slogdet(xs.to(torch.float64).cpu().numpy())[1]))
    return (2.0 * logabs).to(device=data.device, dtype=data.dtype).contiguous()


def pretrain_hartree_fock_usingHF(params, data, batch_orbitals, sharded_key, cell, scf_approx, iterations=1000, learning_rate=5e-3,
                                  nsteps=1, full_det=False, history=None, noise=None):
    """pretrain.py:172-302 (`pretrain.method = 'hf'`): Adam(learning_rate) on the orbital-matching loss with the walkers
    following the HARTREE-FOCK density, so there is no network move.  Per iteration: `nsteps` symmetric all-electron moves of
    width 0.02 on 2 log|det_HF| (`ds_mh_propose`, `scf_approx.eval_slogdet`, `ds_mh_accept`; torch noise on the device), the
    targets at the new walkers, one loss / gradient / Adam update through `ds_pretrain_loss_vjp`, and the log line of :295-300
    (the network's 2 log|det| summed over spins from `batch_orbitals`, before the update, as the reference evaluates it).
    `scf_approx` needs `eval_orb_mat` and `eval_slogdet`; with a true `on_device` both get device tensors, else numpy on the host.
    `noise=(normals (iterations, nsteps, B, 3N), uniforms (iterations, nsteps, B))` replays explicit tensors instead of drawing.
    `history` receives one dict per iteration (iteration, loss, pmove, logprob, logprob_target, and `accepts`: this rank's accept
    count of each of the nsteps moves).  -> (params, data)."""
    from . import train
    from .inference import _rank_generator
    if not isinstance(batch_orbitals, NetworkApply) or batch_orbitals.method_name != 'eval_mats':
        raise TypeError("expected the .apply of make_solid_fermi_net(method_name='eval_mats')")
    if bool(batch_orbitals.net_kw.get('full_det', False)) != bool(full_det):
        raise ValueError('full_det differs from the setting the network was built with')
    if not hasattr(scf_approx, 'eval_slogdet'):
        raise TypeError("pretrain method 'hf' samples the target density: scf_approx needs eval_slogdet next to eval_orb_mat")
    system = batch_orbitals.system
    from .qmc import _check_latvec
    _check_latvec(cell.lattice_vectors(), system)
    opt_init, opt_update = train.adam(learning_rate)
    state = opt_init(params)
    gen = None if noise is not None else _rank_generator(sharded_key, data.device)
    n = int(cell.nelectron) if hasattr(cell, 'nelectron') else int(sum(cell.nelec))
    batch = data.shape[0]
    width = 0.02                                    # the default of the reference's mh_update, never overridden (:269-273)
    data = data.clone().contiguous()
    logprob = _hf_logprob(scf_approx, data, n)                                          # :265-266
    n_accept = torch.zeros(max(1, nsteps), dtype=data.dtype, device=data.device)     # one counter per move of an iteration
    for t in range(iterations):
        n_accept.zero_()
        for i in range(nsteps):                                                         # :277-283
            if noise is not None:
                normal = noise[0][t, i].to(device=data.device, dtype=data.dtype)
                uniform = noise[1][t, i].to(device=data.device, dtype=data.dtype).contiguous()
            else:
                normal = torch.randn(data.shape, dtype=data.dtype, device=data.device, generator=gen)
                uniform = torch.rand(batch, dtype=data.dtype, device=data.device, generator=gen)
            x2 = system.mh_propose(data, normal, width)
            lp2 = _hf_logprob(scf_approx, x2, n)
            system.mh_accept(data, logprob, x2, lp2, uniform, n_accept[i:i + 1])
        target = _targets(scf_approx, data, n, cell.nelec)                              # :286-287
        # :289-290 -- with the parameters of before the update
        slogprob_net = functools.reduce(lambda a, b: a + b, [2 * torch.linalg.slogdet(m)[1] for m in batch_orbitals(params, data)])
        loss, flat = system.pretrain_loss_vjp(params, data, target)                     # :293
        packed = constants.pmean_vector(torch.cat([flat.to(torch.float64), loss.reshape(1)]))
        loss_val, flat = packed[-1], packed[:-1].to(flat.dtype)
        state, params = opt_update(state.get('count', 0), system.unpack_grad(flat, params), params, state)
        pmove, lpn, lpt = constants.pmean_packed(n_accept[-1] / batch, slogprob_net.mean(), logprob.mean())
        row = {'iteration': t, 'loss': float(loss_val), 'pmove': float(pmove), 'logprob': float(lpn), 'logprob_target': float(lpt)}
        logging.info('Pretrain iter %05d: Loss=%03.6f, pmove=%0.2f, Norm of Net prob=%03.4f, Norm of HF prob=%03.4f',
                     t, row['loss'], row['pmove'], row['logprob'], row['logprob_target'])
        if history is not None:
            history.append(dict(row, accepts=[int(v) for v in n_accept[:nsteps].tolist()]))
    return params, data
