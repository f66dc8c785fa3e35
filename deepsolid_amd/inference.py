"""Driver loops.  `run_inference`: energy evaluation of a fixed wavefunction, the `optimizer='none'` branch of the reference driver
(reference DeepSolid/process.py:256-374), i.e. burn-in, then per iteration
``mcmc_step -> total_energy -> one CSV row -> MCMC width adaptation``.

This is SURVEY.md section 8 row f1: the smallest step from "kernel" to "usable VMC energy of a trained
wavefunction".  Everything numeric runs in the HIP chain; this module is host bookkeeping only.
"""
import logging
import os

import numpy as np
import torch

from . import qmc, train

TRAIN_SCHEMA = ['step', 'energy', 'variance', 'pmove', 'imaginary', 'kinetic', 'ewald']   # process.py:276


class Writer:
    """CSV writer with the reference's file layout (utils/writers.py:27-91, iteration_key=None)."""

    def __init__(self, name, schema, directory='logs/'):
        self._schema = list(schema)
        os.makedirs(directory, exist_ok=True)
        self._filename = os.path.join(directory, name + '.csv')

    def __enter__(self):
        header = not os.path.exists(self._filename)
        self._file = open(self._filename, 'a+')
        if header:
            self._file.write(','.join(self._schema) + '\n')
        return self

    def write(self, t, **data):
        for key in data:
            if key not in self._schema:
                raise ValueError('Not a recognized key for writer: %s' % key)
        self._file.write(','.join(str(data.get(key, '')) for key in self._schema) + '\n')

    def __exit__(self, *exc):
        self._file.flush()
        self._file.close()


def _rank_generator(key, device, t_init=0):
    """Per-rank noise stream: the reference folds the host index into the key and splits it per device
    (process.py:104, constants.py:54-57); here one process drives one GPU, so the rank is folded into the seed.
    Walkers must be initialised per rank as well (`init_guess.init_electrons` takes its own key).
    `t_init` (the first iteration of a resumed run) is folded in as well, so that a run restarted from a checkpoint with
    the same key does not replay the noise of iterations 0..k of the first run (the reference draws a fresh, time-based
    key on every start, process.py:99-104)."""
    if isinstance(key, torch.Generator):
        return key
    from . import constants
    seed = int(key) * max(1, constants.world_size()) + constants.rank()
    seed = (seed + 0x9E3779B97F4A7C15 * int(t_init)) % (1 << 63)
    return torch.Generator(device=device).manual_seed(seed)


def _observables(simulation_cell, complex_polarization, structure_factor, structure_factor_nq, save_path):
    """cfg.log.complex_polarization / cfg.log.structure_factor (base_config.py:94-95, process.py:277-283): -> (schema, f) with
    f(data) -> dict of the observables for the returned row (and the CSV column), appending the S(k) row to
    <save_path>/structure_factor.csv on every call (process.py:339-342); f is None when both switches are off."""
    schema = list(TRAIN_SCHEMA)
    if not (complex_polarization or structure_factor):
        return schema, None
    from . import estimator
    if complex_polarization:
        schema.append('complex_polarization')                            # process.py:277-278
    obs = estimator.make_observables(simulation_cell, polarization_direction=0 if complex_polarization else None,
                                     nq=structure_factor_nq if structure_factor else None)
    sk_path = os.path.join(save_path, 'structure_factor.csv') if save_path else None

    def evaluate(data):
        pol, sk = obs(data)
        out = {}
        if pol is not None:
            out['complex_polarization'] = np.asarray(pol.cpu().numpy())  # process.py:362
        if sk is not None:
            out['structure_factor'] = sk.cpu().numpy()
            if sk_path:
                estimator.append_structure_factor_row(sk_path, out['structure_factor'])
        return out
    return schema, evaluate


def _pseudopotential_kw(pseudopotential, key):
    """Keywords of `train.make_loss` for a run with a pseudopotential (none without: the call is then the one it always was).  A
    generator as `key` has no integer to fold: the rotations are then seeded with 0."""
    if pseudopotential is None:
        return {}
    return dict(pseudopotential=pseudopotential, key=0 if isinstance(key, torch.Generator) else int(key))


def _csv_row(row, schema):
    """The keys of a returned row that are CSV columns (S(k) has a file of its own)."""
    return {k: v for k, v in row.items() if k in schema}


def run_inference(slog_net, logdet_net, params, data, simulation_cell, iterations, key=0, move_width=0.02,
                  mcmc_steps=20, burn_in=100, adapt_frequency=100, stats_frequency=1, save_path=None,
                  stats_file_name='train_stats', laplacian_mode='for', partition_number=3, complex_polarization=False,
                  structure_factor=False, structure_factor_nq=4, accumulators=(), pseudopotential=None):
    """Returns (data, mcmc_width, rows).  `slog_net` / `logdet_net` are the objects returned by
    ``make_solid_fermi_net(method_name='eval_slogdet' | 'eval_logdet')``; `data` is (B, 3N) on the device.
    Energies are reported per primitive cell like process.py:330-334 (divided by ``simulation_cell.scale``).
    `complex_polarization` / `structure_factor` (cfg.log switches, base_config.py:94-95): evaluate the observables of
    `deepsolid_amd.estimator` on the walkers after every step; rows carry 'complex_polarization' (also a CSV column) and
    'structure_factor' (the nq^3 values, `structure_factor_nq` = nq, one row per iteration in
    <save_path>/structure_factor.csv).
    `accumulators`: `estimator.RealSpaceAccumulator` objects (or anything with `update(data)`, `reduce()` and `save(path,
    results=True)`): each takes the walkers of every iteration after its `total_energy` (one kernel call, nothing is read back),
    is summed over the ranks once on exit and, on rank 0 with a `save_path`, written to <save_path>/realspace.npz (the i-th of
    several to realspace_<i>.npz): counts, walker number, lattices, grid, r edges, normalised density and g(r).  A run that
    raises inside the loop does not reduce (a collective on the way out of an exception could hang the other ranks): with a
    `save_path` every rank writes the counts it has, unreduced, to realspace_partial_rank<r>.npz (realspace_<i>_partial_rank<r>.npz)
    before the exception goes on; `RealSpaceAccumulator.load` + `merge` put such files together.  The return value and the CSV do
    not change; with the default () nothing changes at all.
    `pseudopotential` (`pseudopotential.SemiLocalECP`): passed on to `train.make_loss` with `key`; rows and the CSV then carry a
    'pseudopotential' column (the batch mean of E_loc + E_nl, complex, per primitive cell)."""
    accumulators = tuple(accumulators)
    gen = _rank_generator(key, data.device)
    batch = data.shape[0]
    mcmc_step = qmc.make_mcmc_step(slog_net.apply, batch, latvec=simulation_cell.a, steps=mcmc_steps)
    total_energy = train.make_loss(logdet_net.apply, None, simulation_cell, mode=laplacian_mode,
                                   partition_number=partition_number, **_pseudopotential_kw(pseudopotential, key))
    width = float(move_width)
    for _ in range(burn_in):                                             # process.py:256-261
        data, _ = mcmc_step(params, data, gen, width)
    scale = float(getattr(simulation_cell, 'scale', 1))
    pmoves = np.zeros(adapt_frequency)
    rows = []
    schema, observe = _observables(simulation_cell, complex_polarization, structure_factor, structure_factor_nq, save_path)
    if pseudopotential is not None:
        schema.append('pseudopotential')
    writer = Writer(stats_file_name, schema, save_path) if save_path else None
    if writer:
        writer.__enter__()
    finished = False
    try:
        for t in range(iterations):
            data, pmove = mcmc_step(params, data, gen, width)            # process.py:320
            loss, aux = total_energy(params, data)                       # :321
            row = {'step': t,
                   'energy': float(loss) / scale,                        # :330-334
                   'variance': float(aux.variance) / scale ** 2,
                   'pmove': float(pmove),
                   'imaginary': float(aux.imaginary) / scale,
                   'kinetic': complex(aux.kinetic.mean().item()) / scale,
                   'ewald': float(aux.ewald.mean()) / scale}
            if aux.pseudopotential is not None:
                row['pseudopotential'] = complex(aux.pseudopotential.mean().item()) / scale
            if observe:                                                  # process.py:337-342
                row.update(observe(data))
            for acc in accumulators:
                acc.update(data)
            if t % stats_frequency == 0:
                rows.append(row)
                if writer:
                    writer.write(t, **_csv_row(row, schema))
            if t > 0 and t % adapt_frequency == 0:                       # :368-373
                if np.mean(pmoves) > 0.55:
                    width *= 1.1
                if np.mean(pmoves) < 0.5:
                    width /= 1.1
                pmoves[:] = 0
            pmoves[t % adapt_frequency] = row['pmove']
        finished = True
    finally:
        if writer:
            writer.__exit__(None, None, None)
        if accumulators and save_path and not finished:
            from . import constants
            for i, acc in enumerate(accumulators):
                stem = 'realspace' if i == 0 else f'realspace_{i}'
                acc.save(os.path.join(save_path, f'{stem}_partial_rank{constants.rank()}.npz'))
    if accumulators:
        from . import constants
        for i, acc in enumerate(accumulators):
            acc.reduce()
            if save_path and constants.rank() == 0:
                acc.save(os.path.join(save_path, 'realspace.npz' if i == 0 else f'realspace_{i}.npz'), results=True)
    return data, width, rows


DMC_SCHEMA = ['block', 'energy', 'variance', 'acceptance', 'tau_eff', 'e_trial', 'weight', 'killed']


def run_dmc(slog_net, logdet_net, params, data, simulation_cell, blocks, steps_per_block, tau, key=0, move_width=0.02, mcmc_steps=20,
            burn_in=100, vmc_iterations=20, branch_every=1, e_cut=None, node_mode=0, feedback=10.0, save_path=None,
            stats_file_name='dmc_stats', accumulators=(), pseudopotential=None, state=None, tmoves=False, forward_walking=None):
    """Fixed-phase diffusion Monte Carlo of a fixed wavefunction (`deepsolid_amd.dmc`).
    Returns (state, rows, info).  Equilibrate `data` (B, 3N) with the existing `qmc.make_mcmc_step` (`burn_in` iterations), take
    the VMC energy over `vmc_iterations` more (info['vmc_energy'], info['vmc_error']: reblocked batch means, per primitive cell;
    info['vmc_series']), initialise the DMC state with e_ref = e_trial = that energy, then run `blocks` blocks of
    `steps_per_block` steps, each ONE `ds_dmc_step` call.  Between blocks, on the host, after one packed all-reduce of the stats
    rows: tau_eff = tau * sum p / (B * steps) of the block; e_ref = the running mixed estimate; e_trial = e_ref -
    log(W_global / W_target) / (feedback * tau * steps), W_target = the number of walkers of all ranks.  Ranks comb their own
    populations.  `e_cut` defaults to 0.2 sqrt(N / tau).  One CSV row per block through `Writer`: block, mixed energy per primitive
    cell, variance, acceptance, tau_eff, e_trial, total weight, walkers killed.  `accumulators` are fed the walkers on blocks that
    end on a comb (all weights are then equal, so the unweighted accumulators give mixed estimates); they are refused when
    steps_per_block % branch_every != 0.  `state` (a `dmc.DmcState`, e.g. `DmcState.load`) resumes a run: no equilibration, and the
    same bits as the run that was not interrupted; with a `save_path` the state is written to <save_path>/dmc_state.npz on exit.
    `pseudopotential` (`pseudopotential.SemiLocalECP`): the locality approximation (`dmc.make_dmc_step`; each block then
    synchronises once per step).  The VMC energy that seeds e_ref goes through `train.make_loss(..., pseudopotential=...)`;
    rows and the CSV carry a 'pseudopotential' column: the mixed estimate sum w (E_loc + E_nl) / sum w of the block, complex, per
    primitive cell, from the block's ecp_stats, which cross the ranks in the same packed all-reduce as the stats rows.  Any
    other form of potential is refused (`dmc.make_dmc_step`).
    `tmoves=True` (with a `pseudopotential`): Casula's T-moves (`ds_dmc_step_tmove`) in place of the
    locality approximation; rows and the CSV gain a 'tmoves' column, the T-moves per walker and step of the block, whose sum is
    the fourth ecp_stats column in the same packed all-reduce.
    `forward_walking` (a `dmc.ForwardWalking`): pure estimators by forward walking.  The blocks are then
    built with `want_parents=True` and `forward_walking.update` runs after EVERY block, whatever `branch_every` is (its weights are
    the walkers' own); `reduce()` runs at the end, and with a `save_path` every rank has written its tracker, before the
    reduction, to <save_path>/forward_walking.npz (forward_walking_rank<r>.npz with several ranks, named as the DMC state
    file is).  A `state=` resume continues it with the same bits when the caller passes a tracker that has loaded that file."""
    from . import constants, dmc
    accumulators = tuple(accumulators)
    from .pseudopotential import SemiLocalECP
    if pseudopotential is not None and not isinstance(pseudopotential, SemiLocalECP):
        dmc.make_dmc_step(logdet_net, simulation_cell, tau, steps_per_block, pseudopotential=pseudopotential)      # (refuses it)
    if accumulators and (branch_every <= 0 or steps_per_block % branch_every != 0):
        raise ValueError('accumulators need blocks that end on a comb: steps_per_block must be a multiple of branch_every')
    for acc in accumulators:
        if getattr(acc, 'vmc_only', False):
            raise ValueError(f'{type(acc).__name__} holds a covariance under |psi|^2 (the wave-function term of the stress): it is a VMC '
                             'estimator, a mixed estimate of it is not the DMC value; use it with run_inference')
    system = logdet_net.apply.system
    scale = float(getattr(simulation_cell, 'scale', 1))
    batch = data.shape[0]
    seed = (int(key) if not isinstance(key, torch.Generator) else 0) * max(1, constants.world_size()) + constants.rank()
    info = {}
    if state is None:
        gen = _rank_generator(key, data.device)
        mcmc_step = qmc.make_mcmc_step(slog_net.apply, batch, latvec=simulation_cell.a, steps=mcmc_steps)
        total_energy = None if pseudopotential is None else train.make_loss(logdet_net.apply, None, simulation_cell,
                                                                            **_pseudopotential_kw(pseudopotential, key))
        for _ in range(burn_in):
            data, _ = mcmc_step(params, data, gen, float(move_width))
        series = []
        for _ in range(max(int(vmc_iterations), 1)):
            data, _ = mcmc_step(params, data, gen, float(move_width))
            if total_energy is not None:
                series.append(float(total_energy(params, data)[0]))        # (the loss is the mean over all ranks already)
                continue
            ke, ew, _, _ = system.local_energy(params, data)
            mean = constants.pmean_if_pmap((ke[:, 0].double() + ew.double()).mean())
            series.append(float(mean))
        e_vmc, err_vmc, _ = dmc.reblock(series)
        info.update(vmc_energy=e_vmc / scale, vmc_error=err_vmc / scale, vmc_series=np.asarray(series) / scale)
        state = dmc.DmcState.fresh(system, data, tau, e_vmc, ecp=pseudopotential is not None)
    block_fn = dmc.make_dmc_step(logdet_net, simulation_cell, tau, steps_per_block, e_cut=e_cut, node_mode=node_mode,
                                 branch_every=branch_every, seed=seed, pseudopotential=pseudopotential, tmoves=tmoves,
                                 want_parents=forward_walking is not None)
    w_target = float(batch * max(1, constants.world_size()))
    rows = []
    schema = DMC_SCHEMA + (['pseudopotential'] if pseudopotential is not None else []) + (['tmoves'] if tmoves else [])
    writer = Writer(stats_file_name, schema, save_path) if save_path else None
    if writer:
        writer.__enter__()
    try:
        for b in range(blocks):
            tau_eff, e_trial = state.tau_eff, state.e_trial
            st = block_fn(params, state)
            if pseudopotential is not None:                # (the ecp_stats columns -- three, four with T-moves -- ride behind the nine of the stats rows)
                st = torch.cat([st, block_fn.ecp_stats], dim=1)
            st = constants.psum_if_pmap(st).cpu().numpy()                               # ONE packed all-reduce per block
            w, we, we2 = st[:, 0].sum(), st[:, 1].sum(), st[:, 2].sum()
            energy = we / w
            state.sum_w, state.sum_we = state.sum_w + float(w), state.sum_we + float(we)
            combed = st[:, 8] > 0
            row = {'block': b, 'energy': energy / scale, 'variance': (we2 / w - energy ** 2) / scale ** 2,
                   'acceptance': st[:, 3].sum() / (w_target * steps_per_block), 'tau_eff': tau_eff, 'e_trial': e_trial / scale,
                   'weight': float(st[-1, 0]), 'killed': int((w_target - st[combed, 8]).sum()) if branch_every > 0 else 0}
            if pseudopotential is not None:
                row['pseudopotential'] = complex(st[:, 9].sum() + st[:, 10].sum(), st[:, 11].sum()) / w / scale
            if tmoves:
                row['tmoves'] = float(st[:, 12].sum()) / (w_target * steps_per_block)
            rows.append(row)
            if writer:
                writer.write(b, **row)
            state.tau_eff = float(tau) * float(st[:, 4].sum()) / (w_target * steps_per_block)
            state.e_ref = state.sum_we / state.sum_w
            state.e_trial = state.e_ref - float(np.log(st[-1, 0] / w_target)) / (float(feedback) * float(tau) * steps_per_block)
            for acc in accumulators:
                acc.update(state.arrays['x'])
            if forward_walking is not None:
                forward_walking.update(system, state, block_fn.parents)
    finally:
        if writer:
            writer.__exit__(None, None, None)
    for i, acc in enumerate(accumulators):
        acc.reduce()
        if save_path and constants.rank() == 0:
            acc.save(os.path.join(save_path, 'realspace.npz' if i == 0 else f'realspace_{i}.npz'), results=True)
    if forward_walking is not None:
        if save_path:
            forward_walking.save(os.path.join(save_path, f'forward_walking_rank{constants.rank()}.npz' if constants.world_size() > 1
                                              else 'forward_walking.npz'))
        forward_walking.reduce()
    if save_path:
        state.save(os.path.join(save_path, f'dmc_state_rank{constants.rank()}.npz' if constants.world_size() > 1 else 'dmc_state.npz'))
    series = np.asarray([r['energy'] for r in rows])
    if len(series):
        e, err, _ = dmc.reblock(series)
        info.update(energy=e, error=err)
    return state, rows, info


def learning_rate_schedule(rate=5e-2, decay=1.0, delay=10000.0):
    """process.py:200-202 with the defaults of base_config.py:46-51."""
    return lambda t: rate * (1.0 / (1.0 + t / delay)) ** decay


def run_training(slog_net, logdet_net, params, data, simulation_cell, iterations, key=0, move_width=0.02, mcmc_steps=10,
                 burn_in=100, adapt_frequency=100, learning_rate=None, clip_local_energy=5.0, clip_type='real',
                 save_path=None, save_every=None, stats_file_name='train_stats', laplacian_mode='for',
                 partition_number=3, t_init=0, opt_state=None, check_nan=True, max_rejected=20, complex_polarization=False,
                 structure_factor=False, structure_factor_nq=4, pretrain_iterations=0, pretrain_lr=5e-3, scf_approx=None,
                 optimizer='adam', kfac=None, pretrain_method='net', pretrain_steps=1, pseudopotential=None, spring=None):
    """The `optimizer='adam'` branch of the reference driver (process.py:204-219, 256-383): burn-in, then per iteration
    ``mcmc_step -> value_and_grad(total_energy) -> gradient pmean -> Adam -> CSV row -> width adaptation``, with
    checkpoints in the reference's layout (`deepsolid_amd.checkpoint.save`) every `save_every` iterations.
    `params` is updated in place.  Returns (data, params, opt_state, mcmc_width, rows).
    `check_nan` (cfg.debug.check_nan, process.py:303-318; on by default here: Adam updates in place, one NaN gradient would
    poison the parameters for good): a step with non-finite local energies / loss / gradient is discarded -- walkers,
    parameters and optimiser state keep their values, no CSV row is written for it (process.py:344), `rows` gets
    ``{'step': t, 'rejected': True, 'pmove': ...}`` and a warning is logged like the reference's (process.py:316).  A walker with a
    non-finite coordinate or non-finite parameters can never recover (the move is never accepted, the step never kept), so
    after `max_rejected` (default 20) rejections IN A ROW the loop writes the state it is stuck in (walkers, parameters, optimiser
    state: nothing of a rejected step was kept) as `aborted_ckpt_<t>.npz` -- a name `find_last_checkpoint` does not pick up, so a
    restart resumes from the last regular checkpoint -- and raises instead of running to the end doing nothing;
    `max_rejected=None` is the reference's behaviour: log and go on (process.py:303-318).
    `complex_polarization` / `structure_factor` / `structure_factor_nq`: as in `run_inference`; the observables are evaluated on
    the walkers the step returns, rejected steps included (their rows carry them too), and the S(k) row is written for a
    rejected step as well, since the reference writes it before its `loss is not None` gate (process.py:339-345).
    `pretrain_iterations` > 0 on a fresh start (`t_init == 0`): the orbital-matching stage of process.py:148-179 runs first
    (`deepsolid_amd.pretrain.pretrain_hartree_fock`, Adam with `pretrain_lr`, base_config.py:149-154) against `scf_approx`
    (any object with `eval_orb_mat`; None: the plane waves of the network's own `klist`).  0 (default): no such stage.
    `pretrain_method` (cfg.pretrain.method, process.py:148,164): 'net' moves the walkers on the network's density, 'hf' on the
    Hartree-Fock density of `scf_approx` (`pretrain_hartree_fock_usingHF`, `pretrain_steps` = cfg.pretrain.steps moves per
    iteration); 'hf' needs a `scf_approx` with `eval_slogdet` (`deepsolid_amd.hf.GaussianOrbitals`): plane waves are singular
    as a density.
    `optimizer='kfac'`: the reference's default optimizer instead (process.py:209-228; `deepsolid_amd.kfac`): the factor pass, the
    damped inverses and the preconditioner run on the GPU every iteration.  `kfac`: dict of the keys of base_config.py:62-75
    (invert_every, damping, cov_ema_decay, norm_constraint, l2_reg; momentum must be 0, register_only_generic False); `learning_rate`
    is then the schedule of the optimizer's own step count.  `opt_state` of a resumed run is the dict `checkpoint.restore` returns
    (through `checkpoint.opt_state_to_single_device`).
    `optimizer='spring'`: SPRING on the per-walker Jacobian (`deepsolid_amd.spring`; beyond the reference): Jacobian pass, Gram
    matrix, solve and the two matrix-vector products on the GPU every iteration; one rank only.  `spring`: dict of the keys
    damping (1e-3), mu (0.99; 0 is MinSR), norm_constraint (1e-3); `learning_rate` is the schedule of the optimizer's own step
    count.  `opt_state` of a resumed run as for kfac.
    `pseudopotential`: as in `run_inference`; all optimizers take their energies from `aux.local_energy` of the same
    `total_energy`, so the gradient follows without another change."""
    from . import checkpoint
    if optimizer not in ('adam', 'kfac', 'spring'):
        raise ValueError(f"optimizer must be 'adam', 'kfac' or 'spring', got {optimizer!r}")
    if kfac is not None and optimizer != 'kfac':
        raise ValueError("the `kfac` settings need optimizer='kfac'")
    if spring is not None and optimizer != 'spring':
        raise ValueError("the `spring` settings need optimizer='spring'")
    if pretrain_method not in ('net', 'hf'):
        raise ValueError(f"pretrain_method must be 'net' or 'hf', got {pretrain_method!r}")
    if pretrain_method == 'hf' and scf_approx is None:
        raise ValueError("pretrain_method='hf' samples the Hartree-Fock density and needs scf_approx (deepsolid_amd.hf."
                         "GaussianOrbitals); the plane-wave stand-in is singular as a density")
    if pretrain_iterations > 0 and t_init == 0:
        from . import pretrain
        from .network import NetworkApply
        net = slog_net.apply
        orbitals = NetworkApply(net.simulation_cell, net.klist, net.net_kw, 'eval_mats', net.dtype)
        full_det = bool(net.net_kw.get('full_det', False))
        if pretrain_method == 'hf':
            params, data = pretrain.pretrain_hartree_fock_usingHF(
                params, data, orbitals, key, simulation_cell, scf_approx, iterations=pretrain_iterations,
                learning_rate=pretrain_lr, nsteps=pretrain_steps, full_det=full_det)
        else:
            params, data = pretrain.pretrain_hartree_fock(
                params, data, net, orbitals, key, simulation_cell, scf_approx or pretrain.PlaneWaveOrbitals(net.klist),
                full_det=full_det, iterations=pretrain_iterations, learning_rate=pretrain_lr)
    gen = _rank_generator(key, data.device, t_init)
    batch = data.shape[0]
    mcmc_step = qmc.make_mcmc_step(slog_net.apply, batch, latvec=simulation_cell.a, steps=mcmc_steps)
    total_energy = train.make_loss(logdet_net.apply, None, simulation_cell, clip_local_energy=clip_local_energy,
                                   clip_type=clip_type, mode=laplacian_mode, partition_number=partition_number,
                                   **_pseudopotential_kw(pseudopotential, key))
    schedule = learning_rate if learning_rate is not None else learning_rate_schedule()
    if optimizer == 'kfac':
        from . import kfac as kfac_mod
        cfg = dict(kfac or {})
        known = {'invert_every': 1, 'cov_update_every': 1, 'damping': 1e-3, 'cov_ema_decay': 0.95, 'momentum': 0.0,
                 'momentum_type': 'regular', 'min_damping': 1e-4, 'norm_constraint': 1e-3, 'mean_center': True, 'l2_reg': 0.0,
                 'register_only_generic': False}
        unknown = sorted(set(cfg) - set(known))
        if unknown:
            raise ValueError(f'unknown kfac settings {unknown} (base_config.py:62-75)')
        cfg = {**known, **cfg}
        if cfg['cov_update_every'] != 1:
            raise NotImplementedError('kfac: cov_update_every != 1 is not supported (process.py never passes it on)')
        kfac_opt = kfac_mod.kfac(schedule, damping=cfg['damping'], l2_reg=cfg['l2_reg'], norm_constraint=cfg['norm_constraint'],
                                 cov_ema_decay=cfg['cov_ema_decay'], invert_every=cfg['invert_every'], momentum=cfg['momentum'],
                                 register_only_generic=cfg['register_only_generic'])
        if opt_state is None:
            opt_state = kfac_opt[0](params)
        step = kfac_mod.make_kfac_training_step(mcmc_step, total_energy, kfac_opt, check_nan=check_nan)
    elif optimizer == 'spring':
        from . import spring as spring_mod
        cfg = dict(spring or {})
        known = {'damping': 1e-3, 'mu': 0.99, 'norm_constraint': 1e-3}
        unknown = sorted(set(cfg) - set(known))
        if unknown:
            raise ValueError(f'unknown spring settings {unknown} (known: {sorted(known)})')
        cfg = {**known, **cfg}
        spring_opt = spring_mod.spring(schedule, damping=cfg['damping'], mu=cfg['mu'], norm_constraint=cfg['norm_constraint'])
        if opt_state is None:
            opt_state = spring_opt[0](params)
        step = spring_mod.make_spring_training_step(mcmc_step, total_energy, spring_opt, check_nan=check_nan)
    else:
        opt_init, opt_update = train.adam(schedule)
        if opt_state is None:
            opt_state = opt_init(params)
        step = train.make_training_step(mcmc_step, total_energy, opt_update, check_nan=check_nan)
    width = float(move_width)
    if t_init == 0:                                                      # process.py:256: burn-in only on a fresh start
        for _ in range(burn_in):
            data, _ = mcmc_step(params, data, gen, width)
    scale = float(getattr(simulation_cell, 'scale', 1))
    pmoves = np.zeros(adapt_frequency)
    rows = []
    schema, observe = _observables(simulation_cell, complex_polarization, structure_factor, structure_factor_nq, save_path)
    if pseudopotential is not None:
        schema.append('pseudopotential')
    writer = Writer(stats_file_name, schema, save_path) if save_path else None
    if writer:
        writer.__enter__()
    t_last = t_init + iterations - 1
    n_rejected = 0
    try:
        for t in range(t_init, t_init + iterations):
            data, params, opt_state, loss, aux, pmove, _ = step(t, data, params, opt_state, gen, width)
            observed = observe(data) if observe else {}                  # process.py:337-342
            if loss is None:                                             # rejected step: nothing was updated, no CSV row
                rows.append({'step': t, 'rejected': True, 'pmove': float(pmove), **observed})
                n_rejected += 1
                logging.warning('step %d: non-finite local energy / loss / gradient, step discarded (%d in a row)', t, n_rejected)
                if max_rejected is not None and n_rejected >= max_rejected:
                    if save_path:
                        # post-mortem state under a name of its own: a restart must not resume from it (the walkers or parameters
                        # that made every step fail are IN it), and it is the state from before the first rejected step, not step t's
                        checkpoint.save(save_path, t, data, params, opt_state, width, prefix='aborted_ckpt_')
                    raise FloatingPointError(f'{n_rejected} consecutive training steps were rejected for non-finite values '
                                             f'(last at step {t}): walkers or parameters are not finite')
            else:
                row = {'step': t, 'energy': float(loss) / scale, 'variance': float(aux.variance) / scale ** 2,
                       'pmove': float(pmove), 'imaginary': float(aux.imaginary) / scale,
                       'kinetic': complex(aux.kinetic.mean().item()) / scale, 'ewald': float(aux.ewald.mean()) / scale}
                if aux.pseudopotential is not None:
                    row['pseudopotential'] = complex(aux.pseudopotential.mean().item()) / scale
                row.update(observed)
                n_rejected = 0
                rows.append(row)
                if writer:
                    writer.write(t, **_csv_row(row, schema))
            if t > 0 and t % adapt_frequency == 0:                       # process.py:368-373
                if np.mean(pmoves) > 0.55:
                    width *= 1.1
                if np.mean(pmoves) < 0.5:
                    width /= 1.1
                pmoves[:] = 0
            pmoves[t % adapt_frequency] = float(pmove)
            # process.py:376-383: every `save_every` iterations and always at the last one; the Adam moments and
            # step count travel with the parameters (process.py:381 saves opt_state)
            if save_path and ((save_every and (t + 1) % save_every == 0) or t >= t_last):
                checkpoint.save(save_path, t, data, params, opt_state, width)
    finally:
        if writer:
            writer.__exit__(None, None, None)
    return data, params, opt_state, width, rows

