"""Fixed-phase diffusion Monte Carlo on the device: host bookkeeping around `ds_dmc_step` (csrc/ds_dmc.h; the algorithm is stated
in include/deepsolid_hip.h and DESIGN.md section 19).  The reference has no DMC; the conventions are this project's own.

`make_dmc_step` returns the block function (one C-ABI call per block of steps; no host synchronisation inside WITHOUT a
pseudopotential -- with one, `ds_dmc_step_ecp` synchronises the stream once per step and once more for the initialisation, to
read the pair total of every pseudopotential evaluation; `ds_dmc_step_tmove`, the same with T-moves, once per step), `DmcState` holds
the six walker arrays (seven with a pseudopotential: 'epp') with the scalars a run carries between blocks (`save` / `load`: one .npz of numbers; a resumed run continues
bit-identically), `reblock` is the blocking error bar of a correlated series.  The driver loop is `inference.run_dmc`.
"""
import numpy as np
import torch

STATS = ('w', 'we', 'we2', 'accepted', 'p', 'clipped', 'nonfinite', 'w2', 'parents')        # columns of a stats row


def default_e_cut(n_elec, tau):
    """The energy cut-off of Zen, Sorella, Gillan, Michaelides and Alfe (Phys. Rev. B 93, 241118): 0.2 sqrt(N / tau)."""
    return 0.2 * float(np.sqrt(n_elec / tau))


class DmcState:
    """Walker state of a DMC run: `arrays` = dict of x, logabs, phase, drift, eloc, weight -- and epp (B, 3) float64 = (E_loc,
    Re E_nl, Im E_nl) in a run with a pseudopotential -- (device tensors, updated in place by every block) and the scalars e_trial, e_ref, tau_eff, offset (the Philox offset of the next step), valid (False until the
    first block has filled logabs .. eloc from x)."""

    def __init__(self, arrays, e_trial=0.0, e_ref=0.0, tau_eff=0.0, offset=0, valid=False, sum_w=0.0, sum_we=0.0):
        self.arrays, self.e_trial, self.e_ref, self.tau_eff, self.offset, self.valid = arrays, float(e_trial), float(e_ref), \
            float(tau_eff), int(offset), bool(valid)
        self.sum_w, self.sum_we = float(sum_w), float(sum_we)        # the running mixed estimate e_ref = sum_we / sum_w

    @classmethod
    def fresh(cls, system, x, tau, e_trial, e_ref=None, weight=None, ecp=False):
        return cls(system.dmc_state(x, weight, ecp=True) if ecp else system.dmc_state(x, weight), e_trial, e_trial if e_ref is None else e_ref, tau, 0, False)

    def save(self, path):
        """One .npz of numbers: the six arrays (and epp when the state has it), e_trial, e_ref (with the two sums behind it), tau_eff and the Philox offset."""
        np.savez(path, **{k: v.cpu().numpy() for k, v in self.arrays.items()}, e_trial=np.float64(self.e_trial),
                 e_ref=np.float64(self.e_ref), tau_eff=np.float64(self.tau_eff), offset=np.uint64(self.offset),
                 valid=np.int64(self.valid), sum_w=np.float64(self.sum_w), sum_we=np.float64(self.sum_we))

    @classmethod
    def load(cls, path, device='cuda'):
        with np.load(path) as f:
            names = ('x', 'logabs', 'phase', 'drift', 'eloc', 'weight') + (('epp',) if 'epp' in f.files else ())
            arrays = {k: torch.as_tensor(f[k], device=device).contiguous() for k in names}
            return cls(arrays, float(f['e_trial']), float(f['e_ref']), float(f['tau_eff']), int(f['offset']), bool(int(f['valid'])),
                       float(f['sum_w']), float(f['sum_we']))


def make_dmc_step(logdet_net, simulation_cell, tau, steps, e_cut=None, node_mode=0, branch_every=1, seed=0, pseudopotential=None,
                  tmoves=False):
    """-> block(params, state) -> stats (steps, 9) float64 device tensor: `steps` DMC steps on `state` (a `DmcState`) in place as ONE
    `ds_dmc_step` call, with the state's e_trial, e_ref and tau_eff; the state's Philox offset advances by `steps`.  `e_cut`
    defaults to `default_e_cut`; 0 switches the clip off.  `seed`: the Philox seed (fold the rank into it).
    `pseudopotential` (a `pseudopotential.SemiLocalECP`): the locality approximation, ONE `ds_dmc_step_ecp` call per block, which
    synchronises the stream once per step (and once for the initialisation); the state needs 'epp' (`DmcState.fresh(...,
    ecp=True)`), and the block's `ecp_stats` (steps, 3) = per step sum w E_loc, sum w Re E_nl, sum w Im E_nl stay on
    `block.ecp_stats`.  Any other form of potential is refused.
    `tmoves=True` (needs a `pseudopotential`): Casula's T-moves, ONE `ds_dmc_step_tmove` call per block;
    `block.ecp_stats` is then (steps, 4), the fourth column the number of walkers that made a T-move."""
    from .pseudopotential import SemiLocalECP
    if pseudopotential is not None and not isinstance(pseudopotential, SemiLocalECP):
        raise NotImplementedError('DMC with this form of pseudopotential is not provided: only a pseudopotential.SemiLocalECP in the '
                                  'locality approximation is (no T-moves: DESIGN.md section 19)')
    if tmoves and pseudopotential is None:
        raise ValueError('tmoves=True needs a pseudopotential')
    system = logdet_net.apply.system
    tau = float(tau)
    e_cut = default_e_cut(system.n, tau) if e_cut is None else float(e_cut)
    del simulation_cell                                    # (the handle carries the cell; kept for the signature of the samplers)

    def block(params, state):
        out = system.dmc_step(params, state.arrays, steps, tau, tau_eff=state.tau_eff, e_trial=state.e_trial, e_ref=state.e_ref,
                              e_cut=e_cut, node_mode=node_mode, branch_every=branch_every, seed=seed, offset=state.offset,
                              state_valid=state.valid, **({} if pseudopotential is None else {'ecp': pseudopotential}),
                              **({'tmoves': True} if tmoves else {}))
        state.valid = True
        state.offset += steps
        block.ecp_stats = out.get('ecp_stats')
        return out['stats']
    block.ecp_stats = None
    block.system, block.e_cut, block.steps, block.branch_every = system, e_cut, int(steps), int(branch_every)
    return block


def reblock(series, min_blocks=8):
    """Blocking error bar (Flyvbjerg and Petersen, J. Chem. Phys. 91, 461) of the mean of a correlated series, host numpy.
    -> (mean, error, block length): the series is halved by pair averages while at least `min_blocks` blocks remain; the error
    is the largest standard error of the mean over the levels (the plateau of the blocking curve, from below)."""
    x = np.asarray(series, dtype=np.float64).reshape(-1)
    if len(x) < 2:
        return (float(x.mean()) if len(x) else float('nan')), float('nan'), 1
    mean, best, length, size = float(x.mean()), 0.0, 1, 1
    while len(x) >= max(min_blocks, 2):
        err = float(np.sqrt(x.var(ddof=1) / len(x)))
        if err > best:
            best, length = err, size
        x = 0.5 * (x[0:2 * (len(x) // 2):2] + x[1:2 * (len(x) // 2):2])
        size *= 2
    return mean, best, length
