"""Walker observables of the reference's estimator.py: the complex polarization (:15-42) and the structure factor S(k)
(:44-84), the two quantities the driver logs when ``cfg.log.complex_polarization`` / ``cfg.log.structure_factor`` are set
(process.py:277-283, 337-342, 361-362).

The batch sums come from one HIP call (``device.observable_sums``, csrc/ds_obs.h); what is left here is host algebra on a few
hundred numbers: per-rank means, ONE packed all-reduce of them (``constants.pmean_vector``), and
S(k) = (pmean<|rho|^2> - |pmean<rho>|^2) / N -- the reference takes the pmeans of <rho> and <|rho|^2> separately and only
then forms S(k) (:73-81), it never averages per-rank S(k).
"""
import numpy as np
import torch

from . import constants

_COMPLEX = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def structure_factor_grid(nq):
    """(nq^3, 3) integer points in the order of estimator.py:55-56: ``jnp.meshgrid`` indexes 'xy', so point
    p = i nq^2 + j nq + k is (n1, n2, n3) = (j, i, k)."""
    mesh = np.meshgrid(*[np.arange(nq) for _ in range(3)])
    return np.stack([m.ravel() for m in mesh], axis=0).T.astype(np.int32)


def combine_sums(sums, batch, n_q, polarization, nelec, dtype=torch.float64):
    """Packed batch sums of one rank (the layout of ``ds_observables``) -> (polarization or None, S(k) or None).
    Only the requested observables travel in the all-reduce; with world size 1 nothing is reduced."""
    sums = sums.to(torch.float64)
    parts = []
    if polarization:
        parts.append(sums[:2])
    if n_q:
        parts.append(sums[2:2 + 3 * n_q])
    if not parts:
        return None, None
    means = constants.pmean_vector(torch.cat(parts) / batch)
    pol = sk = None
    if polarization:
        pol = torch.complex(means[0], means[1]).to(_COMPLEX[dtype])
        means = means[2:]
    if n_q:
        one_re, one_im, two = means[:n_q], means[n_q:2 * n_q], means[2 * n_q:3 * n_q]
        sk = ((two - (one_re * one_re + one_im * one_im)) / nelec).to(dtype)
    return pol, sk


def make_observables(simulation_cell, polarization_direction=None, nq=None, ndim=3):
    """Both observables from one kernel call and one all-reduce: f(data) -> (polarization or None, S(k) or None).
    `polarization_direction` None / `nq` None switches the one off."""
    if ndim != 3:
        raise ValueError(f'ndim = {ndim}: only three-dimensional walkers are supported')
    if polarization_direction is not None and polarization_direction not in (0, 1, 2):
        raise ValueError(f'polarization direction must be 0, 1 or 2, got {polarization_direction}')
    if nq is not None and not 1 <= int(nq) <= 8:
        raise ValueError(f'nq = {nq}: the structure factor supports 1 <= nq <= 8')
    recvec = np.asarray(simulation_cell.reciprocal_vectors(), dtype=np.float64)
    nelec = int(simulation_cell.nelectron) if hasattr(simulation_cell, 'nelectron') else int(sum(simulation_cell.nelec))
    grid = structure_factor_grid(int(nq)) if nq is not None else np.zeros((0, 3), np.int32)
    pol_dir = -1 if polarization_direction is None else int(polarization_direction)

    def observables(data):
        from . import device
        if data.shape[-1] != 3 * nelec:
            raise ValueError(f'walkers have {data.shape[-1]} coordinates, the cell has {nelec} electrons')
        x = data.reshape(-1, 3 * nelec)
        sums = device.observable_sums(recvec, x, grid, pol_dir)
        return combine_sums(sums, x.shape[0], grid.shape[0], pol_dir >= 0, nelec, x.dtype)

    return observables


def make_complex_polarization(simulation_cell, direction=0, ndim=3):
    """estimator.py:15-42: f(data (B, 3N)) -> complex scalar tensor, the batch (and rank) mean of exp(i g_dir . sum_e r_e)."""
    f = make_observables(simulation_cell, polarization_direction=direction, ndim=ndim)
    return lambda data: f(data)[0]


def make_structure_factor(simulation_cell, nq=4, ndim=3):
    """estimator.py:44-84: f(data (B, 3N)) -> real (nq^3,) tensor S(k) = (<|rho_k|^2> - |<rho_k>|^2) / N on the
    grid of ``structure_factor_grid(nq)``, in the dtype of the walkers."""
    f = make_observables(simulation_cell, nq=nq, ndim=ndim)
    return lambda data: f(data)[1]


def _csv_value(v):
    """One value as pandas' DataFrame.to_csv writes it (default float_format, na_rep='')."""
    if np.isnan(v):
        return ''
    return repr(float(v)) if v.dtype == np.float64 else str(v)


def append_structure_factor_row(path, sk):
    """Append S(k) to `path` exactly as process.py:339-342 does with
    ``pd.DataFrame(sk[None, :]).to_csv(path, mode='a', sep=',', header=False)``: the row index 0, then the nq^3 values."""
    sk = np.asarray(sk.detach().cpu() if isinstance(sk, torch.Tensor) else sk).reshape(-1)
    with open(path, 'a') as f:
        f.write(','.join(['0'] + [_csv_value(v) for v in sk]) + '\n')
