#!/usr/bin/env python3
"""Generate tests/golden/kfac_inverse.npz by EXECUTING the reference's own `pi_adjusted_inverse` and `psd_inv_cholesky`
(utils/kfac_ferminet_alpha/utils.py:130-218).

Runs only where the reference checkout is (DEEPSOLID_REFERENCE, as tools/make_golden.py).  The module is loaded from its file
under tools/jax_torch_standin.py; the names the stand-in lacks are supplied here: `lax.cond` (a python branch on the predicate),
`jax.scipy.linalg.solve` (torch.linalg.solve in float64), `jax.tree_util`, and `core.axis_frame` raising NameError (no pmap axis:
`pmean_if_pmap` is then the identity, as on one device).

Cases: random SPD pairs of the sizes (2, 3), (33, 8), (65, 32) and one pair whose first factor is zero, each at the dampings 1e-3
and 1e-1.  The file holds, under '<case>:<key>': factor_0, factor_1, damping, inverse_0, inverse_1, and for the first factor
`chol_damping` / `chol_inverse` of a direct `psd_inv_cholesky` call.  Numbers and names only; the archive is written with fixed
member timestamps, so two runs give the same bytes.
"""
import importlib.util
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools import jax_torch_standin as standin            # noqa: E402
from tools.make_golden import REF                          # noqa: E402  (DEEPSOLID_REFERENCE)
from tools.make_pretrain_golden import save_npz_deterministic   # noqa: E402

SIZES = [(2, 3), (33, 8), (65, 32)]
DAMPINGS = [1e-3, 1e-1]


def spd(rng, n):
    """Q^T D Q with eigenvalues spread over [1e-3, 1]."""
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    d = np.exp(rng.uniform(np.log(1e-3), 0.0, size=n))
    a = (q.T * d) @ q
    return (a + a.T) / 2


def load_reference_utils():
    import torch
    jax = standin.install(REF)
    lax = sys.modules['jax.lax']
    lax.cond = lambda pred, true_fun, false_fun, operand=None: true_fun(operand) if bool(pred) else false_fun(operand)
    jsl = types.ModuleType('jax.scipy.linalg')
    jsl.solve = lambda a, b, sym_pos=False: torch.linalg.solve(torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64))
    jsp = types.ModuleType('jax.scipy')
    jsp.linalg = jsl
    tu = types.ModuleType('jax.tree_util')
    tu.register_pytree_node = lambda *a, **k: None
    jax.scipy, jax.tree_util = jsp, tu
    jax.local_device_count = lambda: 1
    sys.modules.update({'jax.scipy': jsp, 'jax.scipy.linalg': jsl, 'jax.tree_util': tu})
    path = os.path.join(REF, 'DeepSolid', 'utils', 'kfac_ferminet_alpha', 'utils.py')
    spec = importlib.util.spec_from_file_location('reference_kfac_utils', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import torch
    ru = load_reference_utils()
    rng = np.random.default_rng(20261018)
    cases = [(f'spd_{a}_{b}', spd(rng, a), spd(rng, b)) for a, b in SIZES]
    cases.append(('zero_5_4', np.zeros((5, 5)), spd(rng, 4)))
    out, names = {}, []
    for name, f0, f1 in cases:
        for damping in DAMPINGS:
            key = f'{name}_d{damping:g}'
            names.append(key)
            t0, t1 = torch.as_tensor(f0), torch.as_tensor(f1)
            i0, i1 = ru.pi_adjusted_inverse(t0, t1, torch.as_tensor(damping, dtype=torch.float64), 'no_such_axis')
            out[f'{key}:factor_0'], out[f'{key}:factor_1'] = f0, f1
            out[f'{key}:damping'] = np.float64(damping)
            out[f'{key}:inverse_0'], out[f'{key}:inverse_1'] = np.asarray(i0, dtype=np.float64), np.asarray(i1, dtype=np.float64)
            if f0.any():
                out[f'{key}:chol_damping'] = np.float64(damping)
                out[f'{key}:chol_inverse'] = np.asarray(ru.psd_inv_cholesky(t0, torch.as_tensor(damping, dtype=torch.float64)), dtype=np.float64)
    out['cases'] = np.array(names)
    path = os.path.join(REPO, 'tests', 'golden', 'kfac_inverse.npz')
    save_npz_deterministic(path, out)
    print(path, os.path.getsize(path), 'bytes,', len(names), 'cases')


if __name__ == '__main__':
    main()
