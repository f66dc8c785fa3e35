#!/usr/bin/env python3
"""Generate tests/golden/estimators.npz by EXECUTING the reference's estimator.py.

Runs only in the build container (needs the reference tree, which does not exist on the GPU box).  JAX and PySCF are not
installable here, so DeepSolid/estimator.py and DeepSolid/constants.py are imported under the stand-ins of
tools/make_golden.py, reduced to what these two files touch:

  * ``jax.numpy``  -> numpy (``meshgrid`` indexes 'xy' by default in both)
  * ``jax.pmap``   -> identity; ``jax.lax.pmean`` -> identity; ``jax.core.axis_frame`` raises NameError, so
    ``constants.pmean_if_pmap`` is the identity as it is outside a pmap
  * ``pyscf.pbc.gto`` -> empty module (estimator.py imports it at the top level for a type annotation)
  * cells are an attribute bag with ``reciprocal_vectors()`` and ``nelectron``

Every other file under tests/golden is left untouched.  The archive is written with fixed zip timestamps, so re-running this
script reproduces it bit for bit.

Contents, per cell c in CELLS:  c_x (B, 3N) float64 walkers, c_a (3, 3) lattice, c_nelec, c_pol<d> (complex128, directions
0..2: the batch mean of the polarization) and c_sk<nq> (nq^3 float64, S(k) for nq = 1..8).
"""
import os
import sys
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
REF = os.environ.get('DEEPSOLID_REFERENCE', '/root/reference')
OUT = os.path.join(REPO, 'tests', 'golden', 'estimators.npz')

BATCH = 48
NQS = tuple(range(1, 9))
DIRECTIONS = (0, 1, 2)


def install_standins():
    jax = types.ModuleType('jax')
    lax = types.ModuleType('jax.lax')
    core = types.ModuleType('jax.core')
    rnd = types.ModuleType('jax.random')
    lax.pmean = lambda x, axis_name=None: x
    lax.psum = lambda x, axis_name=None: x

    def axis_frame(name):
        raise NameError(name)
    core.axis_frame = axis_frame
    jax.numpy, jax.lax, jax.core, jax.random = np, lax, core, rnd
    jax.pmap = lambda f, **kw: f
    sys.modules.update({'jax': jax, 'jax.numpy': np, 'jax.lax': lax, 'jax.core': core, 'jax.random': rnd})
    for m in ('pyscf', 'pyscf.pbc', 'pyscf.pbc.gto'):
        sys.modules[m] = types.ModuleType(m)
    sys.modules['pyscf'].pbc = sys.modules['pyscf.pbc']
    sys.modules['pyscf.pbc'].gto = sys.modules['pyscf.pbc.gto']
    sys.modules['pyscf.pbc.gto'].Cell = object
    sys.path.insert(0, REF)


class RefCell:
    """What estimator.py reads of a pyscf.pbc.gto.Cell."""
    def __init__(self, a, nelectron):
        self.a = np.asarray(a, dtype=np.float64)
        self.nelectron = int(nelectron)

    def reciprocal_vectors(self):
        return 2 * np.pi * np.linalg.inv(self.a).T


def hydrogen_chain(n=8, L=1.8):
    """config/hydrogen_chain.py:15-45 with 'H,<n>,1,1,<L>,...': one H at (L/2, 0, 0) in an L x 100 x 100 cell, tiled n times
    along x; closed shell (n/2, n/2)."""
    from deepsolid_amd.cell import Cell
    from deepsolid_amd.supercell import get_supercell
    prim = Cell(np.diag([L, 100.0, 100.0]), [('H', [L / 2, 0.0, 0.0])], spin=1)
    return get_supercell(prim, np.diag([n, 1, 1]), nelec=(n // 2, n // 2))


def cells():
    from deepsolid_amd import systems
    return {
        'lih': systems.lih_rocksalt(),          # fcc: non-orthogonal simulation cell, 4 e-
        'bcc_li': systems.bcc_li(),             # 2x2x2 bcc Li, 24 e-
        'graphene': systems.graphene(),         # hexagonal 2x2x1, 48 e-
        'h_chain': hydrogen_chain(),            # 1-D chain, 8 e-
    }


def walkers(cell, batch, seed):
    """Fractional coordinates in [-0.5, 1.5): walkers inside and outside the cell."""
    rng = np.random.default_rng(seed)
    n = cell.nelec[0] + cell.nelec[1]
    return ((rng.uniform(size=(batch, n, 3)) * 2.0 - 0.5) @ cell.a).reshape(batch, 3 * n)


def write_npz(path, arrays):
    """np.savez with a fixed entry timestamp (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, 'w') as f:
                np.lib.format.write_array(f, np.asarray(arrays[name]), allow_pickle=False)


def main():
    install_standins()
    from DeepSolid import estimator
    out = {}
    for i, (name, cell) in enumerate(cells().items()):
        x = walkers(cell, BATCH, 2024 + i)
        ref_cell = RefCell(cell.a, cell.nelectron)
        out[f'{name}_x'] = x
        out[f'{name}_a'] = cell.a
        out[f'{name}_nelec'] = np.asarray(cell.nelec, dtype=np.int64)
        for d in DIRECTIONS:
            out[f'{name}_pol{d}'] = np.asarray(estimator.make_complex_polarization(ref_cell, direction=d)(x), dtype=np.complex128)
        for nq in NQS:
            out[f'{name}_sk{nq}'] = np.asarray(estimator.make_structure_factor(ref_cell, nq=nq)(x), dtype=np.float64)
        print(f'{name}: N = {cell.nelectron}, B = {BATCH}, P0 = {complex(out[name + "_pol0"]):.6f}, '
              f'S(k) nq=4 mean = {out[name + "_sk4"].mean():.6f}')
    write_npz(OUT, out)
    print(f'wrote {OUT} ({os.path.getsize(OUT)} bytes)')


if __name__ == '__main__':
    main()
