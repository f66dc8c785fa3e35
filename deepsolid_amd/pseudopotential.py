"""Semi-local pseudopotentials (effective core potentials): the host-side tables of `ds_ecp_energy` (csrc/ds_ecp.h, DESIGN.md
section 18).  The reference has no pseudopotentials; the conventions are this project's own and stated in include/deepsolid_hip.h.

A species is a local radial function `v_loc` (WITHOUT the -Z_eff / r tail, which Ewald carries) and `n_l` non-local channels `v_l`,
each  v(r) = sum_k c_k r^(n_k - 2) exp(-zeta_k r^2),  n_k in 0..4, at most 16 terms: the Gaussian expansion in which ccECP, BFD and
Stuttgart potentials are published.  Inside its cutoff a function is used as it is, outside it is exactly 0.

This module is numpy only: building, checking, saving and loading a potential needs no GPU.  `deepsolid_amd.device.EcpTables`
puts it on the device, `DeviceSystem.ecp_energy` evaluates it.
"""
import numpy as np

MAX_TERMS = 16
SLOTS = 5                     # radial functions per species in the tables: v_loc, then v_l for l = 0..3
RULE_DEGREE = {6: 3, 12: 5}
CUTOFF_GRID = 1e-3            # Bohr: the grid of the cutoff search ...
CUTOFF_MAX = 10.0             # ... and where it ends


def quadrature_points(n_quad):
    """The unrotated points u_q (n_quad, 3) of the equal-weight rule: the octahedron +x, -x, +y, -y, +z, -z (exact to degree 3) or
    the icosahedron (exact to degree 5): with phi = (1 + sqrt 5) / 2 and n = sqrt(1 + phi^2), for (s1, s2) in the order (+,+), (+,-),
    (-,+), (-,-) all four of (0, s1, s2 phi) / n, then all four of (s1, s2 phi, 0) / n, then all four of (s2 phi, 0, s1) / n."""
    if n_quad == 6:
        return np.asarray([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    if n_quad == 12:
        phi = (1.0 + np.sqrt(5.0)) / 2.0
        n = np.sqrt(1.0 + phi * phi)
        signs = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
        pts = [(0.0, s1, s2 * phi) for s1, s2 in signs] + [(s1, s2 * phi, 0.0) for s1, s2 in signs] + \
              [(s2 * phi, 0.0, s1) for s1, s2 in signs]
        return np.asarray(pts, dtype=np.float64) / n
    raise ValueError(f'n_quad must be 6 or 12 (got {n_quad})')


def cell_heights(a):
    """Heights of the cell with lattice vectors in the rows of `a`: height c = 1 / ||column c of inv(a)||."""
    return 1.0 / np.linalg.norm(np.linalg.inv(np.asarray(a, dtype=np.float64).reshape(3, 3)), axis=0)


def eval_radial(terms, r):
    """v(r) of a term table [(n, zeta, c), ...] at r (any shape), the terms added in table order."""
    r = np.asarray(r, dtype=np.float64)
    r2 = r * r
    v = np.zeros_like(r)
    with np.errstate(divide='ignore', invalid='ignore'):
        for n, z, c in terms:
            pw = (1.0 / r2, 1.0 / r, np.ones_like(r), r, r2)[int(n)]
            v = v + (c * pw) * np.exp(-(z * r2))
    return v


def find_cutoff(terms, tol=1e-5):
    """The smallest radius on the 1e-3-Bohr grid up to 10 Bohr beyond which |v| <= tol everywhere on the grid (0.0 for a function that
    never exceeds tol).  Raises if |v| > tol at 10 Bohr: such a function has no cutoff."""
    if not len(terms):
        return 0.0
    grid = CUTOFF_GRID * np.arange(1, int(round(CUTOFF_MAX / CUTOFF_GRID)) + 1)
    above = np.nonzero(~(np.abs(eval_radial(terms, grid)) <= tol))[0]
    if not len(above):
        return 0.0
    if above[-1] == len(grid) - 1:
        raise ValueError(f'the radial function still exceeds {tol} Ha at {CUTOFF_MAX} Bohr: no cutoff')
    return float(grid[above[-1] + 1])


def _terms(t, what):
    """A term table from [(n, zeta, c), ...], a dict(n=, zeta=, c=) or an (K, 3) array -> list of (int, float, float), checked."""
    if t is None:
        return []
    if isinstance(t, dict):
        t = list(zip(t['n'], t['zeta'], t['c']))
    arr = np.asarray(t, dtype=np.float64).reshape(-1, 3) if len(t) else np.zeros((0, 3))
    if len(arr) > MAX_TERMS:
        raise ValueError(f'{what} has {len(arr)} terms; at most {MAX_TERMS} terms are provided')
    out = []
    for k, (n, z, c) in enumerate(arr):
        if n != int(n) or not 0 <= int(n) <= 4:
            raise ValueError(f'{what}, term {k} has n_k = {n}; n_k must be in 0..4')
        if not (np.isfinite(z) and np.isfinite(c)):
            raise ValueError(f'{what}, term {k} is not finite')
        out.append((int(n), float(z), float(c)))
    return out


class SemiLocalECP:
    """The pseudopotential of one simulation cell.

    species: a list (or a dict name -> entry; `atom_species` then holds names) of dicts with the keys
        'local':    term table of v_loc, [(n, zeta, c), ...] / dict(n=, zeta=, c=) / (K, 3) array (may be empty),
        'channels': list of the term tables of v_0, v_1, ... (n_l = its length, at most 3 with n_quad = 12 and 2 with n_quad = 6),
        'r_cut_loc', 'r_cut_nl': optional cutoffs in Bohr; a missing one is found by `find_cutoff(.., tol)` (r_cut_nl: the largest
                    over the channels),
        'z_eff':    optional, informational.
    atom_species: the species of every atom of the SIMULATION cell, in the order of `simulation_cell.atom_coords()`.
    z_eff: optional (n_atoms,) effective charges, checked against `simulation_cell.atom_charges()`.
    Every cutoff must be at most half the smallest height of the simulation cell (`cell_heights`)."""

    def __init__(self, simulation_cell, species, atom_species, n_quad=12, tol=1e-5, z_eff=None):
        if n_quad not in RULE_DEGREE:
            raise ValueError(f'n_quad must be 6 or 12 (got {n_quad})')
        self.n_quad = int(n_quad)
        self.tol = float(tol)
        self.a = np.ascontiguousarray(np.asarray(simulation_cell.a, dtype=np.float64).reshape(3, 3))
        self.atoms = np.ascontiguousarray(np.asarray(simulation_cell.atom_coords(), dtype=np.float64).reshape(-1, 3))
        if isinstance(species, dict):
            names = list(species)
            species = [species[k] for k in names]
            atom_species = [names.index(k) for k in atom_species]
        self.atom_species = np.ascontiguousarray(np.asarray(atom_species, dtype=np.int32).reshape(-1))
        if len(self.atom_species) != len(self.atoms):
            raise ValueError(f'atom_species names {len(self.atom_species)} atoms, the simulation cell has {len(self.atoms)}')
        if len(species) < 1 or self.atom_species.min() < 0 or self.atom_species.max() >= len(species):
            raise ValueError('atom_species must index the species')
        if z_eff is not None:
            z_eff = np.asarray(z_eff, dtype=np.float64).reshape(-1)
            charges = np.asarray(simulation_cell.atom_charges(), dtype=np.float64).reshape(-1)
            if z_eff.shape != charges.shape or np.any(z_eff != charges):
                raise ValueError(f'z_eff {z_eff.tolist()} differs from the charges of the simulation cell {charges.tolist()}: the cell '
                                 'must be built with the valence electron count and Z_eff')
        self.local, self.channels = [], []
        cut_loc, cut_nl = [], []
        for s, sp in enumerate(species):
            loc = _terms(sp.get('local'), f'species {s}, v_loc')
            ch = [_terms(t, f'species {s}, v_{l}') for l, t in enumerate(sp.get('channels', ()))]
            if len(ch) > 4:
                raise ValueError(f'species {s} has n_l = {len(ch)}; n_l must be in 0..4')
            if len(ch) == 4:
                raise ValueError(f'species {s} has n_l = 4: an l = 3 channel needs a quadrature rule of degree >= 6, which is not provided')
            if 2 * (len(ch) - 1) > RULE_DEGREE[self.n_quad]:
                raise ValueError(f'species {s} has n_l = {len(ch)}: channels up to l = {len(ch) - 1} need a rule of degree '
                                 f'{2 * (len(ch) - 1)}, n_quad = {self.n_quad} is exact to degree {RULE_DEGREE[self.n_quad]}')
            self.local.append(loc)
            self.channels.append(ch)
            rl = sp.get('r_cut_loc')
            rn = sp.get('r_cut_nl')
            cut_loc.append(find_cutoff(loc, self.tol) if rl is None else float(rl))
            cut_nl.append((max([find_cutoff(t, self.tol) for t in ch]) if ch else 0.0) if rn is None else float(rn))
        self.r_cut_loc = np.asarray(cut_loc, dtype=np.float64)
        self.r_cut_nl = np.asarray(cut_nl, dtype=np.float64)
        if np.any(~np.isfinite(self.r_cut_loc)) or np.any(~np.isfinite(self.r_cut_nl)) or np.any(self.r_cut_loc < 0) or \
                np.any(self.r_cut_nl < 0):
            raise ValueError('a cutoff is negative or not finite')
        limit = 0.5 * float(cell_heights(self.a).min())
        for i, s in enumerate(self.atom_species):
            rc = max(self.r_cut_loc[s], self.r_cut_nl[s] if self.channels[s] else 0.0)
            if rc > limit:
                raise ValueError(f'atom {i} (species {s}) has the cutoff {rc:.6f} Bohr; the limit is {limit:.6f} Bohr, half the '
                                 'smallest height of the simulation cell')

    # ------------------------------------------------------------------ what the library reads
    @property
    def n_species(self):
        return len(self.local)

    @property
    def n_l(self):
        return np.asarray([len(c) for c in self.channels], dtype=np.int32)

    def tables(self):
        """-> dict of the flat arrays of `ds_ecp_desc`: term_offset (5 n_species + 1,), term_n, term_zeta, term_c."""
        off, n, z, c = [0], [], [], []
        for s in range(self.n_species):
            slots = [self.local[s]] + self.channels[s] + [[]] * (SLOTS - 1 - len(self.channels[s]))
            for t in slots:
                for tn, tz, tc in t:
                    n.append(tn), z.append(tz), c.append(tc)
                off.append(len(n))
        return dict(term_offset=np.asarray(off, dtype=np.int32), term_n=np.asarray(n, dtype=np.int32),
                    term_zeta=np.asarray(z, dtype=np.float64), term_c=np.asarray(c, dtype=np.float64))

    def radial(self, species, channel, r):
        """v(r) of `species`: channel 'loc' (or -1) is v_loc, channel l >= 0 is v_l.  The cutoff is NOT applied."""
        t = self.local[species] if channel in ('loc', -1) else self.channels[species][int(channel)]
        return eval_radial(t, r)

    # ------------------------------------------------------------------ one .npz
    def save(self, path):
        np.savez(path, a=self.a, atoms=self.atoms, atom_species=self.atom_species, n_l=self.n_l, r_cut_loc=self.r_cut_loc,
                 r_cut_nl=self.r_cut_nl, n_quad=np.int32(self.n_quad), tol=np.float64(self.tol), **self.tables())

    @classmethod
    def load(cls, path, simulation_cell=None):
        """The potential saved by `save`.  With `simulation_cell` its cell and atoms are checked against the file's."""
        with np.load(path) as f:
            d = {k: f[k] for k in f.files}
        self = cls.__new__(cls)
        self.a, self.atoms, self.atom_species = d['a'], d['atoms'], d['atom_species'].astype(np.int32)
        self.r_cut_loc, self.r_cut_nl = d['r_cut_loc'], d['r_cut_nl']
        self.n_quad, self.tol = int(d['n_quad']), float(d['tol'])
        off = d['term_offset']
        rows = list(zip(d['term_n'].tolist(), d['term_zeta'].tolist(), d['term_c'].tolist()))
        self.local, self.channels = [], []
        for s, nl in enumerate(d['n_l'].tolist()):
            slot = lambda j: rows[off[SLOTS * s + j]:off[SLOTS * s + j + 1]]
            self.local.append(slot(0))
            self.channels.append([slot(1 + l) for l in range(nl)])
        if simulation_cell is not None:
            a = np.asarray(simulation_cell.a, dtype=np.float64).reshape(3, 3)
            atoms = np.asarray(simulation_cell.atom_coords(), dtype=np.float64).reshape(-1, 3)
            if a.shape != self.a.shape or atoms.shape != self.atoms.shape or not (np.allclose(a, self.a, rtol=0, atol=1e-10) and
                                                                                np.allclose(atoms, self.atoms, rtol=0, atol=1e-10)):
                raise ValueError(f'{path} was saved for another simulation cell')
        return self
