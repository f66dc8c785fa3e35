"""Shared by test_dmc_ecp_cpu.py and test_gpu_dmc_ecp.py: DMC with a semi-local pseudopotential in the locality approximation
(`ds_dmc_step_ecp`, include/deepsolid_hip.h) -- the potentials of the tests on the fixture cells, and the numpy model: `DmcOracle`
(dmc_helpers) with E_loc + Re E_nl from the model of ecp_helpers added to E_L, and `run_model`'s bookkeeping with the rotation
counters philox_offset (initialisation) and philox_offset + 1 + i (step i)."""
import functools

import numpy as np

import dmc_helpers as dh
import ecp_helpers as eh
import sampler_helpers as sh

NAME = 'lih'                       # the default case: 4 electrons, 3-5 pairs per fixture walker at r_cut 2.18
R_CUT = eh.CASES[NAME][0]          # (every case's non-local cutoff is ecp_helpers.CASES[name][0])
KEYS7 = ('x', 'logabs', 'phase', 'drift', 'eloc', 'weight', 'epp')


def cell(name=NAME):
    return sh.case(name)[1]


@functools.lru_cache(maxsize=None)
def potential(name=NAME, n_quad=12):
    """The synthetic potential of ecp_helpers on the cell of case `name`, with that case's cutoff."""
    return eh.make_ecp(cell(name), eh.CASES[name][0], n_quad)


@functools.lru_cache(maxsize=None)
def zero_potential():
    """The same species with every coefficient 0 and the cutoffs given explicitly: pairs exist, every term is 0."""
    from deepsolid_amd.pseudopotential import SemiLocalECP
    c = cell()
    zero = lambda t: [(n, z, 0.0) for n, z, _ in t]
    species = [dict(local=zero(s['local']), channels=[zero(t) for t in s['channels']], r_cut_loc=eh.LOCAL_FRACTION * R_CUT, r_cut_nl=R_CUT)
               for s in (eh.SPECIES_A, eh.SPECIES_B)]
    n_atoms = np.asarray(c.atom_coords()).reshape(-1, 3).shape[0]
    return SemiLocalECP(c, species, [I % 2 for I in range(n_atoms)], n_quad=12)


# ------------------------------------------------------------------------------------------------------------------- the model
class DmcEcpOracle(dh.DmcOracle):
    """`DmcOracle` whose E_L carries the pseudopotential: evaluate(x, counter) adds E_loc + Re E_nl of the model of ecp_helpers with
    the rotations of (seed, counter) and returns the triple and what its tolerances scale with beside the five arrays."""

    def __init__(self, name, ecp, seed):
        super().__init__(name)
        self.ecp, self.seed, self.r_cut = ecp, seed, eh.CASES[name][0]
        self._ecp_cache = {}

    def evaluate(self, x, counter=None):
        base = super().evaluate(x)
        if counter is None:
            return base
        x = np.asarray(x, dtype=np.float64)
        key = (x.tobytes(), int(counter))
        if key not in self._ecp_cache:
            self._ecp_cache[key] = self._with_ecp(base, x, int(counter))
        return self._ecp_cache[key]

    def _with_ecp(self, base, x, counter):
        la, ph, dr, el, kr = base
        B, nq, ecp = len(x), self.ecp.n_quad, self.ecp
        ok = np.isfinite(x).all(1)
        rot = eh.replay_rotations(self.seed, counter, B)
        xs = np.where(ok[:, None], x, 0.0)                               # (a walker with a NaN coordinate has no pair and NaN energies)
        pl = eh.pair_list(ecp, x)
        xd = eh.displaced(xs, pl, rot, nq)
        q = eh.oracle_ratios(self.o, xs, xd, np.repeat(pl['w'], nq))
        Wn = eh.weights(ecp, pl, rot, nq)
        e_nl, scale = eh.energy(q, Wn, pl, B, nq)
        e_loc, mag, cnt = eh.local_energy(ecp, xs)
        r = eh.min_image(xs, ecp.atoms, ecp.a)[0][ok]
        cut = min(float(np.abs(r - rc).min()) for rc in (self.r_cut, eh.LOCAL_FRACTION * self.r_cut)) if ok.any() else np.inf
        bad = ~ok
        e_loc[bad], e_nl[bad] = np.nan, np.nan
        with np.errstate(invalid='ignore'):
            total = (el + e_loc) + e_nl.real
        epp = np.stack([e_loc, e_nl.real, e_nl.imag], axis=1)
        return la, ph, dr, total, kr, epp, dict(e_nl_scale=scale, e_loc_bound=(8 + cnt) * eh.EPS * mag, pairs=int(pl['counts'].sum()),
                                                cutoff_distance=cut)


def run_model(orc, x0, weight0, steps, tau, tau_eff, e_trial, e_ref, e_cut, branch_every, seed, offset):
    """`dmc_helpers.run_model` (fixed phase) with the pseudopotential in E_L and epp carried through selection and comb.  Beside its
    entries: state['epp'], per step epp_prop, aux (the tolerance scales of the proposal), ecp_row (3,), pairs; aux0 and pairs0 of
    the initialisation."""
    cell_, N = orc.cell, orc.n
    B = len(x0)
    x = np.array(x0, dtype=np.float64)
    w = np.array(weight0, dtype=np.float64)
    la, ph, dr, el, kr, epp, aux0 = orc.evaluate(x, offset)
    la, ph, dr, el, kr, epp = (np.array(v) for v in (la, ph, dr, el, kr, epp))
    w[~(np.isfinite(la) & np.isfinite(el))] = 0.0
    state0 = dict(x=x.copy(), logabs=la.copy(), phase=ph.copy(), drift=dr.copy(), eloc=el.copy(), weight=w.copy(), ke=kr.copy(),
                  epp=epp.copy())
    nz_all, un_all = sh.noise(seed, offset, steps, B, N)
    xi_all = np.array([sh.uniform(seed, offset, i, np.uint64(B)) for i in range(steps)], dtype=np.float64).reshape(steps)
    tol_el = dh_eloc_tolerance(kr, aux0)
    out = []
    for i in range(steps):
        chi, u = nz_all[i], un_all[i]
        vb = dh.limited(dr, tau)
        xp = dh.wrap(cell_, x + tau * vb + np.sqrt(tau) * chi)
        la2, ph2, dr2, el2, kr2, epp2, aux = orc.evaluate(xp, offset + 1 + i)
        tol2 = dh_eloc_tolerance(kr2, aux)
        vb2 = dh.limited(dr2, tau)
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            A = 2.0 * (la2 - la) + 0.5 * ((chi ** 2).sum(1) - ((chi + np.sqrt(tau) * (vb + vb2)) ** 2).sum(1))
            logu = np.log(u)
            finite = np.isfinite(A) & np.isfinite(el2)
            acc = finite & (A > logu)
            p = np.where(finite, np.minimum(1.0, np.exp(np.where(finite, A, 0.0))), 0.0)
            e_new = np.where(acc, el2, el)
            tol_new = np.where(acc, tol2, tol_el)
            cn, co = dh.clip(e_new, e_ref, e_cut), dh.clip(el, e_ref, e_cut)
            wn = w * np.exp(-tau_eff * (0.5 * (cn + co) - e_trial))
            # distance of every energy that is clipped from the two clip edges, in units of its tolerance
            edge = np.inf
            if e_cut > 0:
                for e, t in ((e_new, tol_new), (el, tol_el)):
                    d = np.minimum(np.abs(e - (e_ref + e_cut)), np.abs(e - (e_ref - e_cut))) / t
                    edge = min(edge, float(np.nanmin(d)))
        w = np.where(np.isfinite(wn), wn, 0.0)
        clipped = np.isfinite(e_new) & (cn != e_new)
        sel = acc[:, None]
        x_prev = x.copy()
        x, dr, epp = np.where(sel, xp, x), np.where(sel, dr2, dr), np.where(sel, epp2, epp)
        la, ph, el, kr = np.where(acc, la2, la), np.where(acc, ph2, ph), np.where(acc, el2, el), np.where(acc, kr2, kr)
        tol_el = tol_new
        live = w != 0.0
        row = np.array([w.sum(), (w[live] * el[live]).sum(), (w[live] * el[live] ** 2).sum(), acc.sum(), p.sum(), clipped.sum(),
                        (~finite).sum(), (w ** 2).sum(), B], dtype=np.float64)
        ecp_row = (w[live, None] * epp[live]).sum(0)
        ecp_tol = (w[live] * tol_el[live]).sum()
        cb, parents = None, np.arange(B)
        if branch_every > 0 and (i + 1) % branch_every == 0:
            cb = dh.comb(w, xi_all[i])
            parents = cb['parents']
            if cb['run']:
                x, dr, la, ph, el, kr, epp, tol_el = (v[parents] for v in (x, dr, la, ph, el, kr, epp, tol_el))
                w = np.full(B, cb['step'])
                row[8] = len(np.unique(parents))
            else:
                row[8] = 0
        out.append(dict(acc=acc, A=A, logu=logu, margin=A - logu, p=p, nonfinite=~finite, node=np.zeros(B, bool), clipped=clipped,
                        parents=parents, comb=cb, row=row, ecp_row=ecp_row, ecp_tol=ecp_tol, x_prev=x_prev, x_prop=xp, e_prop=el2,
                        epp_prop=epp2, aux=aux, pairs=aux['pairs'], crossings=0, w_after=w.copy(), xi=xi_all[i], chi=chi, u=u,
                        edge=edge, tol_prop=tol2, ke_max=float(np.nanmax(np.abs(np.concatenate([kr, kr2]))))))
    state = dict(x=x, logabs=la, phase=ph, drift=dr, eloc=el, weight=w, ke=kr, epp=epp, tol_eloc=tol_el)
    return dict(state=state, state0=state0, steps=out, aux0=aux0, pairs0=aux0['pairs'], normals=nz_all, uniforms=un_all,
                comb_uniforms=xi_all)


def tol_q():
    """The float64 tolerance on a ratio that test_gpu_ecp.py takes from test_gpu_onebody.py."""
    from test_gpu_onebody import TOL_Q
    return TOL_Q


def dh_eloc_tolerance(ke, aux):
    """Per walker, the tolerance on E_L with a pseudopotential: what test_gpu_dmc.eloc_bound allows on Re ke + ewald, plus the
    per-walker E_nl tolerance of test_gpu_ecp.check_against_reference (the same constant times e_nl_scale), plus the E_loc bound."""
    with np.errstate(invalid='ignore'):
        return (1e-8 * np.maximum(1.0, np.abs(ke)) + 1e-9) + tol_q() * aux['e_nl_scale'] + aux['e_loc_bound']


# case -> (B, tau, steps, seed): the replays of the GPU suite.  The seeds are from tools/find_dmc_ecp_seeds.py (oracle only); the
# comments are what they gave.  lih is a real wavefunction (Im E_nl = 0 to rounding); the two others have a complex one.
REPLAYS = {
    'lih': (12, 0.1, 2, 1),
    # 21 accepted, 3 rejected, 2 duplicated, min |A - log u| 7.4e-2, cutoff distance 7.6e-3, max |Im E_nl| 3.5
    'lih_twist': (12, 0.1, 2, 1),
    # 7 accepted, 5 rejected, 2 duplicated, min |A - log u| 0.23, cutoff distance 3.0e-3, max |Im E_nl| 11.3
    'bcc_li': (6, 0.05, 2, 1),
}


@functools.lru_cache(maxsize=None)
def replay_reference(name=NAME, seed=None):
    """The model's run of the replay of case `name` from state_valid = 0, comb every step, Philox offset 0; e_ref, e_trial and e_cut
    as dmc_helpers.replay_reference chooses them, from the energies with the pseudopotential."""
    B, tau, steps, sd = REPLAYS[name]
    sd = sd if seed is None else seed
    ecp = potential(name)
    orc = DmcEcpOracle(name, ecp, sd)
    x0 = dh.start_walkers(name, B, sd)
    el0 = orc.evaluate(x0, 0)[3]
    e_ref = float(np.round(np.mean(el0), 3))
    e_cut = 0.05 * np.sqrt(orc.n / tau)
    w0 = dh.preset_weights('ramp', B)
    r = run_model(orc, x0, w0, steps, tau, tau, e_ref, e_ref, e_cut, 1, sd, 0)
    r['tau_eff'] = tau
    r.update(x0=x0, w0=w0, e_ref=e_ref, e_cut=e_cut, tau=tau, seed=sd, B=B, ecp=ecp, name=name, cond=conditions(r, name))
    return r


def conditions(r, name=NAME):
    """`dmc_helpers.conditions` plus: the smallest distance of any visited position's pair from a cutoff of case `name`, the smallest
    distance of a clipped-or-not decision from a clip edge in units of the energy tolerance, the weight tolerance with the
    pseudopotential's share of the energy tolerance, and the largest |Im E_nl| over the start walkers and the proposals."""
    c = dh.conditions(r)
    st = r['steps']
    c['name'], c['r_cut'] = name, eh.CASES[name][0]
    c['im_e_nl'] = float(max(np.nanmax(np.abs(e[:, 2])) for e in [r['state0']['epp']] + [s['epp_prop'] for s in st]))
    c['cutoff_distance'] = min([r['aux0']['cutoff_distance']] + [s['aux']['cutoff_distance'] for s in st])
    c['edge'] = min(s['edge'] for s in st)
    tol_e = max(float(np.nanmax(s['tol_prop'])) for s in st)
    c['tol_w'] = r.get('tau_eff', 0.0) * len(st) * tol_e
    return c


def assert_conditions(c):
    assert c['undecidable'] == 0 and c['min_margin'] > dh.TOL_A, c
    assert c['min_tooth'] > c['tol_w'], c
    assert c['cutoff_distance'] > eh.CUTOFF_MARGIN, c
    assert c['edge'] > 1.0, c
    for k in ('accepted', 'rejected', 'duplicated'):
        assert c[k] >= 1, (k, c)
