"""Shared by test_dmc_tmove_cpu.py and test_gpu_dmc_tmove.py: DMC with a semi-local pseudopotential and Casula's T-moves
(`ds_dmc_step_tmove`, the algorithm as include/deepsolid_hip.h states it) in plain numpy -- `heat_bath`, the choice of step 6 with
sequential float64 additions (bit for bit what k_ecp_tmove forms from the same terms); `quadrature_point`, where the chosen
electron goes; `tree_row4`, the four columns of out_ecp_stats in the device's order; and `run_model`, the new order of the step
(decide, evaluate the pseudopotential where the walker stands, commit with the one-point weight, T-move, second chain pass) on
the oracle of dmc_ecp_helpers."""
import functools

import numpy as np

import dmc_ecp_helpers as deh
import dmc_helpers as dh
import dmc_parts_helpers as ph
import ecp_helpers as eh
import sampler_helpers as sh

NAME = deh.NAME
KEYS7 = deh.KEYS7


# --------------------------------------------------------------------------------------------------------------- the heat bath
def intervals(terms, tau):
    """t_c = -tau min(Re term_c, 0) and r_c = r_{c-1} + t_c from r_{-1} = 1, each addition one rounded float64 addition in
    configuration order -> (t (n,), r (n + 1,) with r[0] = r_{-1} = 1 and r[c + 1] = r_c)."""
    re = np.asarray(terms).real.astype(np.float64).reshape(-1)
    t = -np.float64(tau) * np.minimum(re, 0.0)
    r = np.empty(len(re) + 1)
    acc = np.float64(1.0)
    r[0] = acc
    for c in range(len(re)):
        acc = acc + t[c]
        r[c + 1] = acc
    return t, r


def heat_bath(terms, tau, u):
    """Step 6 on the terms (W / N_q) q of ONE walker (complex or real, (pair, q) order): theta = u Z; theta < 1 stays (-1);
    otherwise the number of c with r_c <= theta, clamped to the last c with t_c > 0.  -> the configuration, or -1."""
    t, r = intervals(terms, tau)
    if len(t) == 0:
        return -1
    theta = np.float64(u) * r[-1]
    pos = np.nonzero(t > 0.0)[0]
    if theta < 1.0 or len(pos) == 0:
        return -1
    return int(min(int((r[1:] <= theta).sum()), pos[-1]))


def midpoint(terms, tau, c):
    """A uniform u for which theta = u Z lies at the middle of configuration c's interval [r_{c-1}, r_c) (c = -1: of [0, 1), the
    interval of no move), and the half width of that interval in units of theta."""
    t, r = intervals(terms, tau)
    lo, hi = (0.0, 1.0) if c < 0 else (r[c], r[c + 1])
    return 0.5 * (lo + hi) / r[-1], 0.5 * (hi - lo)


def wrap_row(cell, p, dtype=np.float64):
    """The wrap of k_dmc_propose (dmc_parts_helpers.proposal) on points p (..., 3), formed in `dtype`."""
    a64 = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    a, ainv = a64.astype(dtype), np.linalg.inv(a64).astype(dtype)
    f = np.asarray(p, dtype=dtype) @ ainv
    return ((f - np.floor(f)) @ a).astype(np.float64)


def quadrature_point(cell, xe, r, dhat, U, dtype=np.float64):
    """wrap((r_i - r dhat) + r U_q): the arithmetic of k_ecp_propose in float64, rounded to `dtype`, then wrapped in `dtype`."""
    p = (np.asarray(xe, dtype=np.float64) - r * np.asarray(dhat)) + r * np.asarray(U)
    return wrap_row(cell, p.astype(dtype), dtype)


def tree_row4(weight, epp, choice):
    """The out_ecp_stats row of ds_dmc_step_tmove: dmc_parts_helpers.ecp_stats_from_state and the number of walkers with a T-move."""
    return np.concatenate([ph.ecp_stats_from_state(weight, epp), [float((np.asarray(choice) >= 0).sum())]])


def one_point_weights(w, e, tau_eff, e_trial, e_ref, e_cut):
    """weight <- weight exp(-tau_eff (clip(E) - e_trial)); a result that is not finite is 0."""
    with np.errstate(invalid='ignore', over='ignore'):
        wn = np.asarray(w, dtype=np.float64) * np.exp(-tau_eff * (ph.clip(e, e_ref, e_cut)[0] - e_trial))
    return np.where(np.isfinite(wn), wn, 0.0)


def tmove_uniforms(seed, offset, steps, B):
    """What a Philox-mode call draws for the T-moves: stream 2 at index B + 1 + w, counter offset + i -> (steps, B) float64."""
    idx = np.arange(B, dtype=np.uint64) + np.uint64(B + 1)
    return np.stack([sh.uniform(seed, offset, i, idx) for i in range(steps)]).astype(np.float64)


def r_tolerance(tau, scale):
    """A-priori bound on |r_c(model) - r_c(device)| of one walker, for every c: a ratio of the device differs from the oracle's by at
    most tol_q() max(1, |q|) (what test_gpu_ecp.py holds it to), a term by |W / N_q| times that, t_c by tau times that, and r_c is
    a sum of at most n such t_c (its n roundings, n 2^-53 Z, are far below): tau tol_q() sum_c |W_c / N_q| max(1, |q_c|)."""
    return tau * deh.tol_q() * float(np.sum(scale))


def steer(terms, scales, tau, tol, kind):
    """The steered choice of one walker: `kind` 0 stays, 1 takes the first configuration with Re term < 0, 2 the last, 3 the one in
    the middle of them.  -> (target, u, skipped): u puts theta at the midpoint of the target's interval.  An interval whose half
    width is below 10 x the a-priori bound on the model-device difference of r_c is skipped (the walker then stays: u = 0).
    The bound: every term of the walker is off by at most tol |W / N_q| max(1, |q|), t_c by tau times that, and r_c adds at most n
    of them: n tau tol max_c |W_c / N_q| max(1, |q_c|), n the number of the walker's terms."""
    neg = np.nonzero(np.asarray(terms).real < 0)[0]
    if kind == 0 or len(neg) == 0:
        return -1, midpoint(terms, tau, -1)[0], False
    c = int(neg[(0, -1, len(neg) // 2)[kind - 1]])
    u, half = midpoint(terms, tau, c)
    if half < 10.0 * len(terms) * tau * tol * float(np.max(scales)):
        return -1, 0.0, True
    return c, u, False


# the steered-choice test: (case, B), the seed of dmc_helpers.start_walkers, (seed, counter) of the rotations, tau
STEER_CASES = [('lih', 37), ('lih_twist', 37), ('bcc_li', 5)]
STEER_WALKERS, STEER_ROT, STEER_TAU = 5, (11, 3), 0.1


def steer_all(terms, scales, counts, nq, tau, tol):
    """`steer` for every walker of an evaluation (terms and scales of all configurations, pair counts per walker), kind = w % 4.
    -> (targets (B,), u (B,), skipped (B,) bool)."""
    off = np.concatenate([[0], np.cumsum(counts)]) * nq
    out = [steer(terms[off[w]:off[w + 1]], scales[off[w]:off[w + 1]], tau, tol, w % 4) if off[w + 1] > off[w] else (-1, 0.0, False)
           for w in range(len(counts))]
    return np.asarray([o[0] for o in out]), np.asarray([o[1] for o in out], dtype=np.float64), np.asarray([o[2] for o in out])


@functools.lru_cache(maxsize=None)
def local_only_potential():
    """The species of ecp_helpers without non-local channels: the local part alone, no pair anywhere."""
    from deepsolid_amd.pseudopotential import SemiLocalECP
    c = deh.cell()
    species = [dict(local=s['local'], channels=[], r_cut_loc=eh.LOCAL_FRACTION * deh.R_CUT, r_cut_nl=deh.R_CUT)
               for s in (eh.SPECIES_A, eh.SPECIES_B)]
    n_atoms = np.asarray(c.atom_coords()).reshape(-1, 3).shape[0]
    return SemiLocalECP(c, species, [I % 2 for I in range(n_atoms)], n_quad=12)


# ------------------------------------------------------------------------------------------------------------------- the model
class TmoveOracle(deh.DmcEcpOracle):
    """`DmcEcpOracle` that also hands back what the T-move needs of an evaluation: per configuration the term (W / N_q) q and the
    scale |W / N_q| max(1, |q|) of its tolerance, the pair list and the rotations (aux['terms'], ['scales'], ['pl'], ['rot'])."""

    def _with_ecp(self, base, x, counter):
        out = super()._with_ecp(base, x, counter)
        B, nq = len(x), self.ecp.n_quad
        ok = np.isfinite(x).all(1)
        rot = eh.replay_rotations(self.seed, counter, B)
        xs = np.where(ok[:, None], x, 0.0)
        pl = eh.pair_list(self.ecp, x)
        q = eh.oracle_ratios(self.o, xs, eh.displaced(xs, pl, rot, nq), np.repeat(pl['w'], nq)).reshape(-1, nq)
        Wn = eh.weights(self.ecp, pl, rot, nq)
        out[-1].update(terms=(Wn * q).reshape(-1), scales=(np.abs(Wn) * np.maximum(1.0, np.abs(q))).reshape(-1), pl=pl, rot=rot)
        return out


def walker_terms(aux, w, nq):
    """-> (first pair of walker w, its terms, their scales) of an evaluation's aux."""
    off = np.concatenate([[0], np.cumsum(aux['pl']['counts'])])
    sl = slice(int(off[w]) * nq, int(off[w + 1]) * nq)
    return int(off[w]), aux['terms'][sl], aux['scales'][sl]


def run_model(orc, x0, weight0, steps, tau, tau_eff, e_trial, e_ref, e_cut, branch_every, seed, offset, tmove_u=None):
    """The algorithm of ds_dmc_step_tmove from state_valid = 0 on the oracle (fixed phase).  -> dict: state (the seven arrays, eloc =
    the chain part), state0, per step: acc, margin (A - log u), p, nonfinite, clipped, x_cur, energy (E of the commit), epp, choice
    (B,), moved (walker, electron, point), tmargin (per walker the smallest distance of theta from an interval edge and from 1,
    in units of `r_tolerance`; inf where no T-move is possible), row, ecp_row (4,), pairs, parents, comb, w_after, evaluated_in_place
    (rejected walkers with pairs), died (walkers whose weight this step took to 0)."""
    cell_, N, nq = orc.cell, orc.n, orc.ecp.n_quad
    B = len(x0)
    x = np.array(x0, dtype=np.float64)
    w = np.array(weight0, dtype=np.float64)
    la, ph_, dr, el, kr = (np.array(v) for v in orc.evaluate(x))
    w[~(np.isfinite(la) & np.isfinite(el))] = 0.0
    epp = np.zeros((B, 3))
    state0 = dict(x=x.copy(), logabs=la.copy(), phase=ph_.copy(), drift=dr.copy(), eloc=el.copy(), weight=w.copy(), epp=epp.copy())
    nz_all, un_all = sh.noise(seed, offset, steps, B, N)
    xi_all = np.array([sh.uniform(seed, offset, i, np.uint64(B)) for i in range(steps)], dtype=np.float64).reshape(steps)
    tu_all = tmove_uniforms(seed, offset, steps, B) if tmove_u is None else np.asarray(tmove_u, dtype=np.float64)
    out = []
    for i in range(steps):
        chi, u = nz_all[i], un_all[i]
        vb = dh.limited(dr, tau)
        xp = dh.wrap(cell_, x + tau * vb + np.sqrt(tau) * chi)
        la2, ph2, dr2, el2, kr2 = orc.evaluate(xp)
        vb2 = dh.limited(dr2, tau)
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            A = 2.0 * (la2 - la) + 0.5 * ((chi ** 2).sum(1) - ((chi + np.sqrt(tau) * (vb + vb2)) ** 2).sum(1))
            logu = np.log(u)
            finite = np.isfinite(A) & np.isfinite(el2)
            acc = finite & (A > logu)
            p = np.where(finite, np.minimum(1.0, np.exp(np.where(finite, A, 0.0))), 0.0)
        sel = acc[:, None]
        x_prev = x.copy()
        x, dr = np.where(sel, xp, x), np.where(sel, dr2, dr)
        la, ph_, el, kr = np.where(acc, la2, la), np.where(acc, ph2, ph_), np.where(acc, el2, el), np.where(acc, kr2, kr)
        # the pseudopotential where the walker stands
        _, _, _, total, _, epp, aux = orc.evaluate(x, offset + 1 + i)
        epp = np.array(epp)
        with np.errstate(invalid='ignore'):
            energy = (el + epp[:, 0]) + epp[:, 1]
        tol_e = deh.dh_eloc_tolerance(kr, aux)
        w_before = w.copy()
        w = one_point_weights(w, energy, tau_eff, e_trial, e_ref, e_cut)
        clipped = ph.clip(energy, e_ref, e_cut)[1]
        edge = np.inf
        if e_cut > 0:
            with np.errstate(invalid='ignore'):
                edge = float(np.nanmin(np.minimum(np.abs(energy - (e_ref + e_cut)), np.abs(energy - (e_ref - e_cut))) / tol_e))
        # the T-move
        choice, tmargin, moved = np.full(B, -1), np.full(B, np.inf), []
        x_cur = x.copy()
        x = x.copy()
        for k in range(B):
            p0, terms, scales = walker_terms(aux, k, nq)
            if not (w[k] > 0.0 and np.isfinite(energy[k]) and len(terms) > 0):
                continue
            t, r = intervals(terms, tau)
            theta = tu_all[i, k] * r[-1]
            edges = np.concatenate([[1.0], r[1:][t > 0.0]])
            tmargin[k] = float(np.abs(edges - theta).min()) / max(r_tolerance(tau, scales), 1e-300)
            c = heat_bath(terms, tau, tu_all[i, k])
            choice[k] = c
            if c >= 0:
                pr, q = p0 + c // nq, c % nq
                pl = aux['pl']
                e = int(pl['i'][pr])
                U = eh.rotated_points(aux['rot'][k:k + 1], nq)[0, q]
                x[k, 3 * e:3 * e + 3] = quadrature_point(cell_, x_cur[k, 3 * e:3 * e + 3], pl['r'][pr], pl['dhat'][pr], U)
                moved.append((k, e, x[k, 3 * e:3 * e + 3].copy()))
        live = w != 0.0
        row = np.array([w.sum(), (w[live] * energy[live]).sum(), (w[live] * energy[live] ** 2).sum(), acc.sum(), p.sum(), clipped.sum(),
                        (~finite).sum(), (w ** 2).sum(), B], dtype=np.float64)
        ecp_row = np.concatenate([(w[live, None] * epp[live]).sum(0), [float((choice >= 0).sum())]])
        ecp_tol = (w[live] * tol_e[live]).sum()
        w_commit, epp_commit = w.copy(), epp.copy()
        # the second chain pass
        mv = choice >= 0
        if mv.any():
            la3, ph3, dr3, el3, kr3 = orc.evaluate(x)
            dr = np.where(mv[:, None], dr3, dr)
            la, ph_, el, kr = np.where(mv, la3, la), np.where(mv, ph3, ph_), np.where(mv, el3, el), np.where(mv, kr3, kr)
            w = np.where(mv & ~(np.isfinite(la) & np.isfinite(el)), 0.0, w)
        cb, parents = None, np.arange(B)
        if branch_every > 0 and (i + 1) % branch_every == 0:
            cb = dh.comb(w, xi_all[i])
            parents = cb['parents']
            if cb['run']:
                x, dr, la, ph_, el, kr, epp = (v[parents] for v in (x, dr, la, ph_, el, kr, epp))
                w = np.full(B, cb['step'])
                row[8] = len(np.unique(parents))
            else:
                row[8] = 0
        out.append(dict(acc=acc, A=A, logu=logu, margin=A - logu, p=p, nonfinite=~finite, node=np.zeros(B, bool), clipped=clipped,
                        parents=parents, comb=cb, row=row, ecp_row=ecp_row, ecp_tol=ecp_tol, x_prev=x_prev, x_prop=xp, x_cur=x_cur,
                        energy=energy, tol_e=tol_e, epp=epp_commit, aux=aux, pairs=aux['pairs'], choice=choice,
                        tmargin=tmargin, moved=moved, w_commit=w_commit, w_after=w.copy(), xi=xi_all[i], chi=chi, u=u, edge=edge,
                        crossings=0, evaluated_in_place=int((~acc & (aux['pl']['counts'] > 0)).sum()),
                        died=int(((w_before > 0) & (w_commit == 0)).sum()),
                        ke_max=float(np.nanmax(np.abs(np.concatenate([kr, kr2]))))))
    state = dict(x=x, logabs=la, phase=ph_, drift=dr, eloc=el, weight=w, ke=kr, epp=epp)
    return dict(state=state, state0=state0, steps=out, normals=nz_all, uniforms=un_all, comb_uniforms=xi_all, tmove_uniforms=tu_all)


# case -> (B, tau, steps, seed): the replays of the GPU suite, as dmc_ecp_helpers.REPLAYS; seeds from tools/find_dmc_tmove_seeds.py
# (oracle only).  One walker of the lih replay starts with a NaN coordinate: it is the walker that dies.
REPLAYS = {
    # 20 accepted, 4 rejected (3 of them evaluated in place), 1 T-move (walker 3, configuration 7), 1 dead, min |A - log u| 7.9e-2,
    # T-move margin 2.2e5 bounds, cutoff distance 3.1e-3  (seeds 1..6 take no T-move)
    'lih': (12, 0.1, 2, 7),
    # 22 accepted, 2 rejected, 2 T-moves (walker 11 -> 5, walker 9 -> 7), min |A - log u| 7.4e-2, T-move margin 1.2e5 bounds
    'lih_twist': (12, 0.1, 2, 1),
    # 7 accepted, 5 rejected, 1 T-move (walker 2 -> 146), min |A - log u| 0.23, T-move margin 5.3e4 bounds
    'bcc_li': (6, 0.05, 2, 1),
}
DEAD = 7                       # the walker of the lih replay that starts with a NaN coordinate


@functools.lru_cache(maxsize=None)
def replay_reference(name=NAME, seed=None):
    """The model's run of the replay of case `name` from state_valid = 0, comb every step, Philox offset 0; e_ref, e_trial and e_cut
    as dmc_ecp_helpers.replay_reference chooses them."""
    B, tau, steps, sd = REPLAYS[name]
    sd = sd if seed is None else seed
    ecp = deh.potential(name)
    orc = TmoveOracle(name, ecp, sd)
    x0 = dh.start_walkers(name, B, sd)
    if name == NAME:
        x0[DEAD, 2] = np.nan
    el0 = orc.evaluate(x0, 0)[3]
    e_ref = float(np.round(np.nanmean(el0), 3))
    e_cut = 0.05 * np.sqrt(orc.n / tau)
    w0 = dh.preset_weights('ramp', B)
    r = run_model(orc, x0, w0, steps, tau, tau, e_ref, e_ref, e_cut, 1, sd, 0)
    r['tau_eff'] = tau
    r.update(x0=x0, w0=w0, e_ref=e_ref, e_cut=e_cut, tau=tau, seed=sd, B=B, ecp=ecp, name=name, cond=conditions(r, name))
    return r


def conditions(r, name=NAME):
    """`dmc_helpers.conditions` plus: the T-moves taken, the smallest distance of a T-move decision from an interval edge in units of
    the a-priori bound on r_c, the rejected walkers evaluated in place, the walkers that died, the cutoff distance and the clip
    edge as dmc_ecp_helpers.conditions, the weight tolerance with the pseudopotential's share."""
    c = dh.conditions(r)
    st = r['steps']
    c['name'] = name
    c['tmoves'] = sum(int((s['choice'] >= 0).sum()) for s in st)
    c['tmove_margin'] = min(float(s['tmargin'].min()) for s in st)
    c['evaluated_in_place'] = sum(s['evaluated_in_place'] for s in st)
    c['died'] = sum(s['died'] for s in st) + int((r['state0']['weight'] == 0).sum())
    c['cutoff_distance'] = min(s['aux']['cutoff_distance'] for s in st)
    c['edge'] = min(s['edge'] for s in st)
    tol_e = max(float(np.nanmax(s['tol_e'])) for s in st)
    c['tol_w'] = r.get('tau_eff', 0.0) * len(st) * tol_e
    return c


def assert_conditions(c, died=True):
    """As dmc_helpers.assert_conditions: fails loudly when a changed fixture or oracle leaves a test comparing nothing."""
    assert c['undecidable'] == 0 and c['min_margin'] > dh.TOL_A, c
    assert c['min_tooth'] > c['tol_w'], c
    assert c['cutoff_distance'] > eh.CUTOFF_MARGIN, c
    assert c['edge'] > 1.0, c
    assert c['tmove_margin'] > 10.0, c
    for k in ('accepted', 'rejected', 'tmoves', 'evaluated_in_place') + (('died',) if died else ()):
        assert c[k] >= 1, (k, c)
