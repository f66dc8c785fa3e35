"""Shared by test_dmc_cpu.py and test_gpu_dmc.py: a plain-numpy restatement of the fixed-phase DMC step and comb of csrc/ds_dmc.h
(the algorithm as include/deepsolid_hip.h states it) on top of the float64 CPU oracle -- `sampler_helpers.Oracle.value_and_grad`,
`oracle.forward_laplacian.stages(...)['ke']`, `oracle.hamiltonian.local_ewald_energy` -- and the noise model of `sampler_helpers`;
the replay fixtures with the margins their seeds gave, and the oracle-only conditions that keep them meaningful."""
import functools

import numpy as np
import torch

import sampler_helpers as sh
from common import tt
from oracle import forward_laplacian as ofl
from oracle import hamiltonian as oham
from oracle.network import params_to_torch

CHUNK = 256          # DMC_CHUNK of csrc/ds_dmc.h


# ------------------------------------------------------------------------------------------------------------------- the comb
def prefix_sums(w):
    """C of the comb in the library's documented order: sequential inside chunks of 256 consecutive walkers, chunk offsets
    sequential, C_j = offset + running sum.  Every sum is one float64 addition, so this is bit for bit what the device forms."""
    w = np.asarray(w, dtype=np.float64)
    C = np.empty_like(w)
    off = np.float64(0.0)
    for c0 in range(0, len(w), CHUNK):
        r = w[c0:c0 + CHUNK].copy()
        for i in range(1, len(r)):                       # (spelled out: the order does not hang on numpy's cumsum)
            r[i] = r[i - 1] + r[i]
        C[c0:c0 + CHUNK] = off + r
        off = off + r[-1]
    return C


def comb(w, xi):
    """-> dict(run, W, step, parents (B,) int, C, margin): parent of tooth k = number of j with (C_j - k step) <= xi step, clamped
    to the last walker of positive weight (the number of j with C_j < W); margin = the smallest |C_j - k step - xi step| / W over
    all (j, k).  run = False (W not finite or not positive): the comb is skipped and the parents are the identity."""
    w = np.asarray(w, dtype=np.float64)
    B = len(w)
    with np.errstate(invalid='ignore', over='ignore'):
        C = prefix_sums(w)
    W = C[-1]
    if not (np.isfinite(W) and W > 0.0):
        return dict(run=False, W=W, step=np.nan, parents=np.arange(B), C=C, margin=np.inf)
    step = W / np.float64(B)
    rhs = np.float64(xi) * step
    base = np.arange(B, dtype=np.float64) * step
    parents, last = np.empty(B, dtype=np.int64), int((C < W).sum())
    margin = np.inf
    for k0 in range(0, B, 512):                          # (B, B) differences in slabs
        d = C[None, :] - base[k0:k0 + 512, None]
        parents[k0:k0 + 512] = np.minimum((d <= rhs).sum(1), last)
        margin = min(margin, float(np.abs(d - rhs).min()) / W)
    return dict(run=True, W=W, step=step, parents=parents, C=C, margin=margin)


# --------------------------------------------------------------------------------------------------------------- the oracle side
class DmcOracle:
    """log|psi|, phase, drift and E_L = Re E_kin + E_ewald per walker from the float64 CPU oracle (or its float32 run)."""

    def __init__(self, name, f32=False):
        _, self.cell, self.klist, self.net_kw, params = sh.case(name)
        self.o = sh.oracle(name, f32)
        self.f32 = f32
        self.p = params_to_torch(params, torch.float32 if f32 else None)
        self.ew = oham.local_ewald_energy(self.cell)
        self.n = self.o.n
        self._cache = {}

    def evaluate(self, x):
        """x (B, 3N) -> (logabs, phase complex, drift (B, 3N), eloc, Re ke), numpy float64.  A walker with a non-finite coordinate
        gets NaN everywhere."""
        x = np.asarray(x, dtype=np.float64)
        key = x.tobytes()
        if key in self._cache:
            return self._cache[key]
        B = len(x)
        la, ph, dr, el, kr = np.full(B, np.nan), np.full(B, np.nan + 0j), np.full(x.shape, np.nan), np.full(B, np.nan), np.full(B, np.nan)
        ok = np.isfinite(x).all(1)
        if ok.any():
            xt = torch.as_tensor(x[ok], dtype=torch.float32 if self.f32 else torch.float64)
            lat, g = self.o.value_and_grad(xt)
            la[ok], dr[ok] = lat.double().numpy(), g.real.double().numpy()
            with self.o._ctx(), torch.no_grad():
                ld = torch.stack([self.o.ld.apply(self.o.p, y) for y in xt])
                ph[ok] = np.exp(1j * ld.imag.double().numpy())
                ke = [complex(ofl.stages(self.p, y, self.klist, self.cell, self.net_kw)['ke']).real for y in xt]
            ew = [float(self.ew(tt(y))) for y in x[ok]]
            el[ok], kr[ok] = np.asarray(ke) + np.asarray(ew), np.asarray(ke)
        if len(self._cache) >= 16:
            self._cache.clear()
        self._cache[key] = (la, ph, dr, el, kr)
        return self._cache[key]


def wrap(cell, x):
    a = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    f = x.reshape(len(x), -1, 3) @ np.linalg.inv(a)
    return ((f - np.floor(f)) @ a).reshape(len(x), -1)


def limited(v, tau):
    """Umrigar-Nightingale-Runge limiter with a = 1, per electron: v * 2 / (1 + sqrt(1 + 2 |v|^2 tau))."""
    v3 = v.reshape(len(v), -1, 3)
    return (v3 * (2.0 / (1.0 + np.sqrt(1.0 + 2.0 * (v3 ** 2).sum(-1, keepdims=True) * tau)))).reshape(v.shape)


def clip(e, e_ref, e_cut):
    return e if e_cut <= 0 else e_ref + np.clip(e - e_ref, -e_cut, e_cut)


def run_model(orc, x0, weight0, steps, tau, tau_eff, e_trial, e_ref, e_cut, node_mode, branch_every, seed, offset, dtype=np.float64):
    """The algorithm of ds_dmc_step from state_valid = 0 on the oracle.  -> dict: state (x, logabs, phase, drift, eloc, weight)
    after the call, state0 (after the initialisation), per step: acc, A, logu, margin (A - log u), p, flags (nonfinite, node,
    clipped), parents, comb (the comb dict or None), row (9,), x_prop, e_prop, crossings; `dtype` rounds the noise as the device
    does."""
    cell, N = orc.cell, orc.n
    B = len(x0)
    x = np.array(x0, dtype=np.float64)
    w = np.array(weight0, dtype=np.float64)
    la, ph, dr, el, kr = (np.array(v) for v in orc.evaluate(x))
    w[~(np.isfinite(la) & np.isfinite(el))] = 0.0
    state0 = dict(x=x.copy(), logabs=la.copy(), phase=ph.copy(), drift=dr.copy(), eloc=el.copy(), weight=w.copy(), ke=kr.copy())
    nz_all, un_all = sh.noise(seed, offset, steps, B, N)
    nz_all = nz_all.astype(dtype).astype(np.float64)
    xi_all = np.array([sh.uniform(seed, offset, i, np.uint64(B)) for i in range(steps)], dtype=np.float64).reshape(steps)
    out = []
    for i in range(steps):
        chi, u = nz_all[i], un_all[i]
        vb = limited(dr, tau)
        xp = wrap(cell, x + tau * vb + np.sqrt(tau) * chi)
        la2, ph2, dr2, el2, kr2 = orc.evaluate(xp)
        vb2 = limited(dr2, tau)
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            A = 2.0 * (la2 - la) + 0.5 * ((chi ** 2).sum(1) - ((chi + np.sqrt(tau) * (vb + vb2)) ** 2).sum(1))
            logu = np.log(u)
            finite = np.isfinite(A) & np.isfinite(el2)
            overlap = (ph2 * np.conj(ph)).real                       # Re(phase' conj(phase))
            node_ok = np.ones(B, bool) if node_mode == 0 else overlap > 0
            acc = finite & node_ok & (A > logu)
            p = np.where(finite & node_ok, np.minimum(1.0, np.exp(np.where(finite, A, 0.0))), 0.0)
            e_new = np.where(acc, el2, el)
            cn, co = clip(e_new, e_ref, e_cut), clip(el, e_ref, e_cut)
            wn = w * np.exp(-tau_eff * (0.5 * (cn + co) - e_trial))
        w = np.where(np.isfinite(wn), wn, 0.0)
        clipped = np.isfinite(e_new) & (cn != e_new)
        cross = sh.crossings(cell, x[np.isfinite(xp).all(1)], xp[np.isfinite(xp).all(1)])
        x_prev = x.copy()
        sel = acc[:, None]
        x, dr = np.where(sel, xp, x), np.where(sel, dr2, dr)
        la, ph, el, kr = np.where(acc, la2, la), np.where(acc, ph2, ph), np.where(acc, el2, el), np.where(acc, kr2, kr)
        live = w != 0.0
        row = np.array([w.sum(), (w[live] * el[live]).sum(), (w[live] * el[live] ** 2).sum(), acc.sum(), p.sum(), clipped.sum(),
                        (~finite).sum(), (w ** 2).sum(), B], dtype=np.float64)
        cb, parents = None, np.arange(B)
        if branch_every > 0 and (i + 1) % branch_every == 0:
            cb = comb(w, xi_all[i])
            parents = cb['parents']
            if cb['run']:
                x, dr, la, ph, el, kr = x[parents], dr[parents], la[parents], ph[parents], el[parents], kr[parents]
                w = np.full(B, cb['step'])
                row[8] = len(np.unique(parents))
            else:
                row[8] = 0
        out.append(dict(acc=acc, A=A, logu=logu, margin=A - logu, p=p, nonfinite=~finite, node=finite & ~node_ok, clipped=clipped,
                        overlap=overlap, parents=parents, comb=cb, row=row, x_prev=x_prev, x_prop=xp, e_prop=el2, la_prop=la2, crossings=cross,
                        w_after=w.copy(), xi=xi_all[i], chi=chi, u=u, ke_max=float(np.nanmax(np.abs(np.concatenate([kr, kr2]))))))
    state = dict(x=x, logabs=la, phase=ph, drift=dr, eloc=el, weight=w, ke=kr)
    return dict(state=state, state0=state0, steps=out, normals=nz_all, uniforms=un_all, comb_uniforms=xi_all)


# ------------------------------------------------------------------------------------------------------------- replay fixtures
# name -> (case, B, tau, steps, seed, preset weights or None).  Walkers: the tiled fixture walkers plus 0.3 x the normals of
# offset 1000 (wrapped).  Seeds from tools/find_dmc_seeds.py (oracle only, on the CPU); the comments are the margins they gave.
REPLAYS = {
    # min |A - log u| 1.7e-02, min tooth distance 4.5e-05 W; 81 accepted, 15 rejected, 67 crossings, 86 clipped, 1 duplicated
    'lih24': ('lih', 24, 0.1, 4, 1, None),
    # min |A - log u| 9.3e-03, min tooth distance 2.8e-07 W; 118 accepted, 22 rejected, 90 crossings, 127 clipped, 3 duplicated
    'lih70': ('lih', 70, 0.1, 2, 1, None),
    # min |A - log u| 7.4e-02, min tooth distance 4.8e-04 W; 26 accepted, 6 rejected, 25 crossings, 31 clipped, 5 duplicated
    # (with equal start weights two steps duplicate nobody: the weights are preset, the buffer is the caller's)
    'lih_twist16': ('lih_twist', 16, 0.1, 2, 1, 'ramp'),
    # min |A - log u| 2.7e-01, min tooth distance 8.5e-03 W; 13 accepted, 3 rejected, 27 crossings, 14 clipped, 1 duplicated
    'bcc_li8': ('bcc_li', 8, 0.05, 2, 1, 'ramp'),
}
TOL_A = 1e-7                  # the tolerance on A: that of the importance sampler's lp (test_gpu_samplers.TOL_LP['imp'])
# (the weight tolerance, relative to W, is worked out per run: tau_eff * steps * the E_L bound 1e-8 max(1, |ke|) + 1e-9 at the
#  largest |ke| the run met -- conditions()['tol_w'])


def start_walkers(name, B, seed):
    fx, cell, _, _, _ = sh.case(name)
    N = sum(int(v) for v in cell.nelec)
    x = sh.tiled_walkers(cell, fx['x'], B)
    nz, _ = sh.noise(seed, 1000, 1, B, N)
    return wrap(cell, x + 0.3 * nz[0])


def preset_weights(kind, B):
    if kind is None:
        return np.ones(B)
    assert kind == 'ramp'
    return 0.25 + 1.5 * np.arange(B, dtype=np.float64) / max(B - 1, 1) * (np.arange(B) % 2) + 0.5 * (np.arange(B) % 3 == 0)


@functools.lru_cache(maxsize=None)
def replay_reference(key):
    """The model's run of a replay fixture from state_valid = 0, comb every step.  e_ref = e_trial = the mean E_L of the start
    walkers rounded to 1e-3; e_cut = a quarter of the default 0.2 sqrt(N / tau), tight enough that energies are clipped."""
    name, B, tau, steps, seed, wk = REPLAYS[key]
    orc = dmc_oracle(name)
    x0 = start_walkers(name, B, seed)
    el0 = orc.evaluate(x0)[3]
    e_ref = float(np.round(np.mean(el0), 3))
    e_cut = 0.05 * np.sqrt(orc.n / tau)
    r = run_model(orc, x0, preset_weights(wk, B), steps, tau, tau, e_ref, e_ref, e_cut, 0, 1, seed, 0)
    r['tau_eff'] = tau
    r.update(x0=x0, w0=preset_weights(wk, B), e_ref=e_ref, e_cut=e_cut, tau=tau, seed=seed, name=name, cond=conditions(r))
    return r


# node_mode = 1: lih (a real wavefunction: the phase is +-1) at a time step large enough that a proposal changes the sign of psi
# and would be accepted otherwise.  (B, tau, seed) from tools/find_dmc_seeds.py --node.
NODE = ('lih', 16, 0.5, 1)


@functools.lru_cache(maxsize=None)
def node_reference(seed=None):
    """One step on lih with node_mode = 0 and 1 from the same start, comb off.  cond['crossing_accepted'] = the proposals with
    Re(phase' conj(phase)) < 0 and A > log u: node_mode = 0 accepts them, node_mode = 1 refuses them."""
    name, B, tau, sd = NODE
    sd = sd if seed is None else seed
    orc = dmc_oracle(name)
    x0 = start_walkers(name, B, sd)
    e_ref = float(np.round(np.nanmean(orc.evaluate(x0)[3]), 3))
    r0 = run_model(orc, x0, np.ones(B), 1, tau, tau, e_ref, e_ref, 0.0, 0, 0, sd, 0)
    r1 = run_model(orc, x0, np.ones(B), 1, tau, tau, e_ref, e_ref, 0.0, 1, 0, sd, 0)
    s = r0['steps'][0]
    cross = (s['overlap'] < 0) & (s['margin'] > TOL_A)
    c = conditions(r0)
    c.update(crossing_accepted=int(cross.sum()), walkers=np.nonzero(cross)[0].tolist())
    return dict(free=r0, fixed=r1, x0=x0, e_ref=e_ref, tau=tau, seed=sd, B=B, name=name, cond=c)


F32 = ('lih', 8, 0.1, 1)      # (case, B, tau, seed) of the float32 step


@functools.lru_cache(maxsize=None)
def f32_reference():
    """One step on lih from float32-rounded walkers, comb off: the float64 model with the noise rounded to float32, and the error
    budget of log|psi| and E_L at the start walkers and at the proposals: 3 x what the oracle's own float32 run loses there (the
    floor rule of common.float32_tolerance), relative to max(1, |value|)."""
    from common import float32_tolerance
    name, B, tau, seed = F32
    o64, o32 = dmc_oracle(name), dmc_oracle(name, True)
    x0 = start_walkers(name, B, seed).astype(np.float32).astype(np.float64)
    e_ref = float(np.round(np.nanmean(o64.evaluate(x0)[3]), 3))
    r = run_model(o64, x0, np.ones(B), 1, tau, tau, e_ref, e_ref, 0.0, 0, 0, seed, 0, dtype=np.float32)
    s = r['steps'][0]
    budget = {}
    for tag, xs in (('start', x0), ('prop', s['x_prop'].astype(np.float32).astype(np.float64))):
        a, b = o64.evaluate(xs), o32.evaluate(xs)
        for q, idx in (('logabs', 0), ('eloc', 3)):
            scale = np.maximum(1.0, np.abs(a[idx]))
            loss = (np.abs(b[idx] - a[idx]) / scale).tolist()
            budget[tag, q] = np.array([float32_tolerance(loss, w) for w in range(B)]) * scale
    # A = 2 (log|psi'| - log|psi|) + ...: what the two budgets can move it by
    tol_a = 2.0 * (budget['start', 'logabs'] + budget['prop', 'logabs'])
    c = conditions(r)
    c['undecidable'] = int((np.abs(s['margin']) <= tol_a).sum())
    r.update(x0=x0, e_ref=e_ref, tau=tau, seed=seed, B=B, name=name, budget=budget, tol_a=tol_a, cond=c)
    return r


@functools.lru_cache(maxsize=None)
def dmc_oracle(name, f32=False):
    return DmcOracle(name, f32)


def conditions(r):
    """The oracle-only conditions of a model run: decidable decisions and teeth, and that every kind of event happened."""
    st = r['steps']
    fin = [s['margin'][np.isfinite(s['margin'])] for s in st]
    tol_w = r.get('tau_eff', 0.0) * len(st) * (1e-8 * max(1.0, max(s['ke_max'] for s in st)) + 1e-9)
    return dict(tol_w=tol_w, min_margin=min(float(np.abs(m).min()) for m in fin if len(m)),
                undecidable=sum(int((np.abs(m) <= TOL_A).sum()) for m in fin),
                min_tooth=min((s['comb']['margin'] for s in st if s['comb'] is not None and s['comb']['run']), default=np.inf),
                accepted=sum(int(s['acc'].sum()) for s in st), rejected=sum(int((~s['acc']).sum()) for s in st),
                crossings=sum(s['crossings'] for s in st), clipped=sum(int(s['clipped'].sum()) for s in st),
                duplicated=sum(int((np.bincount(s['parents']) > 1).sum()) for s in st),
                killed=sum(int(len(s['parents']) - len(np.unique(s['parents']))) for s in st))


def assert_conditions(c, need=('accepted', 'rejected', 'crossings', 'clipped', 'duplicated', 'killed')):
    """Fails loudly when a changed fixture or oracle leaves a test comparing nothing.  No decision is left out."""
    assert c['undecidable'] == 0 and c['min_margin'] > TOL_A, c
    assert c['min_tooth'] > c['tol_w'], c
    for k in need:
        assert c[k] >= 1, (k, c)
