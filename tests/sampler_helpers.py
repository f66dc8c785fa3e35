"""Shared by test_cabi_cpu.py and test_gpu_samplers.py: a plain-numpy model of the in-kernel noise of csrc/ds_mcmc.h (Philox4x32-10,
the 53-bit uniforms, the float64 Box-Muller and the counter layout), and the float64 CPU oracle side of the sampler and walker-
gradient tests (oracle/qmc.py per move, torch autograd over oracle/network.py) with the decision margins of every move."""
import contextlib

import numpy as np
import torch

from common import oracle_net, tt
from oracle import qmc as oqmc
from oracle.network import params_to_torch, working_dtype

_M32 = np.uint64(0xFFFFFFFF)
_U64 = np.uint64


def _u64(v):
    """Python ints / arrays of ints in [0, 2^64) -> uint64 array (values are taken modulo 2^64, like the C ABI's uint64_t)."""
    if isinstance(v, np.ndarray) and v.dtype == np.uint64:
        return v
    return np.asarray([int(t) & (2 ** 64 - 1) for t in np.asarray(v, dtype=object).reshape(-1)],
                      dtype=np.uint64).reshape(np.shape(v))


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11), vectorised: counter words c0..c3 and key words k0, k1 are uint64 arrays
    holding 32-bit values (broadcast against each other) -> (4, ...) uint64 array of the four 32-bit output words."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = _U64(0xD2511F53) * c0                      # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = _U64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> _U64(32), p0 & _M32, p1 >> _U64(32), p1 & _M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + _U64(0x9E3779B9)) & _M32, (k1 + _U64(0xBB67AE85)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3))


def philox_block(seed, offset, step, index, stream):
    """The block the kernels draw for (seed, offset + step, index, stream) -- the interface of `ds_philox_host`: the index fills
    c0 / c1, offset + step (modulo 2^64) fills c2 and the low 30 bits of c3, the stream number its two top bits."""
    seed, index = _u64(seed), _u64(index)
    off = _u64(offset) + _u64(step)                      # uint64 arithmetic wraps like the kernel's
    c3 = ((off >> _U64(32)) & _U64(0x3FFFFFFF)) | (np.asarray(stream, dtype=np.uint64) << _U64(30))
    return philox4x32_10(index & _M32, index >> _U64(32), off & _M32, c3, seed & _M32, seed >> _U64(32))


def _u53(a, b):
    return ((a << _U64(21)) ^ (b >> _U64(11))) & _U64(2 ** 53 - 1)


def u53_co(a, b):
    """Two 32-bit words -> a float64 uniform in [0, 1)."""
    return _u53(a, b).astype(np.float64) * (1.0 / 9007199254740992.0)


def u53_oc(a, b):
    """Two 32-bit words -> a float64 uniform in (0, 1]."""
    return (_u53(a, b) + _U64(1)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normal3(seed, offset, step, index):
    """The three standard-normal deviates of electron `index` at move `step`: Box-Muller in float64 on the blocks of streams 0
    (both deviates of its pair) and 1 (the cosine deviate only).  -> (..., 3)."""
    a = philox_block(seed, offset, step, index, 0)
    b = philox_block(seed, offset, step, index, 1)
    ra = np.sqrt(-2.0 * np.log(u53_oc(a[0], a[1])))
    ta = 2.0 * np.pi * u53_co(a[2], a[3])
    rb = np.sqrt(-2.0 * np.log(u53_oc(b[0], b[1])))
    return np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(2.0 * np.pi * u53_co(b[2], b[3]))], axis=-1)


def uniform(seed, offset, step, walker):
    """The uniform deviate in [0, 1) of walker `walker`'s accept test at move `step` (stream 2)."""
    a = philox_block(seed, offset, step, walker, 2)
    return u53_co(a[0], a[1])


def noise(seed, offset, steps, B, N, one_electron=False, first_electron=0):
    """What a fused sampler draws in Philox mode, in the shapes `SystemDevice.mcmc_step` takes as explicit noise:
    -> (normals (steps, B, 3N), uniforms (steps, B)) float64; with `one_electron` normals is (steps, B, 3) and holds, for move
    i, the deviates of electron (first_electron + i) % N of every walker.  Electron e of walker w has index w * N + e."""
    w = np.arange(B, dtype=np.uint64)
    un = np.stack([uniform(seed, offset, i, w) for i in range(steps)]) if steps else np.zeros((0, B))
    nz = []
    for i in range(steps):
        if one_electron:
            idx = w * _U64(N) + _U64((first_electron + i) % N)
            nz.append(normal3(seed, offset, i, idx))
        else:
            nz.append(normal3(seed, offset, i, np.arange(B * N, dtype=np.uint64)).reshape(B, 3 * N))
    return (np.stack(nz) if steps else np.zeros((0, B, 3 if one_electron else 3 * N))), un


# ---------------------------------------------------------------------------------------------------------------- oracle side
def tiled_walkers(cell, x, B):
    """Fixture walkers tiled to B rows and wrapped into the simulation cell (numpy float64)."""
    x = np.tile(np.asarray(x, dtype=np.float64), ((B + len(x) - 1) // len(x), 1))[:B]
    a = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    frac = x.reshape(B, -1, 3) @ np.linalg.inv(a)
    return ((frac - np.floor(frac)) @ a).reshape(B, -1)


def distinct_walkers(cell, x, B):
    """`tiled_walkers` plus a displacement of every coordinate, uniform in +-0.05 Bohr from a fixed seed, wrapped into the cell again:
    B rows of which no two are equal, so a result read from the wrong walker differs.  Row w is the same for every B > w."""
    t = tiled_walkers(cell, x, B)
    a = np.asarray(cell.a, dtype=np.float64).reshape(3, 3)
    t = t + np.random.default_rng(20251021).uniform(-0.05, 0.05, t.shape)
    frac = t.reshape(B, -1, 3) @ np.linalg.inv(a)
    out = ((frac - np.floor(frac)) @ a).reshape(B, -1)
    assert len(np.unique(out, axis=0)) == B
    return out


class Oracle:
    """The CPU oracle of one case: log|psi| and its complex walker gradient per walker (torch autograd over oracle/network.py),
    and single moves of the four samplers of oracle/qmc.py with the margin every decision was taken on.
    dtype=torch.float32 runs the same restatement in float32 (what the float32 tests take their error budget from).
    Evaluations are cached per walker, so a move that is evaluated twice (once with every walker accepting, to see the
    proposal's own lp_2) costs one forward per walker."""

    def __init__(self, cell, klist, net_kw, params, dtype=None):
        self.cell, self.dtype = cell, dtype
        self.rd = dtype or torch.float64
        with self._ctx():
            self.ld = oracle_net(cell, klist, net_kw, 'eval_logdet')
            self.p = params_to_torch(params, dtype)
        self.latvec = torch.as_tensor(np.asarray(cell.a, dtype=np.float64).reshape(3, 3)).to(self.rd)
        self.n = sum(int(v) for v in cell.nelec)
        self._val, self._vg = {}, {}

    def _ctx(self):
        return working_dtype(self.dtype) if self.dtype is not None else contextlib.nullcontext()

    def _x(self, x):
        return (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(self.rd)

    def _cached(self, store, xs, fn):
        k = xs.numpy().tobytes()
        if k not in store:
            if len(store) >= 8:
                store.clear()
            store[k] = fn(xs)
        return store[k]

    def logdet(self, xs, step=None):
        """The complex eval_logdet = log|psi| + i arg psi of every row of xs (n, 3N), `step` rows per vmap -> torch tensor (n,) in
        the oracle's complex dtype.  Default: 8 rows from 48 electrons on (one vmap over a thousand configurations of such a cell
        needs more memory than a test may take; 8 rows stay under 0.9 GB up to 108 electrons), all rows in one vmap below, where
        the results are what they were before there were slices.  With a float32 oracle the rows are rounded to float32."""
        xs = self._x(np.array(xs, dtype=np.float64))
        if step is None:
            step = 8 if self.n >= 48 else max(len(xs), 1)
        with self._ctx(), torch.no_grad():
            f = torch.func.vmap(lambda y: self.ld.apply(self.p, y))
            if len(xs) == 0:
                return torch.zeros(0, dtype=torch.complex64 if self.rd == torch.float32 else torch.complex128)
            return torch.cat([f(xs[i:i + step]) for i in range(0, len(xs), step)])

    def logabs(self, p, xs):
        """f(params, x) of oracle/qmc.py: log|psi| of a batch (the per-walker oracle under torch.func.vmap)."""
        with self._ctx(), torch.no_grad():
            return self._cached(self._val, self._x(xs), lambda x: torch.func.vmap(lambda y: self.ld.apply(self.p, y).real)(x))

    def value_and_grad(self, xs):
        """-> (log|psi| (B,), grad (B, 3N) complex: Re = autograd of log|psi|, Im = autograd of arg psi, both from the oracle's
        eval_logdet = log|psi| + i arg psi)."""
        def both(y):
            out = self.ld.apply(self.p, y)
            return torch.stack([out.real, out.imag]), out.real

        def run(x):
            if x.shape[0] == 0:
                return torch.zeros(0, dtype=self.rd), torch.zeros(0, x.shape[1], dtype=torch.complex64 if self.rd == torch.float32 else torch.complex128)
            jac, la = torch.func.vmap(torch.func.jacrev(both, has_aux=True))(x)
            return la.detach(), torch.complex(jac[:, 0], jac[:, 1]).detach()
        with self._ctx():
            return self._cached(self._vg, self._x(xs), run)

    def logabs_and_drift(self, p, xs):
        """f(params, x) of oracle.qmc.importance_update: (log|psi|, grad log|psi|)."""
        la, g = self.value_and_grad(xs)
        return la, g.real

    def update(self, kind, x1, lp1, width, normal, uniform, atoms=None, i=0):
        """oracle/qmc.py's own per-move function of `kind` -> (x_new, lp_new, num_accepts)."""
        zero = torch.zeros((), dtype=self.rd)
        kw = dict(stddev=width, normal=self._x(normal), uniform=self._x(uniform))
        x1, lp1 = self._x(x1), self._x(lp1)
        with self._ctx():
            if kind == 'mh':
                return oqmc.mh_update(self.p, self.logabs, x1, lp1, zero, self.latvec, **kw)
            if kind == 'asym':
                return oqmc.mh_update(self.p, self.logabs, x1, lp1, zero, self.latvec, atoms=np.asarray(atoms, dtype=np.float64), **kw)
            if kind == 'one':
                return oqmc.mh_one_electron_update(self.p, self.logabs, x1, lp1, zero, self.latvec, i=i, **kw)
            if kind == 'imp':
                return oqmc.importance_update(self.p, self.logabs_and_drift, x1, lp1, zero, self.latvec, **kw)
        raise ValueError(kind)

    def move(self, kind, x1, lp1, width, normal, uniform, atoms=None, i=0):
        """One move of `kind` in ('mh', 'one', 'imp', 'asym') from (x1, lp1).  -> dict: x, lp, nacc (what the oracle's function
        returns), x2, lp2 (the proposal and ITS lp_2 for every walker: the same function with u = 0, so that every walker
        accepts), margin (ratio - log u, the quantity the decision is the sign of) and cond (the oracle's decisions)."""
        x1, lp1, un = self._x(x1), self._x(lp1), self._x(uniform)
        x2, lp2, _ = self.update(kind, x1, lp1, width, normal, torch.zeros_like(un), atoms, i)
        x, lp, nacc = self.update(kind, x1, lp1, width, normal, un, atoms, i)
        ratio = lp2 - lp1
        if kind == 'asym':           # + lq_2 - lq_1: the proposal densities of oracle.qmc.mh_update's asymmetric branch
            with self._ctx():
                at = self._x(np.asarray(atoms, dtype=np.float64))
                a1, a2 = x1.reshape(len(x1), -1, 1, 3), x2.reshape(len(x1), -1, 1, 3)
                # enforce_pbc moved x2: the oracle takes the densities on the WRAPPED proposal, as its reference does
                h1, h2 = oqmc._harmonic_mean(a1, at), oqmc._harmonic_mean(a2, at)
                ratio = ratio + oqmc._log_prob_gaussian(a2, a1, width * h2) - oqmc._log_prob_gaussian(a1, a2, width * h1)
        margin = ratio - torch.log(un)
        cond = margin > 0
        assert int(cond.sum()) == int(nacc) and torch.equal(torch.where(cond, lp2, lp1), lp)     # the margins ARE the oracle's decisions
        return dict(x=x, lp=lp, nacc=int(nacc), x2=x2, lp2=lp2, margin=margin, cond=cond)


KINDS = ('mh', 'one', 'imp', 'asym')


def crossings(cell, x1, x2):
    """Number of electrons whose fractional coordinates jumped by more than half a cell between x1 and x2 (both wrapped):
    proposals that crossed a cell face and were brought back by the wrap."""
    ainv = np.linalg.inv(np.asarray(cell.a, dtype=np.float64).reshape(3, 3))
    d = (np.asarray(x2, dtype=np.float64) - np.asarray(x1, dtype=np.float64)).reshape(len(x1), -1, 3) @ ainv
    return int((np.abs(d) > 0.5).any(-1).sum())


# ------------------------------------------------------------------------------------- references of tests/test_gpu_samplers.py
import functools

from common import float32_tolerance, load_case


@functools.lru_cache(maxsize=None)
def case(name):
    """load_case(name), or for 'mirror_0_3' / 'mirror_1_2' the one-atom bcc-Li cells with nelec = (0, 3) / (1, 2) (more spin-down
    than spin-up electrons: the library runs them as their mirror image) -> (fixture or None, cell, klist, net_kw, params)."""
    if name.startswith('mirror_'):
        from deepsolid_amd import systems
        from oracle.testing import make_test_params
        nelec = tuple(int(v) for v in name.split('_')[1:])
        cell, klist = systems.build('bcc_li', S=1, nelec=nelec)
        net_kw = dict(systems.DETNET_DEFAULTS)
        return None, cell, klist, net_kw, make_test_params(77, cell.original_cell.atom_coords(), cell.nelec, net_kw)
    return load_case(name)


@functools.lru_cache(maxsize=None)
def oracle(name, f32=False):
    _, cell, klist, net_kw, params = case(name)
    return Oracle(cell, klist, net_kw, params, torch.float32 if f32 else None)


def nuclei(cell):
    return np.asarray(cell.atom_coords(), dtype=np.float64).reshape(-1, 3)


def _conditions(moves, cell):
    """The three oracle-only conditions on a list of (start walkers, move dict, tolerance per walker): every decision decidable,
    at least one acceptance and one rejection, at least one proposed electron crossed a cell face."""
    smallest = min(float((m['margin'].double().abs() - t).min()) for _, m, t in moves)
    return dict(min_margin=min(float(m['margin'].abs().min()) for _, m, _ in moves),
                undecidable=sum(int((m['margin'].double().abs() <= t).sum()) for _, m, t in moves), slack=smallest,
                accepted=sum(int(m['cond'].sum()) for _, m, _ in moves),
                rejected=sum(int((~m['cond']).sum()) for _, m, _ in moves),
                crossings=sum(crossings(cell, x1, m['x2'].double().numpy()) for x1, m, _ in moves))


def assert_conditions(c):
    """Fails loudly when a changed fixture or oracle leaves a test comparing nothing."""
    assert c['undecidable'] == 0, c
    assert c['accepted'] >= 1 and c['rejected'] >= 1, c
    assert c['crossings'] >= 1, c


@functools.lru_cache(maxsize=None)
def single_move_reference(name, kind, seed, width, B, i=0, f32=False):
    """One move of `kind` from the oracle's own state on the first B (tiled, wrapped) fixture walkers of `name`, noise from
    noise(seed, ...).  -> dict: x1, lp1 (= 2 log|psi|), nz, un (what the device is given; float32-rounded with f32), the
    float64 oracle's move (x, lp, nacc, x2, lp2, margin, cond), tol (the tolerance on lp per walker: 1e-7, or with f32 the
    float32 budget -- 3 x what the oracle's own float32 run of this move loses at the proposal, floor rule of
    common.float32_tolerance, times max(1, |lp_2|)), loss (that run's relative loss per walker) and cond3 (the conditions)."""
    fx, cell, _, _, _ = case(name)
    o = oracle(name)
    x1 = tiled_walkers(cell, fx['x'], B)
    nz, un = noise(seed, 0, 1, B, o.n, one_electron=kind == 'one', first_electron=i % o.n)
    nz, un = nz[0], un[0]
    if f32:
        x1, nz, un = (v.astype(np.float32).astype(np.float64) for v in (x1, nz, un))
    lp1 = 2.0 * o.logabs(o.p, tt(x1))
    r = dict(o.move(kind, x1, lp1, width, nz, un, nuclei(cell), i))
    if f32:
        r32 = oracle(name, True).move(kind, x1, lp1.float(), width, nz, un, nuclei(cell), i)
        scale = r['lp2'].abs().clamp(min=1.0)
        loss = ((r32['lp2'].double() - r['lp2']).abs() / scale).tolist()
        tol = torch.as_tensor([float32_tolerance(loss, b) for b in range(B)], dtype=torch.float64) * scale
        r['x2_f32'] = r32['x2'].double()
    else:
        loss, tol = [0.0] * B, torch.full((B,), 1e-7, dtype=torch.float64)
    r.update(x1=x1, lp1=lp1, nz=nz, un=un, tol=tol, loss=loss, cond3=_conditions([(x1, r, tol)], cell))
    return r


@functools.lru_cache(maxsize=None)
def chain_reference(name, kind, seed, width, B, steps):
    """The oracle's chain of `steps` moves of `kind` on B tiled fixture walkers, with the noise the kernels draw for
    (seed, offset 0): -> dict x0, nz, un, moves (the oracle's move dict per step) and cond3 (tolerance on lp: 1e-7)."""
    fx, cell, _, _, _ = case(name)
    o = oracle(name)
    x0 = tiled_walkers(cell, fx['mcmc_x0'] if 'mcmc_x0' in fx else fx['x'], B)
    nz, un = noise(seed, 0, steps, B, o.n, one_electron=kind == 'one')
    x, lp = tt(x0), 2.0 * o.logabs(o.p, tt(x0))
    tol = torch.full((B,), 1e-7, dtype=torch.float64)
    moves, tri = [], []
    for i in range(steps):
        m = o.move(kind, x, lp, width, nz[i], un[i], nuclei(cell), i)
        moves.append(m)
        tri.append((x.numpy(), m, tol))
        x, lp = m['x'], m['lp']
    return dict(x0=x0, nz=nz, un=un, moves=moves, cond3=_conditions(tri, cell))


# Seeds and widths found by tools/find_sampler_seeds.py (oracle only, on the CPU); each comment is the smallest |margin| the entry
# gave, and what the oracle decided.  (The asymmetric move takes its proposal densities on the WRAPPED proposal, like the reference:
# a walker with an electron across a cell face has a margin of hundreds and is rejected.)
CHAIN_BATCH = 70          # two accept workgroups, the second partial; B * N = 1680 > 1024 electrons on bcc_li for k_max_norm3
# (case, kind) -> (seed, width, moves); the one-electron sampler gets N moves
CHAINS = {
    ('lih', 'mh'): (1, 0.05, 3),         # min |m| 1.21e-03; 198 accepted, 12 rejected, 27 crossings
    ('lih', 'one'): (1, 0.5, 4),        # min |m| 2.53e-04; 175 accepted, 105 rejected, 70 crossings
    ('lih', 'imp'): (1, 0.05, 2),        # min |m| 1.33e-02; 134 accepted, 6 rejected, 12 crossings
    ('lih', 'asym'): (1, 0.02, 3),       # min |m| 1.04e-03; 155 accepted, 55 rejected, 54 crossings
    ('bcc_li', 'mh'): (1, 0.05, 3),      # min |m| 1.71e-02; 170 accepted, 40 rejected, 62 crossings
    ('bcc_li', 'one'): (1, 0.5, 24),     # min |m| 1.92e-03; 1266 accepted, 414 rejected, 218 crossings
    ('bcc_li', 'imp'): (1, 0.05, 2),     # min |m| 1.26e-04; 124 accepted, 16 rejected, 35 crossings
    ('bcc_li', 'asym'): (1, 0.02, 3),    # min |m| 1.05e-02; 116 accepted, 94 rejected, 201 crossings
}
# (case, float32, kind) -> (seed, width, B, electron index of the one-electron move)
SINGLE_MOVES = {
    ('graphene', False, 'mh'): (1, 0.1, 4, 0),        # min |m| 1.87e-01; 2 acc, 2 rej, 3 crossings
    ('graphene', False, 'one'): (2, 0.5, 4, 29),      # min |m| 1.23e-01; 3 acc, 1 rej, 1 crossings
    ('graphene', False, 'imp'): (1, 0.1, 4, 0),       # min |m| 5.31e-02; 3 acc, 1 rej, 3 crossings
    ('graphene', False, 'asym'): (1, 0.02, 4, 0),      # min |m| 2.27e+01; 1 acc, 3 rej, 14 crossings
    ('diamond', False, 'one'): (2, 2.0, 2, 77),       # min |m| 1.64e+00; 1 acc, 1 rej, 1 crossings
    ('diamond', False, 'imp'): (1, 0.05, 2, 0),        # min |m| 6.33e-01; 1 acc, 1 rej, 1 crossings
    ('diamond', False, 'asym'): (1, 0.02, 2, 0),       # min |m| 1.53e+03; 1 acc, 1 rej, 4 crossings
    ('lih', True, 'mh'): (1, 0.4, 6, 0),              # min |m| 2.29e-01; 3 acc, 3 rej, 1 crossings
    ('lih', True, 'one'): (1, 0.5, 6, 3),             # min |m| 4.54e-01; 5 acc, 1 rej, 1 crossings
    ('lih', True, 'imp'): (1, 0.4, 6, 0),             # min |m| 1.46e-01; 5 acc, 1 rej, 2 crossings
    ('lih', True, 'asym'): (1, 0.05, 6, 0),            # min |m| 2.10e-01; 5 acc, 1 rej, 1 crossings
    ('bcc_li', True, 'mh'): (1, 0.05, 4, 0),           # min |m| 1.06e+00; 3 acc, 1 rej, 2 crossings
    ('bcc_li', True, 'one'): (1, 1.0, 4, 17),         # min |m| 7.60e-01; 3 acc, 1 rej, 2 crossings
    ('bcc_li', True, 'imp'): (1, 0.05, 4, 0),          # min |m| 4.02e-01; 3 acc, 1 rej, 2 crossings
    ('bcc_li', True, 'asym'): (1, 0.1, 4, 0),         # min |m| 3.25e+01; 2 acc, 2 rej, 18 crossings
    ('diamond', True, 'mh'): (1, 0.05, 4, 0),          # min |m| 1.55e+00; 3 acc, 1 rej, 4 crossings
    ('diamond', True, 'one'): (1, 0.5, 4, 77),        # min |m| 1.60e-01; 3 acc, 1 rej, 1 crossings
    ('diamond', True, 'imp'): (1, 0.05, 4, 0),         # min |m| 6.33e-01; 3 acc, 1 rej, 4 crossings
    ('diamond', True, 'asym'): (1, 0.02, 4, 0),        # min |m| 1.53e+03; 1 acc, 3 rej, 18 crossings
}
