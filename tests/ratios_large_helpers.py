"""Shared by test_ratios_large_cpu.py and test_gpu_ratios_large.py: which samples of the large cells (48 to 108 electrons) and of the
full lih batches the ratio passes `ds_one_body_ratios`, `ds_spin_exchange_ratios` and `ds_ecp_energy` are tested on, and the oracle
side of each, computed once.  Every oracle call goes through `sampler_helpers.Oracle.logdet`, 8 configurations per vmap."""
import functools

import numpy as np

import ecp_helpers as eh
import onebody_helpers as oh
import sampler_helpers as sh
import spin_helpers as sp

TOL_Q = 2 * (1e-9 + 1e-8)              # test_gpu_onebody.TOL_Q
TOL_Q_F32 = 2 * (2e-3 + 5e-3)          # test_gpu_onebody.TOL_Q_F32
SEED, OFFSET = 20240607, 5             # the Philox key of the one-body shifts (test_gpu_onebody's)
WALKERS = 2                            # fixture walkers of a large cell
ONEBODY_CELLS = ['graphene', 'diamond', 'bcc_li_333', 'graphene_331']
SPIN_CELLS = ['diamond', 'bcc_li_333']
SPIN_M = 130                           # more than two laps of the 64 lanes of k_spin_walker
ECP_RULES = [('diamond', 12), ('bcc_li_333', 12), ('bcc_li_333', 6)]
F32_M = 24


def nelec_of(name):
    return tuple(int(v) for v in sh.case(name)[1].nelec)


def onebody_samples(name, f32=False):
    """-> (M, first_electron): float64 moves every electron once and wraps; float32 takes the last 12 up and the first 12 down."""
    N = sum(nelec_of(name))
    return (F32_M, N - 12) if f32 else (N + 1, N - 1)


def onebody_reference(name, f32=False):
    M, first = onebody_samples(name, f32)
    return oh.reference(name, SEED, OFFSET, M, first, f32, WALKERS), M, first


def spin_samples(name, f32=False):
    """-> (M, first_pair): the pair index wraps after 7 samples."""
    nu, nd = nelec_of(name)
    return (F32_M if f32 else SPIN_M), nu * nd - 7


def spin_reference(name, f32=False):
    M, first = spin_samples(name, f32)
    return sp.large_reference(name, M, first, f32, WALKERS), M, first


def ecp_reference(name, n_quad=12, f32=False):
    return eh.reference(name, n_quad, f32, eh.LARGE_WALKERS)


def scaled(q, q_ref):
    return np.abs(q - q_ref) / np.maximum(1.0, np.abs(q_ref))


def q_range(q):
    m = np.abs(q)
    return f'|q| in [{m.min():.3g}, {m.max():.3g}]'


# ------------------------------------------------------------------------------------------------------ full batches on lih
LIH_FIRST = 3                          # first_electron of the big one-body batch: the index wraps at once
OB_BIG = (1100, 61)                    # 67 100 configurations > 65 520 = 819 groups of 80
OB_CHECK = (0, 1074, 1099)             # walker 1074's samples are configurations 65 514 .. 65 574
SPIN_BIG = (700, 4)                    # 2 * 256 + 188 walkers: k_spin_final's thread t adds up to three walkers
SPIN_BAD = (300, 699)
SPIN_CHECK = (0, 255, 256, 698)
ECP_BIG = 2100                         # k_ecp_offsets: three walkers per thread, threads 700.. empty
ECP_CHECK = (0, 1023, 1024, 2099)
ECP_BAD = 1500


@functools.lru_cache(maxsize=None)
def lih_walkers(B):
    fx, cell, _, _, _ = sh.case('lih')
    x = sh.distinct_walkers(cell, fx['x'], B)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def onebody_big_reference():
    """x (B, 12), s (B, M, 3) replayed, and the oracle's q (3, M) on the walkers OB_CHECK."""
    B, M = OB_BIG
    cell = sh.case('lih')[1]
    x = lih_walkers(B)
    s, _ = oh.replay_shifts(SEED, OFFSET, B, M, cell.a)
    assert OB_CHECK[1] * M < 65520 < (OB_CHECK[1] + 1) * M
    w = list(OB_CHECK)
    q = oh.oracle_ratios(sh.oracle('lih'), x[w], s[w], LIH_FIRST)
    return dict(x=x, s=s, q=q, cell=cell, nelec=nelec_of('lih'))


@functools.lru_cache(maxsize=None)
def spin_big_reference():
    """x (B, 12) with a NaN coordinate in the walkers SPIN_BAD, and the oracle's q (4, M) on the walkers SPIN_CHECK."""
    B, M = SPIN_BIG
    x = np.array(lih_walkers(B))
    for k, w in enumerate(SPIN_BAD):
        x[w, 5 * k + 1] = np.nan
    q = sp.oracle_ratios(sh.oracle('lih'), x[list(SPIN_CHECK)], nelec_of('lih'), M, 0)
    return dict(x=x, q=q, nelec=nelec_of('lih'))


@functools.lru_cache(maxsize=None)
def ecp_big_reference():
    """The model of the ECP pass on ECP_BIG distinct lih walkers with the rotations of (eh.SEED, eh.OFFSET): x, ecp, pairs (the pair
    list), rot, Wn, e_loc / e_loc_mag / e_loc_terms, the walker `straddle` whose configurations contain number 65 520, and for the
    walkers `check` = ECP_CHECK + (straddle,) the oracle's ratios q[w], the energy e_nl[w] and its scale e_nl_scale[w]."""
    B, nq = ECP_BIG, 12
    cell = sh.case('lih')[1]
    x = lih_walkers(B)
    ecp = eh.make_ecp(cell, eh.CASES['lih'][0], nq)
    r, _, _ = eh.min_image(x, ecp.atoms, ecp.a)
    for rc in (eh.CASES['lih'][0], eh.LOCAL_FRACTION * eh.CASES['lih'][0]):
        assert np.abs(r - rc).min() > eh.CUTOFF_MARGIN, (rc, np.abs(r - rc).min())
    pl = eh.pair_list(ecp, x)
    off = np.concatenate([[0], np.cumsum(pl['counts'])]) * nq
    assert off[-1] > 65520, off[-1]
    straddle = int(np.searchsorted(off, 65520, side='right') - 1)
    assert off[straddle] < 65520 < off[straddle + 1], (off[straddle], off[straddle + 1])
    rot = eh.replay_rotations(eh.SEED, eh.OFFSET, B)
    Wn = eh.weights(ecp, pl, rot, nq)
    e_loc, mag, cnt = eh.local_energy(ecp, x)
    check = tuple(ECP_CHECK) + (straddle,)
    q, e_nl, scale = {}, {}, {}
    o = sh.oracle('lih')
    for w in check:
        k = pl['w'] == w
        sub = {key: pl[key][k] for key in ('w', 'i', 'I', 'r', 'd', 'dhat')}
        xd = eh.displaced(x, sub, rot, nq)
        q[w] = eh.oracle_ratios(o, x[w:w + 1], xd, np.zeros(len(xd), dtype=int))
        t = Wn[k] * q[w].reshape(-1, nq)
        e_nl[w] = t.sum()
        scale[w] = (np.abs(Wn[k]) * np.maximum(1.0, np.abs(q[w].reshape(-1, nq)))).sum()
    return dict(x=x, ecp=ecp, pairs=pl, off=off, rot=rot, Wn=Wn, e_loc=e_loc, e_loc_mag=mag, e_loc_terms=cnt, straddle=straddle,
                check=check, q=q, e_nl=e_nl, e_nl_scale=scale)


# ------------------------------------------------------------------------------------------------------ what float32 loses by itself
@functools.lru_cache(maxsize=None)
def onebody_f32_oracle_loss(name):
    """The float32 oracle's one-body ratios of the float32 samples of `name` against the float64 oracle at the same float32-rounded
    configurations: the largest scaled difference (what a float32 evaluation loses by itself, 48 samples)."""
    ref, M, first = onebody_reference(name, True)
    xd = oh.displaced(ref['x'], ref['s'], first).astype(np.float32).astype(np.float64)
    B, M, n3 = xd.shape
    o = sh.oracle(name)
    q64 = np.exp((o.logdet(xd.reshape(B * M, n3)).reshape(B, M) - o.logdet(ref['x'])[:, None]).numpy())
    return float(scaled(ref['q'], q64).max())


# ------------------------------------------------------------------------------------------------------ conditioning of the inputs
def ulp_perturbed(v, k, rng):
    """Every entry of v moved by +-k units in its last place, the sign drawn per entry."""
    v = np.asarray(v, dtype=np.float64)
    return v + rng.choice([-1.0, 1.0], v.shape) * k * np.spacing(np.abs(v))


def onebody_conditioning(name, n_samples=24):
    """The oracle's q of `n_samples` one-body samples per walker of a large cell (spread over the electrons the GPU test moves) at
    inputs x, s perturbed by +-2 and +-4 ulp, against q at the inputs themselves: -> (largest scaled change, |q|)."""
    ref, M, first = onebody_reference(name)
    N = sum(ref['nelec'])
    m = np.unique(np.linspace(0, M - 1, n_samples).round().astype(int))
    o = sh.oracle(name)
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in (2, 4):
        x, s = ulp_perturbed(ref['x'], k, rng), ulp_perturbed(ref['s'][:, m], k, rng)
        xd = np.repeat(x.reshape(len(x), 1, N, 3), len(m), axis=1).copy()
        xd[:, np.arange(len(m)), oh.electrons(M, N, first)[m]] += s
        l0, l1 = o.logdet(x), o.logdet(xd.reshape(len(x) * len(m), 3 * N)).reshape(len(x), len(m))
        q = np.exp((l1 - l0[:, None]).numpy())
        worst = max(worst, float(scaled(q, ref['q'][:, m]).max()))
    return worst, np.abs(ref['q'][:, m])
