"""numpy float64 oracle of the real-space counts (`ds_realspace_counts`, csrc/ds_realspace.h) and the inputs the tests share.

The oracle deliberately does not use the kernel's algorithm.  The density follows the folding rule of the header.  The pairs are
brute force: every electron is wrapped into the simulation cell, then EVERY image shift in -2..2 per axis of every pair is
measured and every image with |d| < r_max is counted (the kernel wraps the difference and keeps the shortest of 27 images).

Both return an *edge margin* next to the counts: the smallest |t - round(t)| over all t = f_j g_j (density) and over all
t = r n_r / r_max below n_r + 1 (pairs).  A value closer than 1e-9 to a bin edge could legitimately fall in either bin under a
different rounding, so every exact-equality test first asserts margin >= MARGIN for its input."""
import functools

import numpy as np

from deepsolid_amd import systems

MARGIN = 1e-9
SHIFTS5 = np.stack([m.ravel() for m in np.meshgrid(*[np.arange(-2, 3)] * 3, indexing='ij')], axis=1).astype(np.float64)


class SimpleCell:
    """The attributes `estimator.RealSpaceAccumulator` reads."""

    def __init__(self, a, nelec, prim=None):
        self.a = np.asarray(a, dtype=np.float64)
        self.nelec = tuple(int(n) for n in nelec)
        self.original_cell = self if prim is None else SimpleCell(prim, nelec)


# a skewed triclinic cell: r_ws = 2.5 (half of |a_0|), plane spacings (4.66, 5.29, 6.00), so r_ws < 1.5 x 4.66
TRICLINIC = np.array([[5.0, 0.0, 0.0], [1.5, 5.5, 0.0], [-1.2, 1.7, 6.0]])


def cubic_cell(n_up, n_dn, edge=9.0):
    return SimpleCell(np.eye(3) * edge, (n_up, n_dn))


def uniform_walkers(a, n, batch, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=(batch, n, 3)) @ np.asarray(a)).reshape(batch, 3 * n)


def push_out(x, a, seed):
    """Every electron moved by its own random lattice vector with coefficients in -2..2 (some coordinates turn negative)."""
    rng = np.random.default_rng(seed + 1000)
    B = x.shape[0]
    r = x.reshape(B, -1, 3)
    return (r + rng.integers(-2, 3, size=r.shape) @ np.asarray(a)).reshape(B, -1)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (cell, walkers (B, 3N) float64 pushed out of the cell).  The four library cells with the batch sizes and seeds of the
    table in DESIGN.md section 15, and the hand-made triclinic cell with nelec (3, 2)."""
    if name == 'triclinic':
        cell = SimpleCell(TRICLINIC, (3, 2), prim=TRICLINIC)
        return cell, push_out(uniform_walkers(TRICLINIC, 5, 64, 81), TRICLINIC, 81)
    batch, seed = {'bcc_li': (1025, 77), 'graphene': (257, 78), 'lih': (1025, 79), 'diamond': (130, 80)}[name]
    cell, _ = systems.build(name)
    return cell, push_out(systems.synthetic_walkers(cell, batch, seed=seed), cell.a, seed)


def density_oracle(x, n_up, fold, grid):
    """-> (counts (2, g0, g1, g2) int64, edge margin)."""
    B = x.shape[0]
    r = np.asarray(x, dtype=np.float64).reshape(B, -1, 3)
    N = r.shape[1]
    g = np.asarray(grid, dtype=np.int64)
    f = r @ np.linalg.inv(np.asarray(fold, dtype=np.float64))
    f = f - np.floor(f)
    t = f * g
    margin = float(np.abs(t - np.round(t)).min())
    idx = np.minimum(t.astype(np.int64), g - 1)
    flat = (idx[..., 0] * g[1] + idx[..., 1]) * g[2] + idx[..., 2]
    spin = (np.arange(N) >= n_up).astype(np.int64)
    counts = np.bincount((spin[None, :] * g.prod() + flat).ravel(), minlength=2 * g.prod())
    return counts.reshape(2, *g).astype(np.int64), margin


def pair_images(x, n_up, a, r_cut):
    """All images of all pairs i < j closer than r_cut, by brute force over the 125 shifts: -> (distances, channels)."""
    a = np.asarray(a, dtype=np.float64)
    B = x.shape[0]
    r = np.asarray(x, dtype=np.float64).reshape(B, -1, 3)
    N = r.shape[1]
    i, j = np.triu_indices(N, 1)
    if i.size == 0:
        return np.zeros(0), np.zeros(0, np.int64)
    chan = np.where(j < n_up, 0, np.where(i < n_up, 1, 2)).astype(np.int64)
    f = r @ np.linalg.inv(a)
    w = (f - np.floor(f)) @ a                          # every electron inside the cell
    d = w[:, i] - w[:, j]                              # (B, P, 3)
    shifts = SHIFTS5 @ a
    dist, ch = [], []
    for s in shifts:
        rr = np.sqrt(((d + s) ** 2).sum(axis=-1))
        m = rr < r_cut
        dist.append(rr[m])
        ch.append(np.broadcast_to(chan, rr.shape)[m])
    return np.concatenate(dist), np.concatenate(ch)


def bin_pairs(dist, chan, n_r, r_max):
    """-> (counts (3, n_r) int64, edge margin) from the image list of `pair_images` (made with r_cut >= r_max (1 + 1/n_r) for
    the margin to see every t below n_r + 1)."""
    t = dist * n_r / r_max
    near = t < n_r + 1
    margin = float(np.abs(t[near] - np.round(t[near])).min()) if near.any() else np.inf
    inside = dist < r_max
    k = t[inside].astype(np.int64)
    assert k.size == 0 or k.max() < n_r
    counts = np.bincount(chan[inside] * n_r + k, minlength=3 * n_r)
    return counts.reshape(3, n_r).astype(np.int64), margin


def pair_oracle(x, n_up, a, n_r, r_max):
    dist, chan = pair_images(x, n_up, a, 2.0 * r_max)
    return bin_pairs(dist, chan, n_r, r_max)


def pair_index_decode(n):
    """csrc/ds_realspace.h `rs_pair_of` for all p < n (n - 1) / 2, with its float32 square root: -> (lo, hi)."""
    p = np.arange(n * (n - 1) // 2)
    h = ((np.float32(1) + np.sqrt(np.float32(1) + np.float32(8) * p.astype(np.float32))) * np.float32(0.5)).astype(np.int64)
    h = np.where(h * (h - 1) // 2 > p, h - 1, h)
    h = np.where((h + 1) * h // 2 <= p, h + 1, h)
    return p - h * (h - 1) // 2, h


def pair_kernel_algorithm(x, n_up, a, n_r, r_max):
    """The pair part of `k_realspace_counts` restated in numpy, step by step -> counts (3, n_r) int64."""
    a = np.asarray(a, dtype=np.float64)
    B = x.shape[0]
    r = np.asarray(x, dtype=np.float64).reshape(B, -1, 3)
    lo, hi = pair_index_decode(r.shape[1])
    f = (r[:, lo] - r[:, hi]) @ np.linalg.inv(a)
    f -= np.floor(f + 0.5)
    best = np.full(f.shape[:2], np.inf)
    for s in SHIFTS5[np.abs(SHIFTS5).max(axis=1) <= 1]:
        v = (f + s) @ a
        best = np.minimum(best, (v * v).sum(axis=-1))
    rr = np.sqrt(best)
    inside = rr < r_max
    k = np.minimum((rr * n_r / r_max).astype(np.int64), n_r - 1)
    chan = np.broadcast_to(np.where(hi < n_up, 0, np.where(lo < n_up, 1, 2)), rr.shape)
    return np.bincount((chan * n_r + k)[inside], minlength=3 * n_r).reshape(3, n_r).astype(np.int64)


def lih_drivers(batch):
    """The LiH fixture network on the device: -> (cell, slogdet net, logdet net, device parameters, walkers (batch, 12))."""
    import torch
    from common import load_case
    from deepsolid_amd import init_guess, network as dnet
    _, cell, klist, net_kw, params = load_case('lih')
    slog = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_slogdet', **net_kw)
    ld = dnet.make_solid_fermi_net(klist=klist, simulation_cell=cell, method_name='eval_logdet', **net_kw)
    dp = {k: [{kk: torch.as_tensor(np.asarray(vv), dtype=torch.float64, device='cuda') for kk, vv in d.items()} for d in v]
          for k, v in params.items()}
    x0 = torch.as_tensor(init_guess.init_electrons(3, cell, cell.a, cell.nelec, batch, init_width=0.8), device='cuda')
    return cell, slog, ld, dp, x0
