"""numpy model of forward walking (csrc/ds_fw.h, `dmc.ForwardWalking`), shared by test_fw_cpu.py and
test_gpu_fw.py: composition of parent rows with the -1 rule, the ring and the update order of the tracker, integer-weighted
density and pair counts built on the oracles of realspace_helpers, and sums through `dmc_parts_helpers.tree_rows`, which is the
device's summation order bit for bit."""
import numpy as np

import realspace_helpers as rh
from dmc_parts_helpers import tree_rows

MAX_Q = 2 ** 24


# ------------------------------------------------------------------------------------------------------------ ancestor tables
def step_map(P, row):
    """One more (earlier) step under the map P: P'[w] = row[P[w]], -1 where P[w] is -1 or row[P[w]] is outside [0, B)."""
    P, row = np.asarray(P, dtype=np.int64), np.asarray(row, dtype=np.int64)
    B = len(row)
    nxt = np.where(P >= 0, row[np.clip(P, 0, B - 1)], -1)
    return np.where((nxt < 0) | (nxt >= B), -1, nxt)


def compose(parents, B):
    """Block map of `ds_dmc_ancestry`: P[w] = parents[0][parents[1][... parents[steps-1][w]]]; -1 once the chain leaves [0, B)."""
    P = np.arange(B, dtype=np.int64)
    for row in np.asarray(parents, dtype=np.int64).reshape(-1, B)[::-1]:
        P = step_map(P, row)
    return P


def carry(anc, P):
    """anc_s[w] <- anc_s_old[P[w]], -1 where P[w] = -1; an old value is copied as it is (-1 stays -1)."""
    anc, P = np.asarray(anc, dtype=np.int64), np.asarray(P, dtype=np.int64)
    if anc.shape[0] == 0:
        return anc.copy()
    return np.where(P[None, :] >= 0, anc[:, np.clip(P, 0, anc.shape[1] - 1)], -1)


# ----------------------------------------------------------------------------------------------------- who contributes with what
def sources(index, B, B_src):
    """-> (src (B,), ok (B,)): the source row of every walker and whether it lies in [0, B_src)."""
    src = np.arange(B, dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    return src, (src >= 0) & (src < B_src)


def quantise(weight, scale, B):
    """-> (q (B,) int64, bad (B,)): q = rint(weight * scale); bad: a weight that is not finite or negative, or q > 2^24."""
    if weight is None:
        return np.ones(B, dtype=np.int64), np.zeros(B, bool)
    w = np.asarray(weight, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        q = np.rint(w * scale)
        bad = ~np.isfinite(w) | (w < 0) | ~(q <= MAX_Q)
    return np.where(bad, 0, q).astype(np.int64), bad


def counts_w(x_src, n_up, index=None, weight=None, scale=1.0, fold=None, grid=None, a=None, n_r=None, r_max=None, B=None):
    """Model of `ds_realspace_counts_w` -> dict(dens, pair (None when not asked for), q_sum, n_bad [index, weight], margin).  The
    contributing walkers are grouped by their integer weight and each group goes through the oracles of realspace_helpers once,
    multiplied by q.  margin: the smallest edge margin over all source rows (the caller asserts it >= rh.MARGIN)."""
    x_src = np.asarray(x_src, dtype=np.float64)
    B_src = len(x_src)
    B = (len(index) if index is not None else len(weight) if weight is not None else B_src) if B is None else B
    src, ok = sources(index, B, B_src)
    q, bad = quantise(weight, scale, B)
    use = ok & ~bad & (q > 0)
    out = dict(dens=None, pair=None, q_sum=int(q[use].sum()), n_bad=[int((~ok).sum()), int((ok & bad).sum())], margin=np.inf)
    if grid is not None:
        out['dens'] = np.zeros((2,) + tuple(grid), np.int64)
        out['margin'] = min(out['margin'], rh.density_oracle(x_src, n_up, fold, grid)[1])
    if n_r is not None:
        out['pair'] = np.zeros((3, n_r), np.int64)
        if x_src.shape[1] > 3:
            out['margin'] = min(out['margin'], rh.pair_oracle(x_src, n_up, a, n_r, r_max)[1])
    for qv in np.unique(q[use]):
        rows = x_src[src[use & (q == qv)]]
        if grid is not None:
            out['dens'] += int(qv) * rh.density_oracle(rows, n_up, fold, grid)[0]
        if n_r is not None:
            out['pair'] += int(qv) * rh.pair_oracle(rows, n_up, a, n_r, r_max)[0]
    return out


def fw_sums(values, index=None, weight=None, B=None):
    """Model of `ds_dmc_fw_sums` -> (out (K, 2), n_bad [index, weight or value]); the sums go through `tree_rows`."""
    values = np.asarray(values, dtype=np.float64)
    B_src, K = values.shape
    B = (len(index) if index is not None else len(weight) if weight is not None else B_src) if B is None else B
    src, ok = sources(index, B, B_src)
    w = np.ones(B) if weight is None else np.asarray(weight, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        bad_w = ok & (~np.isfinite(w) | (w < 0))
        live = ok & ~bad_w & (w != 0)
    v = values[np.clip(src, 0, B_src - 1)]
    fin = np.isfinite(v)
    use = live[:, None] & fin
    with np.errstate(invalid='ignore', over='ignore'):
        num = np.where(use, w[:, None] * np.where(fin, v, 0.0), 0.0)
    den = np.where(use, w[:, None], 0.0)
    out = np.stack([tree_rows(num), tree_rows(den)], axis=-1)
    return out, [int((~ok).sum()), int(bad_w.sum() + (live[:, None] & ~fin).sum())]


# ------------------------------------------------------------------------------------------------------------------ the tracker
class Tracker:
    """The ring and the update order of `dmc.ForwardWalking`, fed the device's own snapshots, parents and weights."""

    def __init__(self, lags, n_up, scale, fold=None, grid=None, a=None, n_r=None, r_max=None):
        self.lags, self.n_slots, self.n_up, self.scale = tuple(lags), max(lags) + 1, n_up, scale
        self.kw = dict(fold=fold, grid=grid, a=a, n_r=n_r, r_max=r_max)
        self.t = 0
        self.ring_x = self.ring_v = self.anc = None
        L = len(self.lags)
        self.dens = None if grid is None else np.zeros((L, 2) + tuple(grid), np.int64)
        self.pair = None if n_r is None else np.zeros((L, 3, n_r), np.int64)
        self.q_sum = np.zeros(L, np.int64)
        self.bad = np.zeros((L, 2, 2), np.int64)
        self.series = [[] for _ in self.lags]
        self.margin = np.inf
        self.anc_rows = {lag: [] for lag in self.lags}     # the ancestor row every lag used, per block

    def update(self, x, values, parents, weight):
        x, values = np.asarray(x, dtype=np.float64), np.asarray(values, dtype=np.float64)
        B = len(x)
        if self.ring_x is None:
            self.ring_x = np.zeros((self.n_slots,) + x.shape)
            self.ring_v = np.zeros((self.n_slots,) + values.shape)
            self.anc = np.full((self.n_slots, B), -1, np.int64)
        self.anc = carry(self.anc, compose(parents, B))                          # 1. the block's parents
        slot = self.t % self.n_slots
        self.ring_x[slot], self.ring_v[slot], self.anc[slot] = x, values, np.arange(B)      # 2. this block's slot
        for i, lag in enumerate(self.lags):                                      # 3. every lag whose slot exists
            if lag > self.t:
                continue
            s = (self.t - lag) % self.n_slots
            self.anc_rows[lag].append(self.anc[s].copy())
            if self.dens is not None or self.pair is not None:
                c = counts_w(self.ring_x[s], self.n_up, self.anc[s], weight, self.scale, **self.kw)
                self.margin = min(self.margin, c['margin'])
                if self.dens is not None:
                    self.dens[i] += c['dens']
                if self.pair is not None:
                    self.pair[i] += c['pair']
                self.q_sum[i] += c['q_sum']
                self.bad[i, 0] += c['n_bad']
            row, bad = fw_sums(self.ring_v[s], self.anc[s], weight)
            self.bad[i, 1] += bad
            self.series[i].append(row)                                           # 4. the lag's series
        self.t += 1
