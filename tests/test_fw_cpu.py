"""CPU checks of forward walking: the properties of the ancestor tables in the numpy model of
tests/fw_helpers.py, the C-ABI boundary of the three entries, and what `dmc.ForwardWalking` does without a device: its refusals and
a `state_dict` round trip on CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

import fw_helpers as fw
import realspace_helpers as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('ds_dmc_ancestry', 'ds_realspace_counts_w', 'ds_dmc_fw_sums')


def comb_like(rng, B):
    """A parent row as a comb writes it: non-decreasing, some walkers duplicated, some killed."""
    return np.sort(rng.integers(0, B, size=B))


def test_composing_a_block_at_once_equals_composing_it_step_by_step():
    rng = np.random.default_rng(1)
    for B, steps in ((1, 3), (7, 1), (257, 4), (64, 0)):
        parents = np.stack([comb_like(rng, B) for _ in range(steps)]) if steps else np.zeros((0, B), np.int64)
        if steps > 1 and B > 1:
            parents[1, 0], parents[0, B - 1] = -1, B                   # a lost lineage at two depths
        anc = np.stack([np.arange(B), comb_like(rng, B), np.where(np.arange(B) % 3 == 0, -1, np.arange(B))])
        at_once = fw.carry(anc, fw.compose(parents, B))
        by_step = anc
        for k in range(steps):                                         # step 0 first: the tables go forward in time
            by_step = fw.carry(by_step, fw.compose(parents[k:k + 1], B))
        np.testing.assert_array_equal(at_once, by_step)
        # and the map itself, spelled out walker by walker
        P = fw.compose(parents, B)
        for w in range(B):
            p = w
            for k in range(steps - 1, -1, -1):
                p = int(parents[k][p])
                if not 0 <= p < B:
                    p = -1
                    break
            assert P[w] == p


def test_every_walker_has_one_ancestor_or_is_lost_and_ancestors_do_not_multiply():
    rng = np.random.default_rng(2)
    B, n_slots = 96, 6
    anc = np.full((n_slots, B), -1, np.int64)
    for t in range(3 * n_slots):
        parents = np.stack([comb_like(rng, B), np.arange(B)])          # a comb and a step without one
        if t == 7:
            parents[0, 5] = B + 3                                      # garbage: the lineage of walker 5 is lost
        anc = fw.carry(anc, fw.compose(parents, B))
        anc[t % n_slots] = np.arange(B)
        for s in range(n_slots):
            lost = int((anc[s] < 0).sum())
            assert np.bincount(anc[s][anc[s] >= 0], minlength=B).sum() + lost == B
        if t >= n_slots:
            # slot of lag l = (t - l) % n_slots: the number of distinct ancestors does not grow with the lag
            distinct = [len(np.unique(anc[(t - lag) % n_slots][anc[(t - lag) % n_slots] >= 0])) for lag in range(n_slots)]
            assert distinct[0] == B and all(a >= b for a, b in zip(distinct, distinct[1:])), distinct
            assert distinct[-1] < B                                    # (the combs did kill lineages: the check compares something)


def test_identity_parents_leave_the_tables_unchanged():
    rng = np.random.default_rng(3)
    B = 33
    anc = np.stack([comb_like(rng, B), np.full(B, -1), np.arange(B)])
    for steps in (0, 1, 5):
        parents = np.tile(np.arange(B), (steps, 1))
        np.testing.assert_array_equal(fw.compose(parents, B), np.arange(B))
        np.testing.assert_array_equal(fw.carry(anc, fw.compose(parents, B)), anc)


def test_model_of_the_weights_and_the_sums():
    """The quantisation and skip rules of the model itself on the edge weights, and its sums on a case small enough to add by hand."""
    w = np.array([0.0, 1.0, 2.0 ** -20, 255.9, 256.5, np.nan, np.inf, -1.0, 0.5 * 2.0 ** -16, 1.5 * 2.0 ** -16])
    q, bad = fw.quantise(w, 2.0 ** 16, len(w))
    assert q.tolist() == [0, 65536, 0, 16770662, 0, 0, 0, 0, 0, 2]    # ties to even: 0.5 -> 0, 1.5 -> 2
    assert bad.tolist() == [False, False, False, False, True, True, True, True, False, False]
    values = np.array([[1.0, 10.0], [2.0, np.nan], [4.0, 40.0]])
    out, n_bad = fw.fw_sums(values, index=np.array([2, 2, 1, -1, 3, 0, 0]), weight=np.array([0.5, 1.0, 2.0, 1.0, 1.0, np.nan, 0.0]))
    np.testing.assert_array_equal(out, [[0.5 * 4 + 4 + 2 * 2, 3.5], [0.5 * 40 + 40, 1.5]])
    assert n_bad == [2, 2]                                             # -1 and 3; the NaN weight and the NaN value


def test_header_declares_the_entries_and_the_library_exports_them():
    from deepsolid_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    for name in ENTRIES + ('ds_dmc_ancestry_workspace_bytes', 'ds_dmc_fw_sums_workspace_bytes'):
        assert re.search(r'\b' + name + r'\s*\(', code), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # the header's own arithmetic for the workspaces, and what the size functions refuse
    assert lib.ds_dmc_ancestry_workspace_bytes(1025, 4) == 4 * 1025 * 5 and lib.ds_dmc_ancestry_workspace_bytes(3, 0) == 12
    assert lib.ds_dmc_fw_sums_workspace_bytes(257, 3) == 16 * 3 * 2 and lib.ds_dmc_fw_sums_workspace_bytes(256, 1) == 16
    assert lib.ds_dmc_ancestry_workspace_bytes(0, 1) < 0 and lib.ds_dmc_ancestry_workspace_bytes(4, -1) < 0
    assert lib.ds_dmc_fw_sums_workspace_bytes(4, 0) < 0 and lib.ds_dmc_fw_sums_workspace_bytes(4, 65) < 0
    # the conventions are stated where the entries are declared
    for phrase in ('P[w] = parents[0][parents[1][', 'llrint(weight[w] * weight_scale)', 'n_bad[0]', 'q > 2^24', '2^55'):
        assert phrase in src, phrase


def test_refusals_of_the_tracker():
    from deepsolid_amd import dmc
    cell = rh.cubic_cell(2, 1)
    for lags in ((0, -1), (0, 2, 2), (), (0, 1.5)):
        with pytest.raises(ValueError, match='lags'):
            dmc.ForwardWalking(cell, lags=lags)
    with pytest.raises(ValueError, match='weight_scale'):
        dmc.ForwardWalking(cell, weight_scale=0.0)
    # a pair setup that RealSpaceAccumulator refuses, refused in its words
    with pytest.raises(ValueError, match='Wigner-Seitz'):
        dmc.ForwardWalking(cell, pair_bins=8, pair_rmax=5.0)
    with pytest.raises(ValueError, match='pair_bins'):
        dmc.ForwardWalking(cell, pair_bins=2000)
    with pytest.raises(ValueError, match='pair_rmax without pair_bins'):
        dmc.ForwardWalking(cell, pair_rmax=1.0)
    with pytest.raises(ValueError, match='density_grid'):
        dmc.ForwardWalking(cell, density_grid=(300, 2, 2))
    with pytest.raises(ValueError, match='built-in'):
        dmc.ForwardWalking(cell, scalars=('energy', 'pressure'))
    with pytest.raises(ValueError, match='callable'):
        dmc.ForwardWalking(cell, scalars={'mine': 3})
    t = dmc.ForwardWalking(cell, lags=(3, 0), density_grid=4, pair_bins=8)
    assert t.n_slots == 4 and t.lags == (3, 0)
    with pytest.raises(ValueError, match='not one of'):
        t.density(2)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='ROCm device'):
            t.update(None, dict(x=torch.zeros(4, 9, dtype=torch.float64), weight=torch.ones(4, dtype=torch.float64)), None)


def filled_tracker(cell, seed):
    """A tracker in the state three updates of B = 5 walkers would leave, made of CPU tensors by hand."""
    from deepsolid_amd import dmc
    rng = np.random.default_rng(seed)
    t = dmc.ForwardWalking(cell, lags=(0, 2), density_grid=(2, 3, 4), pair_bins=6, scalars={'energy': None, 'mine': lambda arrays: None})
    B, n3, K, L = 5, 9, 3, 2
    t.columns, t.batch, t.n3, t.t = {'energy': (0, 1), 'mine': (1, 2)}, B, n3, 3
    t.ring_x = torch.as_tensor(rng.normal(size=(3, B, n3)))
    t.ring_v = torch.as_tensor(rng.normal(size=(3, B, K)))
    t.anc = torch.as_tensor(rng.integers(-1, B, size=(3, B)).astype(np.int32))
    t.dens = torch.as_tensor(rng.integers(0, 2 ** 40, size=(L, 2, 2, 3, 4)))
    t.pair = torch.as_tensor(rng.integers(0, 2 ** 40, size=(L, 3, 6)))
    t.q_sum = torch.as_tensor(rng.integers(1, 2 ** 40, size=L))
    t.bad = torch.as_tensor(rng.integers(0, 9, size=(L, 2, 2)))
    t.series = [[torch.as_tensor(rng.normal(size=(K, 2))) for _ in range(n)] for n in (3, 1)]
    return t


def test_state_dict_round_trip_on_cpu_tensors(tmp_path):
    from deepsolid_amd import dmc
    cell = rh.cubic_cell(2, 1)
    t = filled_tracker(cell, 4)
    sd = t.state_dict()
    assert all(isinstance(v, np.ndarray) or np.isscalar(v) for v in sd.values())
    u = dmc.ForwardWalking(cell, lags=(0, 2), density_grid=(2, 3, 4), pair_bins=6, scalars={'energy': None, 'mine': lambda arrays: None})
    t.save(tmp_path / 'fw.npz')
    u.load(tmp_path / 'fw.npz')
    sd2 = u.state_dict()
    assert sorted(sd) == sorted(sd2)
    for k in sd:
        a, b = np.asarray(sd[k]), np.asarray(sd2[k])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k       # the same bits
    assert u.anc.dtype == torch.int32 and u.dens.dtype == torch.int64 and u.t == 3 and u.columns == t.columns
    # results come from the loaded buffers: q_sum normalises them
    np.testing.assert_array_equal(u.density_counts(2), t.dens[1].numpy())
    assert np.allclose(u.density(0) * int(t.q_sum[0]), u.density(0) * int(u.q_sum[0]))
    e, err, _ = u.scalar('energy', 0)
    ser = np.stack([r.numpy() for r in t.series[0]])
    assert e == ser[:, 0, 0].sum() / ser[:, 0, 1].sum()
    assert np.asarray(u.scalar('mine', 0)[0]).shape == (2,)
    # merge adds counts and appends series
    m = filled_tracker(cell, 5)
    dens0, n0 = m.dens.clone(), len(m.series[0])
    m.merge(u)
    assert torch.equal(m.dens, dens0 + u.dens) and len(m.series[0]) == n0 + 3 and int(m.q_sum[1]) > int(u.q_sum[1])
    # a state of another setup is refused
    for other in (dmc.ForwardWalking(cell, lags=(0, 3), density_grid=(2, 3, 4), pair_bins=6, scalars={'energy': None, 'mine': len}),
                  dmc.ForwardWalking(cell, lags=(0, 2), density_grid=(2, 3, 5), pair_bins=6, scalars={'energy': None, 'mine': len}),
                  dmc.ForwardWalking(cell, lags=(0, 2), density_grid=(2, 3, 4), pair_bins=6, scalars=('energy',)),
                  dmc.ForwardWalking(rh.cubic_cell(2, 1, edge=8.0), lags=(0, 2), density_grid=(2, 3, 4), pair_bins=6,
                                     scalars={'energy': None, 'mine': len})):
        with pytest.raises(ValueError, match='belongs to another'):
            other.load_state_dict(sd)
    with pytest.raises(ValueError, match='differ'):
        dmc.ForwardWalking(cell, lags=(0, 3), density_grid=(2, 3, 4), pair_bins=6).merge(u)
    u.reduce()
    with pytest.raises(RuntimeError, match='already'):
        u.reduce()
