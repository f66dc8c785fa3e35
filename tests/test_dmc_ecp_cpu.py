"""CPU tests of DMC with a semi-local pseudopotential (locality approximation): the numpy model of dmc_ecp_helpers.py against the
plain model, the oracle-only conditions of the replay fixture that test_gpu_dmc_ecp.py runs, what `make_dmc_step` refuses, and
`DmcState` files with and without the seventh array."""
import numpy as np
import pytest
import torch

import dmc_ecp_helpers as deh
import dmc_helpers as dh
import ecp_helpers as eh


def test_zero_potential_model_equals_the_plain_model_bit_for_bit():
    """A potential whose coefficients are all 0, with explicit cutoffs so that pairs exist: state and rows of the model with the
    pseudopotential are those of dmc_helpers.run_model, bit for bit."""
    B, tau, steps, seed = 6, 0.1, 2, 1
    zero = deh.zero_potential()
    orc = deh.DmcEcpOracle(deh.NAME, zero, seed)
    x0 = dh.start_walkers(deh.NAME, B, seed)
    w0 = dh.preset_weights('ramp', B)
    e_ref, e_cut = -8.0, 0.05 * np.sqrt(orc.n / tau)
    a = dh.run_model(dh.dmc_oracle(deh.NAME), x0, w0, steps, tau, tau, e_ref, e_ref, e_cut, 0, 1, seed, 0)
    b = deh.run_model(orc, x0, w0, steps, tau, tau, e_ref, e_ref, e_cut, 1, seed, 0)
    assert b['pairs0'] > 0 and all(s['pairs'] > 0 for s in b['steps'])
    for k in ('x', 'logabs', 'phase', 'drift', 'eloc', 'weight'):
        assert np.array_equal(a['state'][k], b['state'][k]) and np.array_equal(a['state0'][k], b['state0'][k]), k
    for sa, sb in zip(a['steps'], b['steps']):
        assert np.array_equal(sa['row'], sb['row']) and np.array_equal(sa['acc'], sb['acc']) and np.array_equal(sa['parents'], sb['parents'])
        assert np.all(sb['ecp_row'] == 0)
    assert np.all(b['state']['epp'] == 0)


@pytest.mark.parametrize('name', list(deh.REPLAYS))
def test_the_replay_fixture_meets_its_conditions(name):
    """Over all positions the replay visits, initial and proposed: no pair within CUTOFF_MARGIN of either cutoff; min |A - log u| and
    the tooth distances above the margins of dmc_helpers; no energy within its tolerance of a clip edge; at least one accepted move,
    one rejected move and one duplicated parent.  (Seed from tools/find_dmc_ecp_seeds.py.)  The cases other than lih have a complex
    wavefunction: Im E_nl is not zero there."""
    ref = deh.replay_reference(name)
    c = ref['cond']
    print(c)
    deh.assert_conditions(c)
    assert ref['pairs0'] > 0 and all(s['pairs'] > 0 for s in ref['steps'])
    # the pseudopotential matters: it moves E_L by more than its tolerance on every start walker -- every one that has an ion within
    # a cutoff: lih_twist (cutoff 1.746) has fixture walkers with none, whose triple is exactly zero; on lih there is no such walker
    plain = dh.dmc_oracle(name).evaluate(ref['x0'])[3]
    moved = np.abs(ref['state0']['eloc'] - plain) > 1e-3
    outside = (ref['state0']['epp'] == 0).all(1)
    assert np.all(moved | outside) and 2 * moved.sum() > len(moved) and (name != deh.NAME or moved.all()), (moved, outside)
    if name != deh.NAME:
        assert c['im_e_nl'] > 0, c


def test_make_dmc_step_refuses_other_potentials_before_touching_its_arguments():
    from deepsolid_amd import dmc
    for bad in (object(), 'ccECP', {'local': []}):
        with pytest.raises(NotImplementedError, match='pseudopotential'):
            dmc.make_dmc_step(None, None, 0.01, 1, pseudopotential=bad)


def test_dmc_state_files_carry_epp_and_old_files_load(tmp_path):
    from deepsolid_amd.dmc import DmcState
    g = torch.Generator().manual_seed(3)
    B, n3 = 5, 12
    six = dict(x=torch.randn(B, n3, generator=g, dtype=torch.float64), logabs=torch.randn(B, generator=g, dtype=torch.float64),
               phase=torch.randn(B, 2, generator=g, dtype=torch.float64), drift=torch.randn(B, n3, generator=g, dtype=torch.float64),
               eloc=torch.randn(B, generator=g, dtype=torch.float64), weight=torch.rand(B, generator=g, dtype=torch.float64))
    seven = dict(six, epp=torch.randn(B, 3, generator=g, dtype=torch.float64))
    for arrays, name in ((seven, 'seven'), (six, 'six')):
        s = DmcState({k: v.clone() for k, v in arrays.items()}, e_trial=-1.25, e_ref=-1.5, tau_eff=0.0099, offset=2 ** 40 + 3, valid=True,
                     sum_w=10.5, sum_we=-15.75)
        path = tmp_path / f'{name}.npz'
        s.save(path)
        back = DmcState.load(path, device='cpu')
        assert set(back.arrays) == set(arrays)
        for k, v in arrays.items():
            assert back.arrays[k].dtype == v.dtype and torch.equal(back.arrays[k], v), k
        assert (back.e_trial, back.e_ref, back.tau_eff, back.offset, back.valid, back.sum_w, back.sum_we) == \
            (-1.25, -1.5, 0.0099, 2 ** 40 + 3, True, 10.5, -15.75)
    # a file written before the seventh array existed: exactly the keys the six-array save writes
    with np.load(tmp_path / 'six.npz') as f:
        assert 'epp' not in f.files
