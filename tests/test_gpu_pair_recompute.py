"""Pair layer 1 of a float64 energy chain runs pair layer 0 in registers (k_two_layer_expand<double, NT2, true, PREV>): layer 0
(network.py:525-528 without residual, 4 'nu' or 8 'tri' input features) then writes the pair-mean rows of the next one-electron
layer only, and level 1 of the pair stream is never in memory.  The recomputed level is the same MFMA k-steps, bias and tanh chain
rule on the same operands, element (a, c, r) of the accumulators being the operand the lane used to load: with
DS_NO_PAIR_RECOMPUTE=1 (layer 0 writes its output, layer 1 reads it) the local energies must be IDENTICAL to the last bit."""
import numpy as np
import pytest
import torch

from deepsolid_amd import systems
from oracle.testing import make_test_params

from common import load_case

pytestmark = pytest.mark.gpu


def dev_params(params, dtype=torch.float64):
    return {k: [{kk: torch.as_tensor(vv, dtype=dtype, device='cuda') for kk, vv in d.items()} for d in v]
            for k, v in params.items()}


def energies(monkeypatch, cell, klist, net_kw, params, x, dtype=torch.float64):
    """-> {switch: kinetic energies}, {switch: pair layers that recompute} for DS_NO_PAIR_RECOMPUTE unset (None) and set ('1')"""
    from deepsolid_amd.device import DeviceSystem
    from deepsolid_amd.ewaldsum import EwaldTables
    monkeypatch.delenv('DS_I8', raising=False)
    dp = dev_params(params, dtype)
    xd = torch.as_tensor(x, dtype=dtype, device='cuda')
    out, ran = {}, {}
    for flag in (None, '1'):
        if flag:
            monkeypatch.setenv('DS_NO_PAIR_RECOMPUTE', flag)
        else:
            monkeypatch.delenv('DS_NO_PAIR_RECOMPUTE', raising=False)
        sysd = DeviceSystem(cell, klist, net_kw, EwaldTables(cell), dtype)
        ran[flag] = sysd.pair_recompute_layers()
        assert sysd.pair_recompute_layers(dump=True) == 0
        out[flag] = sysd.local_energy(dp, xd)[0]
    return out, ran


# bcc-Li 2x2x2: 24 pairs per electron in two waves, the second half idle (and layer 0 goes from two electrons per workgroup to one);
# LiH: one partly filled wave; graphene: 48 pairs, three full waves; Li (3, 0): one spin channel; 'tri': 8 pair features, two
# k-steps of layer 0; use_last_layer: layer 1 writes its output (into the buffer layer 0 left unwritten) for the orbital head
@pytest.mark.parametrize('name', ['bcc_li', 'lih', 'graphene', 'li_polarized', 'lih_tri', 'lih_lastlayer'])
def test_recomputed_pair_layer_gives_identical_energies(name, monkeypatch):
    fx, cell, klist, net_kw, params = load_case(name)
    nw = min(3, len(fx['x']))
    out, ran = energies(monkeypatch, cell, klist, net_kw, params, fx['x'][:nw])
    assert ran == {None: 1, '1': 0}, ran
    assert torch.isfinite(out[None]).all()
    assert torch.equal(out[None], out['1'])


def test_recomputed_pair_layer_with_unequal_spin_counts(monkeypatch):
    """bcc-Li primitive cell with (3, 2) electrons: the two partner-spin means of an electron run over different counts."""
    cell, klist = systems.build('bcc_li', nelec=(3, 2))
    net_kw = dict(systems.DETNET_DEFAULTS)
    params = make_test_params(29, cell.original_cell.atom_coords(), cell.nelec, net_kw)
    out, ran = energies(monkeypatch, cell, klist, net_kw, params, systems.synthetic_walkers(cell, 3, seed=23))
    assert ran == {None: 1, '1': 0}, ran
    assert torch.isfinite(out[None]).all()
    assert torch.equal(out[None], out['1'])


@pytest.mark.parametrize('name', ['bcc_li', 'graphene'])
def test_recomputed_pair_layer_vs_reference_kinetic_energies(name, monkeypatch):
    """... and against numbers the repository did not make: the reference-executed kinetic energies of the golden fixtures."""
    from deepsolid_amd.device import DeviceSystem
    from deepsolid_amd.ewaldsum import EwaldTables
    fx, cell, klist, net_kw, params = load_case(name)
    monkeypatch.delenv('DS_I8', raising=False)
    monkeypatch.delenv('DS_NO_PAIR_RECOMPUTE', raising=False)
    nw = min(4, len(fx['ke_ref']))
    sysd = DeviceSystem(cell, klist, net_kw, EwaldTables(cell), torch.float64)
    assert sysd.pair_recompute_layers() == 1
    ke = torch.view_as_complex(sysd.local_energy(dev_params(params), torch.as_tensor(fx['x'][:nw], device='cuda'))[0]).cpu().numpy()
    for b in range(nw):
        assert abs(ke[b] - fx['ke_ref'][b]) < 1e-9 * max(1.0, abs(fx['ke_ref'][b])), (b, ke[b], fx['ke_ref'][b])


def test_float32_and_stage_dumps_keep_the_level_in_memory(monkeypatch):
    """A float32 handle never recomputes (its accumulator rows sit in other lanes than its operands), and a stage dump shows level 1
    of the pair stream as before: identical float32 energies and identical 'h2_1' / 'h2_2' dumps with the switch either way."""
    from deepsolid_amd.device import DeviceSystem
    from deepsolid_amd.ewaldsum import EwaldTables
    fx, cell, klist, net_kw, params = load_case('bcc_li')
    out, ran = energies(monkeypatch, cell, klist, net_kw, params, fx['x'][:2], torch.float32)
    assert ran == {None: 0, '1': 0}, ran
    assert torch.isfinite(out[None]).all()
    assert torch.equal(out[None], out['1'])
    dp = dev_params(params)
    x = torch.as_tensor(fx['x'][:2], device='cuda')
    N = sum(cell.nelec)
    n_h2 = 2 * 32 * 5 * ((N * N + 15) // 16 * 16)
    dumps = {}
    for flag in (None, '1'):
        if flag:
            monkeypatch.setenv('DS_NO_PAIR_RECOMPUTE', flag)
        else:
            monkeypatch.delenv('DS_NO_PAIR_RECOMPUTE', raising=False)
        sysd = DeviceSystem(cell, klist, net_kw, EwaldTables(cell), torch.float64)
        assert sysd.pair_recompute_layers(dump=True) == 0
        dumps[flag] = [sysd.debug_stage(dp, x, st, n_h2).clone() for st in ('h2_1', 'h2_2')]
    for a, b in zip(dumps[None], dumps['1']):
        assert a.numel() == n_h2 and torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
