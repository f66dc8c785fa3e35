"""Cases of tests/test_params_cpu.py and the block rule of include/deepsolid_hip.h restated on the host, so that a `ParamMap` can
be built without a system handle.  tests/test_gpu_workspace.py holds `header_blocks` to `ds_param_layout` of a real handle."""
import numpy as np
import torch

from deepsolid_amd import network, systems
from deepsolid_amd.device import device_plan
from deepsolid_amd.params import ParamMap

SMALL = ((64, 16), (64, 16))
ODD = ((40, 20), (56, 24), (56, 7))          # padded one-electron and pair widths, layers without a residual, an unused last pair width
# name -> (system, system_kw, net_kw over DETNET_DEFAULTS): one case per branch of the gather builder
CASES = {
    'lih_plain':        ('lih', {}, dict(hidden_dims=SMALL)),
    'lih_last_bias':    ('lih', {}, dict(hidden_dims=SMALL, use_last_layer=True, bias_orbitals=True)),
    'lih_fulldet_diag': ('lih', {}, dict(hidden_dims=SMALL, full_det=True, envelope_type='diagonal')),
    'lih_fullenv':      ('lih', {}, dict(hidden_dims=SMALL, envelope_type='full')),
    'lih_tri':          ('lih', {}, dict(hidden_dims=SMALL, distance_type='tri')),
    'li_polarized':     ('bcc_li', dict(S=1, nelec=(3, 0)), dict(hidden_dims=SMALL)),
    'lih_odd':          ('lih', {}, dict(hidden_dims=ODD)),
}
# the default widths: only the SHA-256 of the gather vector is committed
DIGEST_CASES = {
    'lih_default':    ('lih', {}, {}),
    'bcc_li_default': ('bcc_li', {}, {}),
}
DTYPES = {'f64': torch.float64, 'f32': torch.float32}


def case_net(name):
    """-> (simulation cell, klist, net_kw) of a case."""
    system, system_kw, kw = {**CASES, **DIGEST_CASES}[name]
    cell, klist = systems.build(system, **system_kw)
    net_kw = dict(systems.DETNET_DEFAULTS)
    net_kw.update(kw)
    return cell, klist, net_kw


def arch(cell, net_kw):
    """The architecture facts `ParamMap` takes, as `DeviceSystem.__init__` derives them (needs the built library: `device_plan`)."""
    nelec = tuple(int(n) for n in cell.nelec)
    if nelec[0] == 0 and nelec[1] > 0:
        nelec = (nelec[1], 0)
    hidden = tuple(tuple(int(v) for v in h) for h in net_kw['hidden_dims'])
    natom = np.asarray(cell.original_cell.atom_coords()).reshape(-1, 3).shape[0]
    nf = 4 if net_kw['distance_type'] == 'nu' else 7
    use_last = bool(net_kw['use_last_layer'])
    device_dims, _ = device_plan(hidden, nf * natom, nf, len(hidden) - (0 if use_last else 1))
    return dict(nelec=nelec, n_det=int(net_kw['determinants']), hidden_dims=hidden, device_dims=device_dims, natom=natom,
                distance_type=net_kw['distance_type'], envelope_type=net_kw['envelope_type'], full_det=bool(net_kw['full_det']),
                use_last_layer=use_last, bias_orbitals=bool(net_kw['bias_orbitals']))


def header_blocks(a):
    """[(offset, rows, cols)] and the element count by the rule of include/deepsolid_hip.h (`ds_param_layout`): the blocks in the
    header's order with padded shapes, every block starting at a multiple of 16 elements."""
    r4 = lambda v: (v + 3) // 4 * 4
    nf = 4 if a['distance_type'] == 'nu' else 7
    nch = 2 if a['nelec'][1] > 0 else 1
    n_layers = len(a['hidden_dims'])
    h1 = [r4(nf * a['natom'])] + [d[0] for d in a['device_dims']]
    h2 = [r4(nf)] + [d[1] for d in a['device_dims']]
    shapes = []
    for l in range(n_layers):
        shapes += [(h1[l] + nch * h2[l], h1[l + 1]), (nch * h1[l], h1[l + 1]), (1, h1[l + 1])]
    for l in range(n_layers - (0 if a['use_last_layer'] else 1)):
        shapes += [(h2[l], h2[l + 1]), (1, h2[l + 1])]
    for c in range(nch):
        nparam = (sum(a['nelec']) if a['full_det'] else a['nelec'][c]) * a['n_det']
        cols = (2 * nparam + 63) // 64 * 64
        shapes.append((h1[-1] + (nch * h2[-1] if a['use_last_layer'] else 0), cols))
        if a['use_last_layer']:
            shapes.append((nch * h1[-1], cols))
        if a['bias_orbitals']:
            shapes.append((1, 2 * nparam))
        shapes.append((a['natom'], nparam))
        shapes.append(({'isotropic': 1, 'diagonal': 3, 'full': 9}[a['envelope_type']] * a['natom'], nparam))
    blocks, off = [], 0
    for rows, cols in shapes:
        blocks.append((off, rows, cols))
        off = (off + rows * cols + 15) // 16 * 16
    return blocks, off


def make_tree(cell, net_kw, seed=5, dtype=torch.float64):
    """A random parameter tree of CPU tensors with the reference's shapes (network.py:60-186)."""
    kw = {k: net_kw[k] for k in ('envelope_type', 'bias_orbitals', 'use_last_layer', 'full_det', 'hidden_dims', 'determinants',
                                 'distance_type')}
    tree = network.init_solid_fermi_net_params(seed, atoms=cell.original_cell.atom_coords(), spins=tuple(int(s) for s in cell.nelec),
                                               dtype=dtype, **kw)
    rng = np.random.default_rng(seed + 1)
    for env in tree['envelope']:                     # ones in the reference's init: make every entry its own
        for k in env:
            env[k] = torch.as_tensor(rng.standard_normal(tuple(env[k].shape)), dtype=dtype)
    return tree


def param_map(name, dtype):
    """-> (ParamMap laid out by `header_blocks`, cell, net_kw)."""
    cell, _, net_kw = case_net(name)
    a = arch(cell, net_kw)
    blocks, count = header_blocks(a)
    return ParamMap(dtype=dtype, blocks=blocks, param_count=count, **a), cell, net_kw
