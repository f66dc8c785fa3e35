#!/usr/bin/env python3
"""Generate tests/golden/pretrain.npz by EXECUTING the reference's own pretrain.py (make_pretrain_step, :43-107).

Runs only where the reference checkout is (DEEPSOLID_REFERENCE, as tools/make_golden.py).  The reference's `pretrain` module is
imported under tools/jax_torch_standin.py with `optax`, `absl` and `DeepSolid.hf` stubbed (none is needed by the step:
`optax.apply_updates` = tree add), `pretrain.qmc` replaced by a namespace whose `mh_update` returns its inputs, and a recording
optimizer whose `update` stores `search_direction` and returns zero updates.  `loss_val` and the recorded tree ARE the reference's
`jax.value_and_grad(loss_fn, argnums=1)` over its own network.py.

Per case (tests/pretrain_helpers.GOLDEN_CASES; walkers = the first walkers of the case's own fixture, targets =
pretrain_helpers.make_targets(klist, x, seed + 900)) the file holds, under '<case>:<key>': n_walkers, target_<s>, loss, seed of
oracle.testing.make_test_direction, names / norm / dot per leaf, and 'leaf:<name>' for leaves of <= 4096 entries.  Numbers only.
The archive is written with fixed member timestamps: running the tool twice gives a byte-identical file (checked when the
fixture was made: same sha256 over two runs).
"""
import hashlib
import io
import os
import sys
import types
import zipfile

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

from tools import jax_torch_standin as standin            # noqa: E402
from tools import make_golden as mg                       # noqa: E402

N_WALKERS = 4


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def save_npz_deterministic(path, arrays):
    """np.savez_compressed with sorted members and a fixed timestamp."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())


def main():
    import torch
    mg._install_shim()
    _stub('optax', apply_updates=lambda params, updates: standin.tree_map(lambda p, u: p + u, params, updates),
          adam=lambda lr: None)
    _stub('absl', logging=types.SimpleNamespace(info=lambda *a, **k: None))
    hf = _stub('DeepSolid.hf', SCF=object)
    import DeepSolid
    DeepSolid.hf = hf
    import jax
    from DeepSolid import network as rnet, supercell as rsc, pretrain as rpre
    from deepsolid_amd import systems
    from oracle.testing import CASES, make_test_direction, make_test_params, params_checksum, klist_from_kpts
    from pretrain_helpers import GOLDEN_CASES, leaf_names, leaves, make_targets

    # the move is not part of the fixture: mh_update returns its inputs (the way make_golden.py swaps rham.ewaldsum)
    rpre.qmc = types.SimpleNamespace(mh_update=lambda params, f, x1, key, lp_1, num_accepts, latvec: (x1, key, lp_1, num_accepts))

    class Recording:
        def update(self, search_direction, state, params):
            self.grads = search_direction
            return standin.tree_map(torch.zeros_like, params), state

    d = {}
    for name in GOLDEN_CASES:
        case = CASES[name]
        my_cell = systems.SYSTEMS[case['system']](**case.get('system_kw', {}))
        prim0 = my_cell.original_cell
        prim = mg.FakeCell(prim0.a, prim0.atom_coords(), prim0.atom_charges(), prim0.nelec)
        sim = mg.ref_supercell(rsc, prim, my_cell.S, my_cell.nelec, case.get('sym_type', 'minimal'))
        kpts = rsc.get_supercell_kpts(sim)
        twist = np.asarray(case.get('twist', (0, 0, 0)), float)
        kpts_t = kpts + np.dot(np.linalg.inv(sim.a), np.mod(twist, 1.0)) * 2 * np.pi
        klist = klist_from_kpts(kpts_t, sim.nelec)
        net_kw = dict(systems.DETNET_DEFAULTS); net_kw.update(case.get('net_kw', {}))
        params = make_test_params(case['seed'], prim.atom_coords(), sim.nelec, net_kw)
        fx = np.load(os.path.join(REPO, 'tests', 'golden', name + '.npz'))
        np.testing.assert_allclose(params_checksum(params), fx['params_checksum'], rtol=1e-13)
        nw = min(N_WALKERS, len(fx['x']))
        x = fx['x'][:nw]
        targets = make_targets(klist, x, case['seed'] + 900)
        tprim = mg.TorchCell(prim)
        tsim = mg.TorchCell(sim, original=tprim)
        tklist = [torch.as_tensor(k) for k in klist]
        tparams = mg.to_torch_params(mg.to_np_params(params))
        with standin.torch_mode():
            nets = {m: rnet.make_solid_fermi_net(klist=tklist, simulation_cell=tsim, method_name=m, **net_kw)
                    for m in ('eval_mats', 'eval_slogdet')}
            batch = {m: jax.vmap(n.apply, in_axes=(None, 0), out_axes=0) for m, n in nets.items()}
            opt = Recording()
            step = rpre.make_pretrain_step(batch['eval_mats'], batch['eval_slogdet'], tsim.lattice_vectors(), opt,
                                           full_det=bool(net_kw['full_det']))
            out = step(torch.as_tensor(x), [torch.as_tensor(t) for t in targets], tparams, None, None)
        loss = float(out[3])
        seed = case['seed'] + 900
        vdir = list(leaves(make_test_direction(seed, params)))
        gl = [g.detach().numpy() for g in leaves(opt.grads)]
        names = list(leaf_names(params))
        assert len(gl) == len(names) == len(vdir)
        pre = name + ':'
        d[pre + 'n_walkers'] = np.asarray(nw)
        d[pre + 'seed'] = np.asarray(seed)
        d[pre + 'loss'] = np.asarray(loss)
        d[pre + 'names'] = np.asarray(names)
        d[pre + 'norm'] = np.asarray([float(np.linalg.norm(g)) for g in gl])
        d[pre + 'dot'] = np.asarray([float((g * v).sum()) for g, v in zip(gl, vdir)])
        for s, t in enumerate(targets):
            d[pre + f'target_{s}'] = t
        for n_, g in zip(names, gl):
            if g.size <= 4096:
                d[pre + 'leaf:' + n_] = g
        print(name, 'walkers', nw, 'loss %.12g' % loss, 'max leaf norm %.6g' % d[pre + 'norm'].max())
    path = os.path.join(REPO, 'tests', 'golden', 'pretrain.npz')
    save_npz_deterministic(path, d)
    print(path, '%.1f KB' % (os.path.getsize(path) / 1024), 'sha256', hashlib.sha256(open(path, 'rb').read()).hexdigest())


if __name__ == '__main__':
    main()
