"""Shared by test_kfac_cpu.py and test_gpu_kfac.py: a torch-CPU restatement of what the reference's KFAC optimizer
(process.py:209-228: kfac_ferminet_alpha.Optimizer, estimation_mode='fisher_exact') accumulates for every tagged layer.

Every `linear_layer` of the network is a `repeated_dense` block (network.py:430-446, curvature_blocks.py:158-281):
    A = x~^T x~ / (B R),   G = dy^T dy / (B R),   x~ = [x | 1] with a bias,
x (B, R.., d_in) the layer's input, dy (B, R.., d_out) = the pull-back of the seed 1 / sqrt(variance 0.5) = sqrt2 on every
walker's log|psi| to the layer's output (train.py:133, loss_functions.py:529-537, estimator.py:284-330).

`x` is captured on the way through the forward of oracle.network (restated below line by line with the oracle's own
functions, and checked against `oracle.network.eval_func` by test_kfac_cpu.py); `dy` comes from torch.autograd of
sum_b sqrt2 log|psi_b| with respect to each layer's output.  The jaxpr tracer of the reference (tag_graph_matcher, tracer) cannot
run under tools/jax_torch_standin.py, so WHICH layers are blocks and WHAT the seed is are pinned by this restatement only, not by
reference-executed numbers."""
import contextlib
import math

import numpy as np
import torch

from oracle import network as onet

SQRT2 = math.sqrt(2.0)


def block_shapes(params, nelec):
    """[(kind, index, has_bias, d_in incl. bias, d_out, repeats)] from the reference's parameter tree, in the order
    single[0..], double[0..], orbital[0..] (the order of `ds_kfac_layout`)."""
    n = int(sum(nelec))
    active = [int(s) for s in nelec if s > 0]
    out = []
    for l, p in enumerate(params['single']):
        w = np.asarray(p['w'])
        out.append(('single', l, True, w.shape[0] + 1, w.shape[1], n))
    for l, p in enumerate(params['double']):
        w = np.asarray(p['w'])
        out.append(('double', l, True, w.shape[0] + 1, w.shape[1], n * n))
    for c, p in enumerate(params['orbital']):
        w = np.asarray(p['w'])
        out.append(('orbital', c, 'b' in p, w.shape[0] + (1 if 'b' in p else 0), w.shape[1], active[c]))
    return out


def forward_captured(params, x, klist, cell, atoms, spins, envelope_type, full_det, distance_type, taps):
    """oracle.network.solid_fermi_net_orbitals + logdet_matmul for ONE walker, line by line, appending (kind, index, input,
    output) of every linear layer to `taps` (the outputs keep their gradient).  -> log|psi|."""
    def lin(kind, idx, h, p):
        z = h @ p['w']
        if 'b' in p:
            z = z + p['b']
        z.retain_grad()
        taps.append((kind, idx, h, z))
        return z

    ae_, ee_, r_ae, r_ee = onet.construct_periodic_input_features(x, atoms, cell, distance_type)
    ae = torch.cat((r_ae, ae_), dim=2).reshape(ae_.shape[0], -1)
    ee = torch.cat((r_ee, ee_), dim=2)
    to_env = r_ae if envelope_type == 'isotropic' else ae_
    envelope = {'isotropic': onet.isotropic_envelope, 'diagonal': onet.diagonal_envelope, 'full': onet.full_envelope}[envelope_type]

    def residual(a, b):
        return (a + b) / math.sqrt(2.0) if a.shape == b.shape else b

    h_one, h_two = ae, ee
    nd = len(params['double'])
    for i in range(nd):
        h_in = onet.construct_symmetric_features(h_one, h_two, spins)
        h_one_next = torch.tanh(lin('single', i, h_in, params['single'][i]))
        h_two_next = torch.tanh(lin('double', i, h_two, params['double'][i]))
        h_one = residual(h_one, h_one_next)
        h_two = residual(h_two, h_two_next)
    if nd != len(params['single']):
        h_in = onet.construct_symmetric_features(h_one, h_two, spins)
        h_one_next = torch.tanh(lin('single', len(params['single']) - 1, h_in, params['single'][-1]))
        h_to_orb = residual(h_one, h_one_next)
    else:
        h_to_orb = onet.construct_symmetric_features(h_one, h_two, spins)
    hs = [h_to_orb[:spins[0]], h_to_orb[spins[0]:]]
    active = [s for s in spins if s > 0]
    hs = [h for h, s in zip(hs, spins) if s > 0]
    orbitals = []
    for c, (h, p) in enumerate(zip(hs, params['orbital'])):
        o = lin('orbital', c, h, p)
        nparams = p['w'].shape[-1] // 2
        orbitals.append(o[..., :nparams] + 1j * o[..., nparams:])
    envs, off = [], 0
    for s in active:
        envs.append(to_env[off:off + s])
        off += s
    orbitals = [envelope(te, pe) * orb for te, orb, pe in zip(envs, orbitals, params['envelope'])]
    ncol = sum(spins) if full_det else None
    orbitals = [orb.reshape(s, -1, ncol if full_det else s).permute(1, 0, 2) for s, orb in zip(active, orbitals)]
    phases = onet.eval_phase(x, klist, spins, full_det)
    orbitals = [orb * p[None, :, :] for orb, p in zip(orbitals, phases)]
    if full_det:
        orbitals = [torch.cat(orbitals, dim=1)]
    return onet.logdet_matmul(orbitals)[1]


def reference_factors(cell, klist, net_kw, params, x, dtype=None):
    """-> (factors [(A, G)] in the order of `block_shapes`, gradient tree of sum_b sqrt2 log|psi_b| shaped like params,
    log|psi| (B,)) at walkers x (B, 3N), float64 unless `dtype`."""
    ctx = onet.working_dtype(dtype) if dtype is not None else contextlib.nullcontext()
    with ctx:
        rd = dtype or torch.float64
        atoms = onet._t(np.asarray(cell.original_cell.atom_coords()))
        spins = tuple(int(s) for s in cell.nelec)
        lv = []

        def req(o):
            if isinstance(o, dict):
                return {k: req(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return [req(v) for v in o]
            t = o.clone().detach().requires_grad_(True)
            lv.append(t)
            return t
        p = req(onet.params_to_torch(params, dtype))
        xs = torch.as_tensor(np.asarray(x)).to(rd)
        B = xs.shape[0]
        taps, lps = [], []
        for xx in xs:
            t = []
            lps.append(forward_captured(p, xx, klist, cell, atoms, spins, net_kw['envelope_type'], bool(net_kw.get('full_det', False)),
                                        net_kw.get('distance_type', 'nu'), t))
            taps.append(t)
        loss = SQRT2 * torch.stack(lps).sum()
        loss.backward()                 # fills .grad of the parameters and of every tapped layer output
        grads = iter([t.grad for t in lv])

        def build(o):
            if isinstance(o, dict):
                return {k: build(v) for k, v in o.items()}
            if isinstance(o, (list, tuple)):
                return [build(v) for v in o]
            g = next(grads)
            return torch.zeros_like(o) if g is None else g
        gtree = build(p)
        factors = []
        for kind, idx, has_bias, d_in, d_out, repeats in block_shapes(params, spins):
            xi, dy = [], []
            for t in taps:
                h, z = next((h, z) for k, i, h, z in t if k == kind and i == idx)
                xi.append(h.detach().reshape(-1, h.shape[-1]))
                dy.append(z.grad.reshape(-1, z.shape[-1]))
            xi, dy = torch.cat(xi), torch.cat(dy)
            assert xi.shape[0] == B * repeats
            if has_bias:
                xi = torch.cat([xi, torch.ones(xi.shape[0], 1, dtype=xi.dtype)], dim=1)
            assert xi.shape[1] == d_in and dy.shape[1] == d_out
            factors.append((xi.T @ xi / (B * repeats), dy.T @ dy / (B * repeats)))
        return factors, gtree, torch.stack(lps).detach()
