"""CPU checks of the KFAC factor pass (csrc/ds_kfac.h, `ds_kfac_factors`): the C-ABI boundary and the torch restatement the
GPU tests compare against (tests/kfac_helpers.py).

The placement of the blocks and the seed are pinned by that restatement only: the reference's jaxpr tracer cannot run outside
JAX, so there are no reference-executed numbers for them.  What is checked here is that the restatement IS the oracle's forward
(same log|psi| to round-off, same parameter gradient as autograd over `oracle.network.eval_func`) and that its factors have the
structure curvature_blocks.py:158-281 prescribes.

`ds_kfac_layout` itself is not called here: it reads a system handle, and creating one allocates on the device.  The layout of
the built library against `kfac_helpers.block_shapes` is checked for every factor case of tests/test_gpu_kfac.py."""
import os
import re

import numpy as np
import pytest
import torch

import kfac_helpers as kh
from common import load_case, oracle_net
from deepsolid_amd import systems
from oracle.network import params_to_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('ds_kfac_block_count', 'ds_kfac_layout', 'ds_kfac_workspace_bytes', 'ds_kfac_factors')


def test_kfac_symbols_exported_and_declared():
    from deepsolid_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
        assert re.search(r'\b%s\s*\(' % n, src), f'{n} is not declared in include/deepsolid_hip.h'


def test_kfac_block_struct_matches_header():
    from deepsolid_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'deepsolid_hip.h')).read()
    body = src[src.index('typedef struct ds_kfac_block {'):src.index('} ds_kfac_block;')].split('{', 1)[1]
    fields = []
    for decl in body.split(';'):
        for part in decl.strip().split(','):
            m = re.search(r'([A-Za-z_][A-Za-z0-9_]*)\s*(\[[^\]]*\])?\s*$', part.strip())
            if m:
                fields.append(m.group(1))
    assert fields == [f[0] for f in _lib.KfacBlock._fields_]
    import ctypes as C
    assert C.sizeof(_lib.KfacBlock) == 56           # ten int32 fields, two int64 offsets, no padding


@pytest.mark.parametrize('name', ['lih', 'lih_lastlayer', 'li_polarized', 'lih_bias',
                                  'lih_twist',          # complex k-points
                                  'bcc_li_fulldet',     # one determinant over both spin channels
                                  'bcc_li_333'])        # unequal non-empty spin channels (41, 40)
def test_restatement_is_the_oracle_forward(name):
    """kfac_helpers.forward_captured against oracle.network: log|psi| to round-off, the gradient of sum_b sqrt2 log|psi_b| against
    autograd over the oracle's own eval_func; the factors are symmetric, positive semi-definite on the diagonal and carry the
    bias corner A[-1, -1] = 1 (x~ ends in a one for every repeat)."""
    fx, cell, klist, net_kw, params = load_case(name)
    x = systems.synthetic_walkers(cell, 2, seed=5)
    factors, gtree, lp = kh.reference_factors(cell, klist, net_kw, params, x)
    net = oracle_net(cell, klist, net_kw, 'eval_slogdet')
    lv = []

    def req(o):
        if isinstance(o, dict):
            return {k: req(v) for k, v in o.items()}
        if isinstance(o, (list, tuple)):
            return [req(v) for v in o]
        t = o.clone().detach().requires_grad_(True)
        lv.append(t)
        return t
    p = req(params_to_torch(params))
    ref = torch.stack([net.apply(p, torch.as_tensor(xx)) for xx in x])
    assert float((ref.detach() - lp).abs().max()) <= 1e-12 * max(1.0, float(ref.detach().abs().max()))
    (kh.SQRT2 * ref.sum()).backward()
    from pretrain_helpers import leaves
    for g, t in zip(leaves(gtree), leaves(p)):
        r = t.grad if t.grad is not None else torch.zeros_like(t)
        assert float((g - r).abs().max()) <= 1e-12 * max(float(r.abs().max()), 1e-300)
    shapes = kh.block_shapes(params, cell.nelec)
    assert len(shapes) == len(params['single']) + len(params['double']) + len(params['orbital']) == len(factors)
    for (kind, idx, has_bias, d_in, d_out, rep), (A, G) in zip(shapes, factors):
        assert tuple(A.shape) == (d_in, d_in) and tuple(G.shape) == (d_out, d_out)
        assert torch.equal(A, A.T) or float((A - A.T).abs().max()) <= 1e-15 * float(A.abs().max())
        assert float(A.diagonal().min()) >= 0 and float(G.diagonal().min()) >= 0
        if has_bias:
            assert abs(float(A[-1, -1]) - 1.0) <= 1e-14


def test_block_shapes_follow_the_parameter_tree():
    """d_in counts the reference's concatenated input row [h | spin means | pair means | 1] with empty spin channels dropped
    (network.py:327-328): li_polarized has one channel, lih two; repeats are N, N^2 and n_s."""
    fx, cell, klist, net_kw, params = load_case('lih')
    s = kh.block_shapes(params, cell.nelec)
    assert s[0][:2] == ('single', 0) and s[0][3] == 3 * 8 + 2 * 4 + 1 and s[0][5] == 4
    assert s[1][3] == 3 * 256 + 2 * 32 + 1 and s[1][4] == 256
    dbl = [b for b in s if b[0] == 'double']
    assert dbl[0][3] == 5 and dbl[0][5] == 16 and dbl[-1][3] == 33
    orb = [b for b in s if b[0] == 'orbital']
    assert len(orb) == 2 and orb[0][2] is False and orb[0][3] == 256 and orb[0][5] == 2
    fx, cell, klist, net_kw, params = load_case('li_polarized')
    s = kh.block_shapes(params, cell.nelec)
    assert s[1][3] == 2 * 256 + 32 + 1 and len([b for b in s if b[0] == 'orbital']) == 1
